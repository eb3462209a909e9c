"""Long attention (csrc/attention_long.hip) at its launch-plan edges, on boundary-weighted and on large scores, against float64.

tests/test_attention_long.py pins the shipped shapes; this file reaches the branches it leaves out.  References are the float64 formula of
tests/test_ops_parity.py (_attention_ref, _temporal_tables) and float64 autograd.  The bars are that file's: 1e-4 forward, 2e-4 backward.
The backward is compared in FOUR parts, each against its own largest reference magnitude: dq (columns 0:256), dk (256:512), dv (512:768)
and dbias - one scale for all of dqkv would let the largest part hide the others.  Every destination (out, stats, dqkv, dbias, the
workspace) is handed over NaN-filled and must come back without a NaN: `torch.empty` would hand a kernel the previous call's values.

Branch -> shape that reaches it (ids without the backend):
  a. every length class, backward (bias + rotary): L = 65 (one live token in the last key tile), 80 (L % 16 == 0, second query tile of
     the last block dead), 96 (L % 32 == 0), 97, 112, 127, 128, 129, 200, 255, 256; scalar bias reads at L % 4 != 0; b = 2 x hw = 3 up
     to 129 (batch boundary in `seq_rows`), b = 1 above          test_backward_length_classes[<L>], test_forward_lengths[97|112]
  b. phase KV's sequence walk g, g + G, ... with the bias gradient carried in LDS: G - 1, G, G + 1, 2 G + 1 sequences at L = 65
     (G = 51; 52 = 2 batches x 26 pixels); G + 1 at L = 128 (G = 32), 129 (28, ragged, scalar bias), 256 (16: sixteen key blocks of 16 KB
     tiles).  Each runs twice: same bits                         test_backward_kv_trips[<L>-<b>-<hw>]
  c. `bias_vec` false with L % 4 == 0: a bias view 4 bytes past a 16-byte boundary, forward and phase Q, L = 128 and 256; the same
     bits as the aligned call                                    test_unaligned_bias[<L>]
  d. mode 1 with a bias and rotary tables of length hw and `row0 = seq * hw` across batches: (b, frames, hw) = (2, 3, 65), (2, 3, 100),
     (2, 3, 256)                                                 test_spatial_with_tables[<hw>]
  e. the optional operands one at a time: none | bias alone (kv_kernel<true>, `unrotate` a no-op) | rotary alone (kv_kernel<false> with
     `unrotate`), L = 96 and 129                                 test_backward_optional_operands[<L>-<which>], test_forward_optional_operands_129
     refused with nothing written: rot_cos without rot_sin, bias without dbias, dbias without bias, mode 2, a workspace one byte short,
     a workspace not 16-byte aligned                             test_c_level_refusals
  f. forward statistics: L = 65, 128, 256 in mode 0, hw = 100 in mode 1; every element replaced; `out` the same bits with and without
                                                                 test_forward_statistics_edges[<mode>-<L>]
  g. boundary-weighted softmax: the temporal bias + 12 at key L - 1 for even queries and at key 0 for odd ones (e^12 = 1.6e5 against at
     most 255 other keys of weight O(1): almost all of a row's mass on the first or on the last live key, so a dropped or shifted
     boundary key is an O(1) error, not O(1 / L)), L = 65, 96, 129, 255       test_boundary_keys[<L>]
  h. large scores: the q and k columns x QK_SCALE = 4, the scores x 16 (standard deviation 16: fast_exp far into its underflow, and in
     phase KV `s - m` slightly positive where the MFMA operand order differs from the sweep that took the maximum), L = 65, 129, 256
                                                                 test_large_scores[<L>]
  i. the same backward on a NaN-filled and on a zero-filled workspace: same bits      test_workspace_independence
  j. autograd.AttentionCL above 64 tokens: the bits of train_ops.attention_long_bwd   test_autograd_routes_long[<L>]

ADMISSION of QK_SCALE (the rule of tests/test_attention_fast_math.py): a factor is admitted only where the FLOAT32 TORCH FORMULA on exactly
these inputs (b = 2, hw = 3, seeds 1 and 3) stays within a tenth of the bar from float64 - 1e-5 forward, 2e-5 for each backward part - so
that the bar cannot hide an error of the kernels behind the conditioning of the inputs.  Measured on the CPU:
  factor 4: forward 6.0e-6 (L = 65), 3.6e-6 (129), 4.2e-6 (256); backward, worst part 2.7e-6 (dq, 65), 4.9e-6 (dk, 129), 4.8e-6 (dk, 256): admitted
  factor 8: forward 1.75e-5 (65), 1.56e-5 (129), 1.30e-5 (256); backward up to 2.2e-5 (dq, 256): not admitted
The test asserts the admission before it looks at the kernel: a change of torch's float32 arithmetic shows as an admission failure.

ACHIEVED on the MI355X (LFDM_PARITY_LOG; the largest fraction of its bar over the comparisons of each group): a 0.0075 (dv, L = 200) | b 0.0080
(dk, 52 sequences of 65) | c 0.0075 (out, 128) | d 0.0061 (dk, hw 256) | e 0.0051 (out, 129, bias alone) | f 0.0075 (out, 128) | g 0.094 (dbias,
65) | h 0.039 (out, 256) | j 0.0067 (dbias, 65).  Under the emulator (expf and IEEE divisions): at most 0.009 in
a - f and j, g 0.083 (the same dbias), h 0.046 (out, 129): what g and h use of their bars is the conditioning of the inputs in float32, not
the hardware exponential."""
import functools

import pytest
import torch

import lfdm_oracle as O
from cvpr23_lfdm_amd import autograd as AG
from cvpr23_lfdm_amd import ops, train_ops
from test_ops_parity import _attention_ref, _temporal_tables
from util import assert_close, rnd

TOL_FWD = 1e-4       # tests/test_attention_long.py TOL_FWD
TOL_BWD = 2e-4       # tests/test_attention_long.py TOL_BWD
QK_SCALE = 4.0       # group h; admitted by the rule in the docstring
BOUNDARY = 12.0      # group g
NAN = float("nan")
PARTS = (("dq", 0, 256), ("dk", 256, 512), ("dv", 512, 768))


def _nan(shape, dev):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device=dev)


def _written(t, what):
    assert not bool(torch.isnan(t).any()), "%s: NaN left in the destination (elements the kernel never wrote)" % what


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        assert (x is None) == (y is None), what
        if x is not None:
            assert torch.equal(x, y), "%s: two calls on the same inputs differ" % what


def _at_offset(t, rem):
    """A dense copy of t whose first byte lies `rem` bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    off = ((rem - buf.data_ptr()) % 16) // 4
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == rem and view.is_contiguous()
    return view


def _formula(qkv32, dout32, bias32, rot64, mode, dtype, grads):
    """The torch formula in `dtype` on float32 inputs -> out rows of 256 and, with `grads`, autograd's dqkv rows of 768 and dbias."""
    qkv = qkv32.to(dtype).requires_grad_(grads)
    bias = None if bias32 is None else bias32.to(dtype).requires_grad_(grads)
    rot = None if rot64 is None else (rot64[0].to(dtype), rot64[1].to(dtype))
    if mode == 0:
        out = _attention_ref(qkv.permute(0, 2, 1, 3), bias, rot).permute(0, 2, 1, 3).reshape(-1, 256)
    else:
        out = _attention_ref(qkv, bias, rot).reshape(-1, 256)
    dqkv = dbias = None
    if grads:
        out.backward(dout32.to(dtype))
        dqkv = qkv.grad.reshape(-1, 768)
        dbias = None if bias is None else bias.grad
    return out.detach(), dqkv, dbias


def _part_errors(dqkv, dbias, ref_dqkv, ref_dbias):
    """{part: largest error / largest reference magnitude of that part}"""
    res = {}
    for name, lo, hi in PARTS:
        r = ref_dqkv[:, lo:hi].double()
        res[name] = float((dqkv[:, lo:hi].double().cpu() - r).abs().max() / r.abs().max())
    if ref_dbias is not None:
        res["dbias"] = float((dbias.double().cpu() - ref_dbias.double()).abs().max() / ref_dbias.abs().max())
    return res


@functools.lru_cache(maxsize=None)
def _case(mode, b, frames, hw, bias=True, rot=True, qk=1.0, boundary=False, grads=True):
    """Inputs, float64 output and float64 autograd gradients of one shape: computed once, shared by every test that needs it, never
    modified.  mode 0: sequences over the frames of a pixel; mode 1: over the pixels of a frame; the tables have the sequence's length
    in both.  qk: factor on the q and k columns.  boundary: BOUNDARY added to the bias at the first / last key (group g).  With qk != 1
    the float32 formula's own errors against float64 ride along as `admission`."""
    L = frames if mode == 0 else hw
    qkv32 = rnd(b, frames, hw, 768, seed=1)
    qkv32[..., :512] *= qk
    dout = rnd(b * frames * hw, 256, seed=3)
    bias64, rot64, _ = _temporal_tables(L, "cpu")
    kw = {}
    bias32 = None
    if bias:
        bias32 = bias64.float().contiguous()
        if boundary:
            bias32[:, 0::2, L - 1] += BOUNDARY
            bias32[:, 1::2, 0] += BOUNDARY
        kw["bias"] = bias32
    if rot:
        kw["rot_cos"], kw["rot_sin"] = rot64[0][:, 0::2].float().contiguous(), rot64[1][:, 0::2].float().contiguous()
    else:
        rot64 = None
    out, dqkv, dbias = _formula(qkv32, dout, bias32, rot64, mode, torch.float64, grads)
    admission = None
    if qk != 1.0:
        o32, g32, d32 = _formula(qkv32, dout, bias32, rot64, mode, torch.float32, grads)
        admission = dict(fwd=float((o32.double() - out).abs().max()) / max(1.0, float(out.abs().max())))
        if grads:
            admission.update(_part_errors(g32, d32, dqkv, dbias))
    return dict(mode=mode, dims=(b, frames, hw), L=L, qkv4=qkv32, qkv=qkv32.reshape(-1, 768).contiguous(), kw=kw, bias32=bias32, rot64=rot64,
                out=out, dout=dout, dqkv=dqkv, dbias=dbias, admission=admission)


def _dev_kw(c, dev):
    return {k: v.to(dev) for k, v in c["kw"].items()}


def _forward(c, dev, kw=None, stats=None):
    """attention_long_cl into a NaN-filled destination."""
    b, frames, hw = c["dims"]
    out = ops.attention_long_cl(c["qkv"].to(dev), b, frames, hw, c["mode"], out=_nan(c["out"].shape, dev), stats=stats,
                                **(_dev_kw(c, dev) if kw is None else kw))
    _written(out, "out")
    return out


def _backward(c, dev, kw=None, ws_fill=NAN):
    """attention_long_bwd into NaN-filled dqkv and dbias, on a workspace of exactly the required size filled with `ws_fill`.  The row
    statistics at the head of the workspace are always written in full (zeros for the padding queries), the bias partials with a bias."""
    b, frames, hw = c["dims"]
    kw = _dev_kw(c, dev) if kw is None else kw
    nbytes = ops._lib().lfdm_attention_long_bwd_ws_bytes(b, frames, hw, c["mode"])
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4,), ws_fill, dtype=torch.float32, device=dev)
    with_bias = kw.get("bias") is not None
    dqkv, dbias = train_ops.attention_long_bwd(c["qkv"].to(dev), c["dout"].to(dev), b, frames, hw, c["mode"], dqkv=_nan(c["qkv"].shape, dev),
                                               dbias=_nan((8, c["L"], c["L"]), dev) if with_bias else None, ws=ws, **kw)
    _written(dqkv, "dqkv")
    nseq = b * hw if c["mode"] == 0 else b * frames
    nstat = nseq * 8 * 3 * ((c["L"] + 15) // 16 * 16)
    if with_bias:
        _written(dbias, "dbias")
        _written(ws, "workspace")
    else:
        assert dbias is None
        _written(ws[:nstat], "row statistics")
    return dqkv, dbias


def _check_fwd(c, out, what):
    assert_close(out.cpu(), c["out"], TOL_FWD, what + " out")


def _check_bwd(c, dqkv, dbias, what, ref=None):
    """dq, dk, dv and dbias each against its own largest reference magnitude."""
    ref_dqkv, ref_dbias = (c["dqkv"], c["dbias"]) if ref is None else ref
    got = dqkv.cpu()
    for name, lo, hi in PARTS:
        r = ref_dqkv[:, lo:hi]
        sc = float(r.abs().max())
        assert sc > 0
        assert_close(got[:, lo:hi] / sc, r / sc, TOL_BWD, "%s %s" % (what, name))
    if ref_dbias is None:
        assert dbias is None
        return
    sc = float(ref_dbias.abs().max())
    assert_close(dbias.cpu() / sc, ref_dbias / sc, TOL_BWD, what + " dbias")


# ---------------------------------------------------------------- a. every length class
LENGTHS = [65, 80, 96, 97, 112, 127, 128, 129, 200, 255, 256]


@pytest.mark.parametrize("L", LENGTHS)
def test_backward_length_classes(backend, L):
    dev = backend
    c = _case(0, 2 if L <= 129 else 1, L, 3)
    dqkv, dbias = _backward(c, dev)
    _check_bwd(c, dqkv, dbias, "a. long attention backward L=%d" % L)


@pytest.mark.parametrize("L", [97, 112])
def test_forward_lengths(backend, L):
    dev = backend
    c = _case(0, 2, L, 3)
    _check_fwd(c, _forward(c, dev), "a. long attention L=%d" % L)


# ---------------------------------------------------------------- b. phase KV trips
@pytest.mark.parametrize("L,b,hw", [(65, 2, 25), (65, 1, 51), (65, 2, 26), (65, 1, 103), (128, 1, 33), (129, 1, 29), (256, 1, 17)])
def test_backward_kv_trips(backend, L, b, hw):
    """G - 1, G, G + 1 and 2 G + 1 sequences at L = 65 (G = 51); G + 1 at 128, 129 and 256.  All of them run on both backends: the largest,
    256 x 17 twice, takes about ten seconds under the emulator."""
    dev = backend
    c = _case(0, b, L, hw)
    first = _backward(c, dev)
    _check_bwd(c, *first, "b. long attention backward L=%d, %d sequences" % (L, b * hw))
    _same_bits(first, _backward(c, dev), "long attention backward L=%d, %d sequences" % (L, b * hw))


# ---------------------------------------------------------------- c. unaligned bias
@pytest.mark.parametrize("L", [128, 256])
def test_unaligned_bias(backend, L):
    """L % 4 == 0 with a bias 4 bytes past a 16-byte boundary: the forward and phase Q read it by scalars.  Same values, same
    arithmetic: the bits of the aligned call."""
    dev = backend
    c = _case(0, 2 if L == 128 else 1, L, 3)
    kw = _dev_kw(c, dev)
    aligned, shifted = dict(kw, bias=_at_offset(kw["bias"], 0)), dict(kw, bias=_at_offset(kw["bias"], 4))
    out_a, out_s = _forward(c, dev, kw=aligned), _forward(c, dev, kw=shifted)
    _check_fwd(c, out_s, "c. long attention L=%d, unaligned bias" % L)
    assert torch.equal(out_a, out_s), "forward: the unaligned bias gives other bits than the aligned one"
    bwd_a, bwd_s = _backward(c, dev, kw=aligned), _backward(c, dev, kw=shifted)
    _check_bwd(c, *bwd_s, "c. long attention backward L=%d, unaligned bias" % L)
    _same_bits(bwd_a, bwd_s, "backward, aligned against unaligned bias")


# ---------------------------------------------------------------- d. mode 1 with tables and several batches
@pytest.mark.parametrize("hw", [65, 100, 256])
def test_spatial_with_tables(backend, hw):
    dev = backend
    c = _case(1, 2, 3, hw)
    _check_fwd(c, _forward(c, dev), "d. long spatial attention with tables hw=%d" % hw)
    dqkv, dbias = _backward(c, dev)
    _check_bwd(c, dqkv, dbias, "d. long spatial attention backward with tables hw=%d" % hw)


# ---------------------------------------------------------------- e. optional operands, refusals
WHICH = {"none": (False, False), "bias": (True, False), "rotary": (False, True)}


@pytest.mark.parametrize("which", list(WHICH))
@pytest.mark.parametrize("L", [96, 129])
def test_backward_optional_operands(backend, L, which):
    dev = backend
    bias, rot = WHICH[which]
    c = _case(0, 2, L, 3, bias=bias, rot=rot)
    dqkv, dbias = _backward(c, dev)
    _check_bwd(c, dqkv, dbias, "e. long attention backward L=%d, tables: %s" % (L, which))


def test_forward_optional_operands_129(backend):
    dev = backend
    for which, (bias, rot) in WHICH.items():
        c = _case(0, 2, 129, 3, bias=bias, rot=rot, grads=False)
        _check_fwd(c, _forward(c, dev), "e. long attention L=129, tables: %s" % which)


def test_c_level_refusals(backend):
    """What the C entry points refuse, each with an error code and nothing written to any destination."""
    dev = backend
    b, L, hw = 1, 65, 1
    c = _case(0, b, L, hw, grads=False)
    kw = _dev_kw(c, dev)
    lib = ops._lib()
    p, st = ops._p, ops._stream(lib)
    need = lib.lfdm_attention_long_bwd_ws_bytes(b, L, hw, 0)
    qkv, dout = c["qkv"].to(dev), c["dout"].to(dev)
    out, dqkv, dbias = _nan((L, 256), dev), _nan((L, 768), dev), _nan((8, L, L), dev)
    ws = _at_offset(_nan((need // 4 + 4,), dev), 0)
    ws_off = _at_offset(_nan((need // 4 + 4,), dev), 4)
    bias, cos, sin = kw["bias"], kw["rot_cos"], kw["rot_sin"]

    def bwd(mode=0, bias=bias, cos=cos, sin=sin, dbias=dbias, ws=ws, nbytes=need):
        return lib.lfdm_attention_long_bwd_cl_f32(p(qkv), p(dout), p(dqkv), b, L, hw, mode, p(bias), p(cos), p(sin), p(dbias), p(ws), nbytes, st)

    def fwd(mode=0, cos=cos, sin=sin):
        return lib.lfdm_attention_long_cl_f32(p(qkv), p(out), b, L, hw, mode, p(bias), p(cos), p(sin), None, st)

    refused = {
        "backward, rot_cos without rot_sin": (lambda: bwd(sin=None), -1, b"attention_long_bwd"),
        "backward, rot_sin without rot_cos": (lambda: bwd(cos=None), -1, b"attention_long_bwd"),
        "backward, bias without dbias": (lambda: bwd(dbias=None), -1, b"dbias iff bias"),
        "backward, dbias without bias": (lambda: bwd(bias=None), -1, b"dbias iff bias"),
        "backward, mode 2": (lambda: bwd(mode=2), -1, b"attention_long_bwd"),
        "backward, workspace one byte short": (lambda: bwd(nbytes=need - 1), -3, b"workspace"),
        "backward, workspace not 16-byte aligned": (lambda: bwd(ws=ws_off), -3, b"workspace"),
        "backward, no workspace": (lambda: bwd(ws=None), -3, b"workspace"),
        "forward, rot_cos without rot_sin": (lambda: fwd(sin=None), -1, b"attention_long"),
        "forward, mode 2": (lambda: fwd(mode=2), -1, b"attention_long"),
    }
    for what, (call, code, text) in refused.items():
        assert call() == code, what
        assert text in lib.lfdm_last_error(), (what, lib.lfdm_last_error())
    for name, t in dict(out=out, dqkv=dqkv, dbias=dbias, ws=ws, ws_off=ws_off).items():
        assert bool(torch.isnan(t).all()), "a refused call wrote to " + name
    assert bwd() == 0 and fwd() == 0            # the same arguments, complete: accepted
    _written(dqkv, "dqkv")
    _written(out, "out")


# ---------------------------------------------------------------- f. forward statistics
def _stats_ref(c):
    """float64 row maxima and row sums of exp(s - max), (nseq * 8, L) each."""
    tokens = c["qkv4"].double().permute(0, 2, 1, 3) if c["mode"] == 0 else c["qkv4"].double()
    q, k, _ = tokens.chunk(3, dim=-1)
    heads = lambda z: z.reshape(*z.shape[:-1], 8, 32).transpose(-2, -3)
    q, k = heads(q) * 32 ** -0.5, heads(k)
    if c["rot64"] is not None:
        q, k = O.apply_rotary(q, *c["rot64"]), O.apply_rotary(k, *c["rot64"])
    sim = q @ k.transpose(-1, -2)
    if c["bias32"] is not None:
        sim = sim + c["bias32"].double()
    m = sim.amax(dim=-1)
    return m.reshape(-1, c["L"]), (sim - m.unsqueeze(-1)).exp().sum(dim=-1).reshape(-1, c["L"])


@pytest.mark.parametrize("mode,L", [(0, 65), (0, 128), (0, 256), (1, 100)])
def test_forward_statistics_edges(backend, mode, L):
    """stats [(sequence, head)][max | sum][L] with L no multiple of 16 (65, 100) and at the limit; every element replaced; the output does
    not depend on whether the statistics are asked for."""
    dev = backend
    c = _case(0, 2 if L < 256 else 1, L, 3) if mode == 0 else _case(1, 2, 3, L)
    m, ssum = _stats_ref(c)
    stats = _nan((m.shape[0], 2, L), dev)
    out = _forward(c, dev, stats=stats)
    assert bool(torch.isfinite(stats).all()), "stats: an element was not replaced or is not finite"
    assert_close(stats[:, 0].cpu(), m, TOL_FWD, "f. long attention row maxima mode %d L=%d" % (mode, L))
    assert_close(stats[:, 1].cpu(), ssum, TOL_FWD, "f. long attention row sums mode %d L=%d" % (mode, L))
    _check_fwd(c, out, "f. long attention with statistics mode %d L=%d" % (mode, L))
    assert torch.equal(out, _forward(c, dev)), "out differs with and without stats"


# ---------------------------------------------------------------- g. boundary-weighted softmax
@pytest.mark.parametrize("L", [65, 96, 129, 255])
def test_boundary_keys(backend, L):
    dev = backend
    c = _case(0, 2, L, 3, boundary=True)
    _, ssum = _stats_ref(c)
    # sum of exp(s - max) = 1 / p(largest key): median 1.001 - 1.003 over the rows, at most 1.84 (L = 255)
    assert float(ssum.median()) < 1.01 and float(ssum.max()) < 2.0, "the boundary key does not dominate its row"
    _check_fwd(c, _forward(c, dev), "g. long attention, boundary keys L=%d" % L)
    dqkv, dbias = _backward(c, dev)
    _check_bwd(c, dqkv, dbias, "g. long attention backward, boundary keys L=%d" % L)


# ---------------------------------------------------------------- h. large scores
@pytest.mark.parametrize("L", [65, 129, 256])
def test_large_scores(backend, L):
    dev = backend
    c = _case(0, 2, L, 3, qk=QK_SCALE)
    adm = c["admission"]
    assert adm["fwd"] <= TOL_FWD / 10, "admission: the float32 torch formula is %.2e from float64 on these inputs" % adm["fwd"]
    for part in ("dq", "dk", "dv", "dbias"):
        assert adm[part] <= TOL_BWD / 10, "admission: float32 torch %s is %.2e from float64 on these inputs" % (part, adm[part])
    out = _forward(c, dev)
    assert bool(torch.isfinite(out).all())
    _check_fwd(c, out, "h. long attention, qk x %g L=%d" % (QK_SCALE, L))
    dqkv, dbias = _backward(c, dev)
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(dbias).all())
    _check_bwd(c, dqkv, dbias, "h. long attention backward, qk x %g L=%d" % (QK_SCALE, L))


# ---------------------------------------------------------------- i. workspace independence
def test_workspace_independence(backend):
    """Nothing the backward reads from its workspace is anything but what the same call wrote there: L = 129 (fifteen padding queries in
    the row statistics, which phase KV loads)."""
    dev = backend
    c = _case(0, 2, 129, 3)
    _same_bits(_backward(c, dev, ws_fill=NAN), _backward(c, dev, ws_fill=0.0), "backward on a NaN-filled against a zero-filled workspace")


# ---------------------------------------------------------------- j. autograd
@pytest.mark.parametrize("L", [65, 129])
def test_autograd_routes_long(backend, L):
    """autograd.AttentionCL sends more than 64 tokens to the long pair: the forward's bits, and gradients that are the bits of
    train_ops.attention_long_bwd and lie within the bar of float64."""
    dev = backend
    b, hw = 2, 3
    c = _case(0, b, L, hw)
    kw = _dev_kw(c, dev)
    qkv, bias = c["qkv"].to(dev).requires_grad_(True), kw["bias"].clone().requires_grad_(True)
    out = AG.AttentionCL.apply(qkv, bias, kw["rot_cos"], kw["rot_sin"], b, L, hw, 0)
    assert torch.equal(out.detach(), _forward(c, dev))
    out.backward(c["dout"].to(dev))
    _same_bits((qkv.grad, bias.grad), _backward(c, dev), "AttentionCL.backward against attention_long_bwd")
    _check_bwd(c, qkv.grad, bias.grad, "j. AttentionCL backward L=%d" % L)
