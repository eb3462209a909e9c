"""Training (backward) kernels at the edges of their launch plans, against float64 torch autograd on the CPU of the ATen graph the
reference model builds.  tests/test_train_ops.py and tests/test_autograd.py pin the shapes the shipped configurations use; this file
takes the branches next to them: the second trip of a capped grid-stride loop, ragged last blocks, the narrowest and widest rows, every
template instantiation at both ends of its range, non-square images and filters.  The shapes are the smallest that reach each branch and
are the same on both backends ("emu": index logic on a GPU-less machine; "hip": what only the device shows - ordering between the phases
of a wave-private LDS tile, prefetches across trips).

Bars are the project's own: test_train_ops.TOL for kernel entry points (parameter gradients divided by the reference's largest
magnitude), test_autograd.TOL through autograd.py.  Every destination the entry points accept is handed over NaN-filled: a row a kernel
forgot to write stays NaN instead of holding a previous call's values.  The cases marked `twice` run a second time on the same
inputs and must give the same bits: the kernels promise a fixed summation order without float atomics, and on the device a race shows
up first as a run that disagrees with itself.  The coverage table is in tests/test_ops_parity.py."""
import os

import pytest
import torch
import torch.nn.functional as F

from cvpr23_lfdm_amd import autograd as A
from cvpr23_lfdm_amd import train_ops
from test_autograd import _cmp
from test_train_ops import TOL, _attention_ref
from util import assert_close, from_cl, rnd, to_cl

NAN = float("nan")


def _nan(shape, dev):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device=dev)


def _written(t, what):
    assert not bool(torch.isnan(t).any()), "%s: NaN left in the destination (elements the kernel never wrote)" % what


def _scaled(got, ref, what):
    """a parameter gradient: compared relative to the reference's largest magnitude"""
    sc = float(ref.abs().max()) + 1e-30
    assert_close(got.cpu() / sc, ref / sc, TOL, what)


def _same_bits(first, second, what):
    for i, (a, b) in enumerate(zip(first, second)):
        if a is not None:
            assert torch.equal(a, b), "%s: output %d differs between two runs on the same inputs" % (what, i)


# ------------------------------------------------------------------------------------------------------------------------------------
# a. / b.  lfdm_attention_bwd_cl_f32 beyond one trip of its grid-stride loop (attn_bwd_blocks: 2048 wavefronts per trip)

# batch 3 x hw 86 = 258 sequences = 2064 (sequence, head) units: one full trip, then a trip of 16 live units and 2032 invalid ones.
# frames: both ends of <16,4> (4, 16), <32,4> (17, 32), <48,4,40> (33, 40), <48,4> (41, 48), <64,2> (49, 64).
# (40, 257): 771 sequences, four trips.  (1, 100): dbias exactly zero.
@pytest.mark.parametrize("frames,hw,twice", [(4, 86, False), (16, 86, False), (17, 86, False), (32, 86, False), (33, 86, False),
                                             (40, 86, False), (41, 86, False), (48, 86, False), (49, 86, False), (64, 86, False),
                                             (40, 257, True), (1, 100, False)])
def test_attention_temporal_bwd_trips(backend, frames, hw, twice):
    import lfdm_oracle as O
    dev = backend
    b = 3
    qkv32 = rnd(b, frames, hw, 768, seed=1)
    qkv = qkv32.double().requires_grad_(True)
    bias32 = O.rel_pos_bias(rnd(32, 8, seed=2), frames)
    bias = bias32.double().clone().requires_grad_(True)
    freqs = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))
    cos, sin = O.rotary_tables(freqs, frames)
    out = _attention_ref(qkv.permute(0, 2, 1, 3), bias, (cos.double(), sin.double())).permute(0, 2, 1, 3).reshape(-1, 256)
    dout = rnd(*out.shape, seed=3)
    out.backward(dout.double())
    ops_in = (qkv32.reshape(-1, 768).to(dev), dout.to(dev))
    tables = dict(bias=bias32.contiguous().to(dev), rot_cos=cos[:, 0::2].contiguous().to(dev), rot_sin=sin[:, 0::2].contiguous().to(dev))

    def run():
        return train_ops.attention_bwd(*ops_in, b, frames, hw, 0, dqkv=_nan(ops_in[0].shape, dev), dbias=_nan((8, frames, frames), dev),
                                       **tables)

    dqkv, dbias = run()
    _written(dqkv, "temporal attention dqkv")
    _written(dbias, "temporal attention dbias")
    assert_close(dqkv.cpu(), qkv.grad.reshape(-1, 768), TOL, "temporal attention dqkv")
    if frames == 1:
        # one key per query: the softmax is the constant 1, the bias has no gradient (and no scale to normalise by)
        assert float(bias.grad.abs().max()) == 0.0
        assert float(dbias.cpu().abs().max()) == 0.0, "temporal attention dbias at one frame"
    else:
        _scaled(dbias, bias.grad, "temporal attention dbias")
    if twice:
        _same_bits((dqkv, dbias), run(), "temporal attention backward")


# (2, 130, 17): 260 sequences = 2080 units of <32,4>; (1, 257, 64): 2056 units of <64,2> (no prefetch: rows fetched at the top of the unit)
@pytest.mark.parametrize("b,frames,hw", [(2, 130, 17), (1, 257, 64)])
def test_attention_spatial_bwd_trips(backend, b, frames, hw):
    dev = backend
    qkv32 = rnd(b, frames, hw, 768, seed=3)
    qkv = qkv32.double().requires_grad_(True)
    out = _attention_ref(qkv, None, None).reshape(-1, 256)
    dout = rnd(*out.shape, seed=4)
    out.backward(dout.double())
    dqkv, none = train_ops.attention_bwd(qkv32.reshape(-1, 768).to(dev), dout.to(dev), b, frames, hw, 1, dqkv=_nan((b * frames * hw, 768), dev))
    assert none is None
    _written(dqkv, "spatial attention dqkv")
    assert_close(dqkv.cpu(), qkv.grad.reshape(-1, 768), TOL, "spatial attention dqkv")


# ------------------------------------------------------------------------------------------------------------------------------------
# c.  lfdm_linear_attention_bwd_cl_f32: token blocks of LA_TOK = 64 with ragged tails, the 4-token inner trip

@pytest.mark.parametrize("hw", [1, 2, 3, 63, 64, 65, 127, 130])
def test_linear_attention_bwd_token_edges(backend, hw):
    dev = backend
    nf = 3
    qkv32 = rnd(nf, hw, 768, seed=4)
    qkv = qkv32.double().requires_grad_(True)
    q, k, v = [z.reshape(nf, hw, 8, 32).permute(0, 2, 3, 1) for z in qkv.chunk(3, dim=-1)]  # b h d n
    q = q.softmax(dim=-2) * (32 ** -0.5)
    k = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).permute(0, 3, 1, 2).reshape(nf * hw, 256)
    dout = rnd(*out.shape, seed=5)
    out.backward(dout.double())
    dqkv = train_ops.linear_attention_bwd(qkv32.reshape(-1, 768).to(dev), dout.to(dev), nf, hw, dqkv=_nan((nf * hw, 768), dev))
    _written(dqkv, "linear attention dqkv")
    _scaled(dqkv, qkv.grad.reshape(-1, 768), "linear attention dqkv")


# ------------------------------------------------------------------------------------------------------------------------------------
# d.  lfdm_groupnorm_silu_bwd_cl_f32 and the training forward

# (batch, C, pixels, groups).  nchunk2 = ceil(pixels / 32) capped at 256 is the trip count of gn_bwd_finalize_kernel's four interleaved
# chunk ranges: 1 (pixels 1, 3, 5, 7, 31), 2 (33, 37, 40), 4 (100), 5 (160), 7 (208), 13 (416), 14 (417), 16 (512), 17 (513, 544),
# 66 (2100), 256 (8193: `per` = 33 with an empty tail of chunks; 9000: ragged `per`).  C = 4: one float4 column, 256 pixel rows per
# sweep; C = 1024: one sweep of 256 columns.  groups 16 / 64: the multi-pass gn_merge_stats.  batch 9 / 8: the `batch >= 8` cap of the
# apply grid (128 blocks: reached by (8, 128, 2100, 8)); (2, 256, 2100, 8): the 1024 / batch cap.
GN_CASES = [(1, 4, 1, 1), (2, 4, 5, 1), (2, 32, 31, 8), (2, 32, 33, 8), (1, 32, 513, 8), (2, 32, 544, 8), (2, 128, 208, 8), (3, 64, 417, 1),
            (1, 64, 8193, 8), (1, 64, 9000, 8), (9, 64, 40, 8), (8, 128, 2100, 8), (2, 256, 100, 16), (1, 256, 3, 64), (1, 512, 7, 64),
            (1, 1024, 37, 8), (2, 32, 160, 8), (2, 32, 416, 8), (2, 32, 512, 8), (2, 256, 2100, 8)]
GN_TWICE = (8, 128, 2100, 8)


@pytest.mark.parametrize("b,c,pixels,groups", GN_CASES)
@pytest.mark.parametrize("with_ss,silu,with_res", [(True, True, False), (False, False, True)])
def test_groupnorm_bwd_edges(backend, b, c, pixels, groups, with_ss, silu, with_res):
    dev = backend
    x32 = rnd(b, c, pixels, seed=1)
    g32, be32 = 1 + 0.2 * rnd(c, seed=2), 0.1 * rnd(c, seed=3)
    ss32 = 0.3 * rnd(b, 2 * c, seed=4) if with_ss else None
    r32 = rnd(b, c, pixels, seed=6) if with_res else None
    x, gamma, beta = x32.double().requires_grad_(True), g32.double().requires_grad_(True), be32.double().requires_grad_(True)
    ss = ss32.double().requires_grad_(True) if with_ss else None
    y = F.group_norm(x, groups, gamma, beta, eps=1e-5)
    if with_ss:
        y = y * (ss[:, :c].view(b, c, 1) + 1) + ss[:, c:].view(b, c, 1)
    if silu:
        y = F.silu(y)
    if with_res:
        y = y + r32.double()
    dy = rnd(*y.shape, seed=5)
    y.backward(dy.double())
    rows = lambda v: v.detach().permute(0, 2, 1).reshape(-1, c).contiguous()
    xd, dyd = rows(x32).to(dev), rows(dy).to(dev)
    gd, bd = g32.to(dev), be32.to(dev)
    ssd = ss32.to(dev) if with_ss else None
    rd = rows(r32).to(dev) if with_res else None

    def run():
        yk, partial, nchunk = train_ops.groupnorm_silu_train(xd, b, gd, bd, scale_shift=ssd, residual=rd, groups=groups, silu=silu,
                                                             out=_nan(xd.shape, dev))
        dx, dg, db, dss = train_ops.groupnorm_silu_bwd(xd, dyd, b, gd, bd, partial, nchunk, scale_shift=ssd, groups=groups, silu=silu,
                                                       dgb=_nan((2, c), dev), dx=_nan(xd.shape, dev),
                                                       dss=_nan((b, 2 * c), dev) if with_ss else None)
        return yk, dx, dg, db, dss

    yk, dx, dg, db, dss = run()
    for t, what in ((yk, "gn y"), (dx, "gn dx"), (dg, "gn dgamma"), (db, "gn dbeta")) + (((dss, "gn dscale_shift"),) if with_ss else ()):
        _written(t, what)
    assert (dss is not None) == with_ss
    assert_close(yk.cpu(), rows(y), TOL, "gn y")
    assert_close(dx.cpu(), rows(x.grad), TOL, "gn dx")
    _scaled(dg, gamma.grad, "gn dgamma")
    _scaled(db, beta.grad, "gn dbeta")
    if with_ss:
        _scaled(dss, ss.grad, "gn dscale_shift")
    if (b, c, pixels, groups) == GN_TWICE:
        _same_bits((yk, dx, dg, db, dss), run(), "groupnorm forward + backward")


def test_groupnorm_refuses_96_channels(backend):
    """C / 4 = 24 float4 columns do not divide the 256 threads of a sweep: refused by the forward and by the backward before anything
    is launched, and no destination is touched."""
    dev = backend
    b, c, pixels = 2, 96, 9
    x, dy = rnd(b * pixels, c, seed=1).to(dev), rnd(b * pixels, c, seed=2).to(dev)
    gamma, beta, ss = torch.ones(c, device=dev), torch.zeros(c, device=dev), torch.zeros(b, 2 * c, device=dev)
    y = _nan(x.shape, dev)
    with pytest.raises(RuntimeError, match=r"groupnorm: unsupported shape \(need C%G==0, \(C/G\)%4==0, 256%\(C/4\)==0\)"):
        train_ops.groupnorm_silu_train(x, b, gamma, beta, scale_shift=ss, out=y)
    nchunk = train_ops.gn_forward_chunks(pixels)
    partial = torch.zeros(b * nchunk * 8 * 2, device=dev)
    dx, dgb, dss = _nan(x.shape, dev), _nan((2, c), dev), _nan((b, 2 * c), dev)
    with pytest.raises(RuntimeError, match=r"groupnorm_bwd: bad arguments \(C%4==0, C<=1024, C/4 divides 256\)"):
        train_ops.groupnorm_silu_bwd(x, dy, b, gamma, beta, partial, nchunk, scale_shift=ss, dgb=dgb, dx=dx, dss=dss)
    for t in (y, dx, dgb, dss):
        assert bool(torch.isnan(t).all()), "a refused call wrote to its destination"


# ------------------------------------------------------------------------------------------------------------------------------------
# e.  lfdm_layernorm_bwd_add_cl_f32

# (rows, C).  layernorm_bwd_kernel: one row per wavefront, a lane holds float4 columns lane, lane + 64, ...: C / 4 = 1 (4), 63 (252),
# 64 (256), 65 (260), 129 (516), 256 (1024); layernorm_bwd_small_kernel<16> (C = 64: four rows per wavefront) and <32> (C = 128: two).
# The grid is min(ceil(rows / 4), 512) blocks of four wavefronts: 4101 x 8, 2049 x 516 (general kernel, 2048 rows per trip), 16395 x 64
# (8192 rows per trip) and 8195 x 128 (4096 rows per trip) make every wavefront take more than one trip, with a ragged last one.
@pytest.mark.parametrize("rows,c,twice", [(1, 4, False), (3, 252, False), (5, 256, False), (5, 260, False), (2, 1024, False), (9, 64, False),
                                          (5, 128, False), (4101, 8, False), (2049, 516, False), (16395, 64, True), (8195, 128, False)])
@pytest.mark.parametrize("add", [False, True])
def test_layernorm_bwd_edges(backend, rows, c, twice, add):
    dev = backend
    x32, g32, dy, extra = rnd(rows, c, seed=1), 1 + 0.2 * rnd(c, seed=2), rnd(rows, c, seed=3), rnd(rows, c, seed=4)
    x, gamma = x32.double().requires_grad_(True), g32.double().requires_grad_(True)
    mean = x.mean(dim=1, keepdim=True)
    var = x.var(dim=1, unbiased=False, keepdim=True)
    y = (x - mean) / (var + 1e-5).sqrt() * gamma          # reference LayerNorm
    y.backward(dy.double())
    want_dx = x.grad + extra.double() if add else x.grad
    xd, dyd, gd, ad = x32.to(dev), dy.to(dev), g32.to(dev), extra.to(dev) if add else None

    def run():
        return train_ops.layernorm_bwd(xd, dyd, gd, dgamma=_nan((c,), dev), dx_add=ad, dx=_nan((rows, c), dev))

    dx, dg = run()
    _written(dx, "ln dx")
    _written(dg, "ln dgamma")
    assert_close(dx.cpu(), want_dx, TOL, "ln dx" + (" + dx_add" if add else ""))
    _scaled(dg, gamma.grad, "ln dgamma")
    if twice:
        _same_bits((dx, dg), run(), "layernorm backward")


# ------------------------------------------------------------------------------------------------------------------------------------
# f.  lfdm_conv2d_wgrad_cl_f32 on non-square images and filters

# (cin, cout, k, stride, pad, n, hi, wi, route).  route "wgrad3": conv_wgrad3_kernel (wgrad_plan: 3x3 / stride 1 / pad 1, hi % 4 == 0,
# >= 32 channels both sides, >= 32 pixel tiles), else conv_wgrad_kernel<wm, wn> with wm / wn = 2 from 96 channels on.
WGRAD_CASES = [
    (64, 64, 3, 1, (1, 1), 16, 4, 16, "wgrad3"),       # <8>: 32 tiles of 8 x 4 pixels on a 4 x 16 image
    (32, 40, 3, 1, (1, 1), 32, 8, 4, "wgrad3"),        # <4>: two images per tile, partial cout tile
    (36, 32, 3, 1, (1, 1), 22, 4, 12, "wgrad3"),       # <4>: 33 tiles over ragged splits, partial cin tile
    (8, 12, 3, 1, (1, 1), 3, 5, 9, "tap"),             # <1, 1> on an odd non-square image
    (8, 100, 3, 1, (1, 1), 2, 7, 3, "tap"),            # <1, 2> under default routing
    (8, 8, 4, 2, (1, 1), 3, 6, 10, "tap"),             # stride 2
    (8, 8, 4, 2, (1, 1), 2, 7, 9, "tap"),              # stride 2 on an odd input (7 x 9 -> 3 x 4)
    (20, 24, 3, 2, (1, 1), 3, 9, 5, "tap"),            # 3x3 under stride 2
    (12, 8, 3, 1, (1, 0), 2, 5, 6, "tap"),             # padding in y only: wq = wi - 2
    (8, 12, (1, 3), 1, (0, 1), 2, 4, 7, "tap"),        # 1 x 3 filter
    (256, 256, 3, 1, (1, 1), 1, 4, 4, "tap"),          # <2, 2>; wgrad_reduce_ref_kernel<4>: ceil(cin / 4) * ceil(cout / 64) = 256
    (64, 1024, 3, 1, (1, 1), 1, 2, 2, "tap"),          # <1, 2>; wgrad_reduce_ref_kernel<4>: 16 * 16 = 256
    (16, 16, 5, 1, (2, 2), 1, 3, 11, "tap"),           # 25 taps: tap-major only
]
WGRAD_TWICE = (36, 32)


@pytest.mark.parametrize("cin,cout,k,stride,pad,n,hi,wi,route", WGRAD_CASES)
def test_conv_wgrad_edges(backend, cin, cout, k, stride, pad, n, hi, wi, route):
    dev = backend
    kh, kw = (k, k) if isinstance(k, int) else k
    x = rnd(n, cin, hi, wi, seed=1)
    w = (rnd(cout, cin, kh, kw, seed=2) * 0.1).double().requires_grad_(True)
    y = F.conv2d(x.double(), w, stride=stride, padding=pad)
    dy = rnd(*y.shape, seed=3)
    y.backward(dy.double())
    hq, wq = y.shape[2], y.shape[3]
    xd, dyd = to_cl(x).to(dev), to_cl(dy).to(dev)
    geom = (n, hi, wi, hq, wq, kh, kw)

    def run():
        dw = train_ops.conv_wgrad(xd, dyd, *geom, stride=stride, pad=pad)
        if kh * kw > 16:
            return dw, None, None
        out, db = _nan((cout, cin, kh, kw), dev), _nan((cout,), dev)
        train_ops.conv_wgrad(xd, dyd, *geom, stride=stride, pad=pad, out=out, ci_off=0, dbias=db)
        return dw, out, db

    dw, out, db = run()
    _scaled(dw.view(kh, kw, cin, cout).permute(3, 2, 0, 1), w.grad, "wgrad, tap-major")
    if out is not None:
        _written(out, "wgrad, reference layout")
        _written(db, "bias sums from the wgrad pass")
        _scaled(out, w.grad, "wgrad, reference layout")
        _scaled(db, dy.double().sum(dim=(0, 2, 3)), "bias sums from the wgrad pass")
    if route == "wgrad3":
        os.environ["LFDM_WGRAD3"] = "0"
        try:
            old = train_ops.conv_wgrad(xd, dyd, *geom, stride=stride, pad=pad)
        finally:
            del os.environ["LFDM_WGRAD3"]
        _scaled(old.view(kh, kw, cin, cout).permute(3, 2, 0, 1), w.grad, "wgrad, tap-major, per-tap kernel")
        sc = float(w.grad.abs().max())
        assert_close(old.cpu() / sc, dw.cpu() / sc, TOL, "per-tap kernel vs nine-tap kernel")
        # the two kernels tile the pixel rows differently: the same bits from both mean the knob chose nothing, i.e. the default route of this
        # case was the per-tap kernel already
        assert not torch.equal(old, dw), "this case did not take the nine-tap route"
    if (cin, cout) == WGRAD_TWICE:
        _same_bits((dw, out, db), run(), "weight gradient")


# ------------------------------------------------------------------------------------------------------------------------------------
# g.  lfdm_colsum_f32: blocks of 1024 rows, capped at 512 blocks

# above 512 * 1024 rows a block takes ceil(rows / 512) rows instead of 1024: 525317 rows = 1027 per block with a short last block (C = 4:
# one float4 column), 525312 = 1026 per block exactly.  (1025, 68): two blocks, the second with one row; two column tiles of 64, one partial
@pytest.mark.parametrize("rows,c,twice", [(525317, 4, True), (525312, 8, False), (1025, 68, False)])
def test_colsum_block_cap(backend, rows, c, twice):
    dev = backend
    x = rnd(rows, c, seed=1)
    xd = x.to(dev)
    got = train_ops.colsum(xd, out=_nan((c,), dev))
    _written(got, "colsum")
    _scaled(got, x.double().sum(0), "colsum")
    if twice:
        _same_bits((got,), (train_ops.colsum(xd, out=_nan((c,), dev)),), "colsum")


# ------------------------------------------------------------------------------------------------------------------------------------
# h.  lfdm_upsample2_pad_cl_f32, forward and adjoint

@pytest.mark.parametrize("n,c,h,w,pad,reflect", [(1, 4, 1, 1, 1, True), (2, 8, 1, 5, 1, True), (2, 4, 5, 1, 0, False), (1, 12, 2, 3, 1, False),
                                                 (3, 4, 4, 7, 0, True)])
def test_upsample2_pad_edges(backend, n, c, h, w, pad, reflect):
    dev = backend
    x32 = rnd(n, c, h, w, seed=1)
    x = x32.double().requires_grad_(True)
    ref = F.interpolate(x, scale_factor=2, mode="nearest")
    if pad:
        ref = F.pad(ref, (pad,) * 4, mode="reflect" if reflect else "constant")
    dy = rnd(*ref.shape, seed=2)
    ref.backward(dy.double())
    ho, wo = 2 * h + 2 * pad, 2 * w + 2 * pad
    y = train_ops.upsample2_pad(to_cl(x32).to(dev), n, h, w, pad, reflect, out=_nan((n * ho * wo, c), dev))
    _written(y, "upsample + pad")
    assert_close(y.cpu(), to_cl(ref.detach()), TOL, "upsample + pad")
    dx = train_ops.upsample2_pad(to_cl(dy).to(dev), n, h, w, pad, reflect, backward=True, out=_nan((n * h * w, c), dev))
    _written(dx, "upsample + pad, adjoint")
    assert_close(dx.cpu(), to_cl(x.grad), TOL, "upsample + pad, adjoint")


# ------------------------------------------------------------------------------------------------------------------------------------
# i.  autograd.ConvCL: the forward and every gradient, on the routes 8 - 16 channels on a 6x6 image never reach

CONV_CASES = {
    "wino_cat_res": dict(c0=32, c1=16, co=48, k=3, h=4, w=8, res=True),              # Winograd data gradient, sliced cat(x0, x1) packs
    "wino_cat_res_tall": dict(c0=16, c1=48, co=32, k=3, h=10, w=2, res=True),
    "direct_cat_res_odd": dict(c0=20, c1=12, co=24, k=3, h=5, w=7, res=True),
    "wino_fork": dict(c0=32, c1=32, co=64, k=3, h=6, w=4, fork=True),               # fused second gradient, against the unforked ATen graph
    "pointwise": dict(c0=64, c1=0, co=40, k=1, h=3, w=7, bias=False),
    "pointwise_cat_res": dict(c0=24, c1=40, co=72, k=1, h=3, w=7, res=True),
    "down": dict(c0=16, c1=0, co=24, k=4, h=6, w=10, stride=2),
    "deconv": dict(c0=24, c1=0, co=16, k=4, h=3, w=5, kind="deconv"),
    "seven_thin_input": dict(c0=4, c1=0, co=32, k=7, h=5, w=9),                      # thin-input im2col route
    "seven_thin_output": dict(c0=32, c1=0, co=4, k=7, h=6, w=9),                     # small-N forward, thin-output route
    "three_relu": dict(c0=16, c1=0, co=8, k=3, h=5, w=4, relu=True),
    "wino_relu": dict(c0=32, c1=0, co=32, k=3, h=4, w=6, relu=True),
    "five": dict(c0=12, c1=0, co=12, k=5, h=4, w=9),
}


@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_conv_function_routes(backend, case):
    dev = backend
    g = CONV_CASES[case]
    n = 3
    c0, c1, co, k, h, w = g["c0"], g["c1"], g["co"], g["k"], g["h"], g["w"]
    kind, stride = g.get("kind", "conv"), g.get("stride", 1)
    x0 = rnd(n, c0, h, w, seed=1).double().requires_grad_(True)
    x1 = rnd(n, c1, h, w, seed=2).double().requires_grad_(True) if c1 else None
    xin = x0 if x1 is None else torch.cat((x0, x1), 1)
    wshape = (c0, co, 1, k, k) if kind == "deconv" else ((co, c0 + c1) if k == 1 else (co, c0 + c1, 1, k, k))
    wt = (rnd(*wshape, seed=3) * 0.1).double().requires_grad_(True)
    b = rnd(co, seed=4).double().requires_grad_(True) if g.get("bias", True) else None
    if kind == "deconv":
        ref = F.conv_transpose2d(xin, wt[:, :, 0], b, stride=2, padding=1)
    elif k == 1:
        ref = F.conv2d(xin, wt[:, :, None, None], b)
    else:
        ref = F.conv2d(xin, wt[:, :, 0], b, stride=stride, padding=1 if k == 4 else k // 2)
    res = rnd(*ref.shape, seed=5).double().requires_grad_(True) if g.get("res") else None
    if res is not None:
        ref = ref + res
    if g.get("relu"):
        ref = F.relu(ref)
    if g.get("fork"):
        wr = (rnd(co, c0 + c1, seed=6) * 0.1).double().requires_grad_(True)        # the block's 1x1 res_conv over the same two inputs
        ref = F.conv2d(xin, wr[:, :, None, None]) + ref
    dy = rnd(*ref.shape, seed=9)
    ref.backward(dy.double())
    leaf = lambda t: None if t is None else t.detach().float().to(dev).requires_grad_(True)
    cl = lambda t: None if t is None else to_cl(t.detach().float()).to(dev).requires_grad_(True)
    kx0, kx1, kres, kw_, kb = cl(x0), cl(x1), cl(res), leaf(wt), leaf(b)
    args = {}
    if kind == "deconv":
        args["kind"] = "deconv"
    if stride == 2:
        args.update(stride=2, pad=(1, 1))
    if k in (5, 7):
        args["pad"] = (k // 2, k // 2)
    if g.get("relu"):
        args["relu"] = True
    if g.get("fork"):
        kwr = leaf(wr)
        hmid, xa, xb = A.conv_cl(kx0, kw_, kb, x1=kx1, n_img=n, hi=h, wi=w, fork=True)
        y = A.conv_cl(xa, kwr, None, x1=xb, residual=hmid, n_img=n, hi=h, wi=w)
    else:
        y = A.conv_cl(kx0, kw_, kb, x1=kx1, residual=kres, n_img=n, hi=h, wi=w, **args)
    ho, wo = ref.shape[2], ref.shape[3]
    _cmp(from_cl(y, n, ho, wo), ref.detach(), case + " y")
    y.backward(to_cl(dy).to(dev))
    _cmp(kw_.grad, wt.grad, case + " dW")
    if b is not None:
        _cmp(kb.grad, b.grad, case + " db")
    _cmp(from_cl(kx0.grad, n, h, w), x0.grad, case + " dx0")
    if x1 is not None:
        _cmp(from_cl(kx1.grad, n, h, w), x1.grad, case + " dx1")
    if res is not None:
        _cmp(from_cl(kres.grad, n, ho, wo), res.grad, case + " dresidual")
    if g.get("fork"):
        _cmp(kwr.grad, wr.grad, case + " dW of the res_conv")
