"""Final-output stores written through (csrc/lfdm_device.h, lfdm_store_f4_out): what a change of a store's cache policy can break.

The float4 epilogues of the Winograd, implicit-GEMM and pointwise convolutions and of the GroupNorm apply kernel store their results
with write-through 16-byte stores; every narrower store and every fallback path keeps its plain store.  The values and addresses are
the ones the plain stores wrote, so every comparison here is bit for bit:

  1. rows wider than the payload: the call into a NaN-filled window (tests/layout.py) equals the call into a contiguous destination,
     and no float of the padding changed;
  2. the fallback side: a destination one float into an aligned buffer, or with a row stride that is no multiple of 4, takes the scalar
     path (or is refused where the entry point always refused it) - parity bar of the entry point, padding untouched;
  3. in place: `out` aliasing the residual (convolutions) or x (GroupNorm apply) equals the unaliased call;
  4. no stale line across a launch boundary: a captured chain conv -> GroupNorm -> conv replayed 200 times on alternating inputs.

The fused temporal-attention block stores its result four bytes per lane and the fused linear-attention block measured slower written
through (profiles/store_through_ab.txt): both keep plain stores, and their cases here pin the layout behaviour either policy must have.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from cvpr23_lfdm_amd import ops
from layout import no_nan, window
from util import assert_close, from_cl, to_cl

TOL = 1e-4            # test_ops_parity.py


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _out(rows, c, dev, spec):
    """A NaN-filled destination: contiguous (spec None) or a window (ld_extra, col_off) with a guard row on either side."""
    if spec is None:
        return torch.full((rows, c), float("nan"), device=dev), lambda what="": None
    return window((rows, c), ld_extra=spec[0], col_off=spec[1], guard_rows=1, device=dev)


# ------------------------------------------------------------------------------------------ Winograd F(2x2)
# one 12 x 12 image: 36 tiles = two workgroups of 32 tiles, the second ragged; 40 output channels: a ragged second column tile
@functools.lru_cache(maxsize=None)
def _wino_problem(cout):
    cin, h, w = 64, 12, 12
    x = rnd(1, cin, h, w, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=1.0 / math.sqrt(9 * cin))
    bias, res = rnd(cout, seed=3), rnd(1, cout, h, w, seed=4)
    conv = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
    return dict(cin=cin, h=h, w=w, x=to_cl(x), wt=wt, bias=bias, res=to_cl(res), ref=conv.float(), ref_res=(conv + res.double()).float())


def _wino_run(dev, cout, ksplit, spec, *, residual=False, alias=False):
    """-> (result rows on the CPU, schedule, (tile_rows, ksplit)); asserts the window's padding itself."""
    pr = _wino_problem(cout)
    h, w = pr["h"], pr["w"]
    xs, wtd = pr["x"].to(dev), pr["wt"].to(dev)
    wd, ww = ops.pack_conv_weight(pr["wt"]).to(dev), ops.pack_wino_weight(wtd)
    res, chk_r = None, None
    if residual:
        res, chk_r = (pr["res"].to(dev).clone(), None) if spec is None else window(pr["res"].to(dev), ld_extra=spec[0], col_off=spec[1], guard_rows=1)
    out, chk = (res, chk_r) if alias else _out(h * w, cout, dev, spec)
    counters = torch.zeros(64, dtype=torch.int32, device=dev) if ksplit > 1 else None          # in-launch reduction: the reducer's final store
    kw = dict(bias=pr["bias"].to(dev), weight_wino=ww, ksplit=ksplit, tile_counters=counters, residual=res, out=out)
    pp, _ = ops.conv_params(xs, wd, cout, 3, 3, 1, h, w, **kw)
    sched, plan = ops.conv_schedule(pp), ops.conv_plan(pp)
    got = ops.conv2d_cl(xs, wd, cout, 3, 3, 1, h, w, **kw)
    if dev == "cuda":
        torch.cuda.synchronize()
    for c_ in (chk, chk_r):
        if c_ is not None:
            c_("winograd cout %d ksplit %d window %s" % (cout, ksplit, spec))
    if counters is not None:
        assert int(counters.abs().sum()) == 0, "tile counters not left at zero"
    return got.cpu().contiguous(), sched, plan


@pytest.mark.parametrize("ksplit", [1, 2])
@pytest.mark.parametrize("cout", [32, 40])
def test_winograd_rows_wider_than_payload(backend, cout, ksplit, monkeypatch):
    monkeypatch.setenv("LFDM_WINO", "1")
    pr = _wino_problem(cout)
    got0, sched, plan = _wino_run(backend, cout, ksplit, None)
    assert sched == 2 and plan[1] == ksplit, (sched, plan)
    if ksplit > 1:          # whole 32-column tiles: reduced in the launch (the reducer's final store); 40 columns: the reduce pass stores them
        assert plan[0] == (128 if cout % 32 == 0 else 16), "unexpected split-K plan %s" % (plan,)
    no_nan(got0, "winograd, contiguous")
    assert_close(from_cl(got0, 1, pr["h"], pr["w"]), pr["ref"], TOL, "winograd cout %d ksplit %d" % (cout, ksplit))
    got, sched1, plan1 = _wino_run(backend, cout, ksplit, (12, 4))
    assert (sched1, plan1) == (sched, plan)
    assert torch.equal(got, got0), "winograd cout %d ksplit %d: the wide destination differs from the contiguous one" % (cout, ksplit)


@pytest.mark.parametrize("spec", [(4, 1), (1, 0)], ids=["out_plus1", "ldo_mod4"])
def test_winograd_fallback_side(backend, spec, monkeypatch):
    """No 16-byte stores are legal: the planner leaves the Winograd schedule, the scalar epilogue stores plain."""
    monkeypatch.setenv("LFDM_WINO", "1")
    pr = _wino_problem(32)
    got, sched, _ = _wino_run(backend, 32, 1, spec)
    assert sched == 0, "schedule %d kept for a destination that is not 16-byte addressable" % sched
    no_nan(got, "winograd fallback")
    assert_close(from_cl(got, 1, pr["h"], pr["w"]), pr["ref"], TOL, "fallback %s" % (spec,))


@pytest.mark.parametrize("ksplit", [1, 2])
def test_winograd_out_aliases_residual(backend, ksplit, monkeypatch):
    monkeypatch.setenv("LFDM_WINO", "1")
    pr = _wino_problem(40)
    got0, sched, plan = _wino_run(backend, 40, ksplit, None, residual=True)
    assert sched == 2 and plan[1] == ksplit
    assert_close(from_cl(got0, 1, pr["h"], pr["w"]), pr["ref_res"], TOL, "winograd + residual")
    for spec in (None, (12, 4)):
        got, sched1, plan1 = _wino_run(backend, 40, ksplit, spec, residual=True, alias=True)
        assert (sched1, plan1) == (sched, plan)
        assert torch.equal(got, got0), "out = residual (%s) differs from the unaliased call" % (spec,)


# ------------------------------------------------------------------------------------------ GroupNorm apply
# 132 pixels x 64 channels in 8 groups; the entry point takes dense rows only, so the "padding" is the guard rows around them
@functools.lru_cache(maxsize=None)
def _gn_problem():
    pixels, c, groups, nchunk = 132, 64, 8, 3
    x = rnd(pixels, c, seed=1) * 2 + 0.5
    gamma, beta, res = rnd(c, seed=2) + 1.0, rnd(c, seed=3), rnd(pixels, c, seed=5)
    xg = x.double().view(nchunk, pixels // nchunk, groups, c // groups)
    partial = torch.stack([xg.sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))], dim=-1).float().contiguous().view(nchunk, 2 * groups)
    y = F.silu(F.group_norm(x.double().t().reshape(1, c, pixels), groups, gamma.double(), beta.double(), eps=1e-5))[0].t()
    return dict(x=x, gamma=gamma, beta=beta, res=res, partial=partial, nchunk=nchunk, ref=y.float(), ref_res=(y + res.double()).float())


def _gn_call(dev, x, out, residual):
    pr = _gn_problem()
    return ops.groupnorm_apply_cl(x, 1, pr["gamma"].to(dev), pr["beta"].to(dev), pr["partial"].to(dev), pr["nchunk"], groups=8,
                                  residual=pr["res"].to(dev) if residual else None, out=out)


@pytest.mark.parametrize("residual", [False, True])
def test_groupnorm_apply_guarded_destination_and_in_place(backend, residual):
    dev = backend
    pr = _gn_problem()
    got0 = _gn_call(dev, pr["x"].to(dev), None, residual).cpu()
    assert_close(got0, pr["ref_res"] if residual else pr["ref"], TOL, "groupnorm apply")
    out, chk = window((132, 64), ld_extra=0, col_off=0, guard_rows=1, device=dev)
    got = _gn_call(dev, pr["x"].to(dev), out, residual).cpu()
    chk("groupnorm apply, guarded destination")
    assert torch.equal(got, got0)
    x, chk = window(pr["x"].to(dev), ld_extra=0, col_off=0, guard_rows=1)          # in place: out = x
    got = _gn_call(dev, x, x, residual).cpu()
    chk("groupnorm apply in place")
    assert torch.equal(got, got0), "out = x differs from the unaliased call"


def test_groupnorm_apply_still_refuses_a_destination_one_float_in(backend):
    dev = backend
    pr = _gn_problem()
    v, chk = window((1, 132 * 64), ld_extra=8, col_off=1, guard_rows=1, device=dev)
    out = v[0].view(132, 64)
    with pytest.raises(RuntimeError, match="lfdm_groupnorm_apply_cl_f32 failed"):
        _gn_call(dev, pr["x"].to(dev), out, False)
    chk("refused groupnorm apply")
    assert bool(torch.isnan(out).all()), "a refused call wrote into its output"


# ------------------------------------------------------------------------------------------ pointwise schedule
# 132 rows (four 32-row tiles and a ragged fifth), K = 64 into 32 and 48 columns (a ragged second column tile).  The res_gn form is refused
# unless the pixels of a sample are a multiple of 32 (lfdm_hip.h): it runs at the next legal size, 160 rows.
@functools.lru_cache(maxsize=None)
def _pw_problem(cout, form):
    cin, groups = 64, 4
    h, w, nchunk = (12, 11, 3) if form == "plain" else (10, 16, 2)
    x = rnd(1, cin, h, w, seed=1)
    wt = rnd(cout, cin, 1, 1, seed=2, scale=1.0 / math.sqrt(cin))
    bias, gamma, beta = rnd(cout, seed=3), rnd(cout, seed=4) * 0.3 + 1, rnd(cout, seed=5) * 0.3
    raw = rnd(h * w, cout, seed=6) * 1.5 + 0.2
    conv = to_cl(F.conv2d(x.double(), wt.double(), bias.double()))
    rs = raw.double()
    act = F.silu(F.group_norm(rs.t().reshape(1, cout, h * w), groups, gamma.double(), beta.double(), eps=1e-5))[0].t()
    rg = rs.view(nchunk, h * w // nchunk, groups, cout // groups)
    partial = torch.stack([rg.sum(dim=(1, 3)), (rg * rg).sum(dim=(1, 3))], dim=-1).float().contiguous().view(nchunk, 2 * groups)
    return dict(cin=cin, h=h, w=w, x=to_cl(x), wt=wt, bias=bias, raw=raw, ref=conv.float(), ref_res_gn=(conv + act).float(),
                res_gn=dict(partial=partial, nchunk=nchunk, pixels=h * w, gamma=gamma, beta=beta, groups=groups))


def _pw_run(dev, cout, form, spec):
    pr = _pw_problem(cout, form)
    h, w = pr["h"], pr["w"]
    xs, wd = pr["x"].to(dev), ops.pack_conv_weight(pr["wt"]).to(dev)
    kw = dict(bias=pr["bias"].to(dev))
    if form == "res_gn":          # h + res_conv(x) with the GroupNorm + SiLU of h in the epilogue: out IS the residual, as the sampler runs it
        out, chk = (pr["raw"].to(dev).clone(), lambda what="": None) if spec is None else window(pr["raw"].to(dev), ld_extra=spec[0], col_off=spec[1], guard_rows=1)
        kw.update(residual=out, res_gn={k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in pr["res_gn"].items()})
    else:
        out, chk = _out(h * w, cout, dev, spec)
    kw["out"] = out
    pp, _ = ops.conv_params(xs, wd, cout, 1, 1, 1, h, w, **kw)
    sched = ops.conv_schedule(pp)
    return sched, chk, out, (lambda: ops.conv2d_cl(xs, wd, cout, 1, 1, 1, h, w, **kw))


@pytest.mark.parametrize("form", ["plain", "res_gn"])
@pytest.mark.parametrize("cout", [32, 48])
def test_pointwise_rows_wider_than_payload(backend, cout, form, monkeypatch):
    monkeypatch.setenv("LFDM_PW", "2")
    pr = _pw_problem(cout, form)
    sched, _, _, go = _pw_run(backend, cout, form, None)
    assert sched == 3, "the pointwise schedule was not selected"
    got0 = go().cpu().contiguous()
    no_nan(got0, "pointwise %s" % form)
    assert_close(got0, pr["ref_res_gn"] if form == "res_gn" else pr["ref"], TOL, "pointwise %s into %d columns" % (form, cout))
    sched, chk, _, go = _pw_run(backend, cout, form, (12, 4))
    assert sched == 3
    got = go().cpu().contiguous()
    chk("pointwise %s, wide destination" % form)
    assert torch.equal(got, got0), "pointwise %s into %d columns: the wide destination differs from the contiguous one" % (form, cout)


@pytest.mark.parametrize("spec", [(4, 1), (1, 0)], ids=["out_plus1", "ldo_mod4"])
def test_pointwise_fallback_side(backend, spec, monkeypatch):
    """Plain: the planner leaves the pointwise schedule and the scalar epilogue stores plain.  res_gn exists on the pointwise schedule only:
    still refused, nothing written."""
    monkeypatch.setenv("LFDM_PW", "2")
    pr = _pw_problem(32, "plain")
    sched, chk, _, go = _pw_run(backend, 32, "plain", spec)
    assert sched != 3
    got = go().cpu().contiguous()
    chk("pointwise fallback")
    assert_close(got, pr["ref"], TOL, "pointwise fallback %s" % (spec,))
    sched, chk, out, go = _pw_run(backend, 32, "res_gn", spec)
    assert sched != 3
    with pytest.raises(RuntimeError, match="lfdm_conv2d_cl_f32 failed.*res_gn"):
        go()
    chk("pointwise res_gn refused")
    assert torch.equal(out.cpu(), _pw_problem(32, "res_gn")["raw"]), "the refused call changed its in/out operand"


# ------------------------------------------------------------------------------------------ fused attention blocks: 2 x 2 pixels, T = 5
def test_temporal_attention_fused_out_rows_wider_than_payload(backend):
    import lfdm_oracle as O
    dev = backend
    c, frames, s = 64, 5, 2
    hw, rows = s * s, frames * s * s
    x = (rnd(rows, c, seed=1) * 2 + 0.5).to(dev)
    wf, wo = rnd(768, c, seed=3, scale=1.0 / math.sqrt(c)), rnd(c, 256, seed=9, scale=1.0 / 16)
    cos, sin = O.rotary_tables(1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)), frames)
    tab = dict(bias=O.rel_pos_bias(rnd(32, 8, seed=4), frames).contiguous().to(dev), rot_cos=cos[:, 0::2].contiguous().to(dev),
               rot_sin=sin[:, 0::2].contiguous().to(dev))
    wqp, wop = (t.to(dev) for t in ops.pack_tattn_weights(wf, wo))
    got0 = ops.temporal_attention_fused_out_cl(x, wqp, wop, 1, frames, hw, **tab).cpu()
    no_nan(got0, "temporal attention block")
    for spec in ((12, 4), (4, 1), (1, 0)):          # (scalar stores: any destination is legal and gives the same bits)
        out, chk = _out(rows, c, dev, spec)
        got = ops.temporal_attention_fused_out_cl(x, wqp, wop, 1, frames, hw, out=out, **tab).cpu().contiguous()
        chk("temporal attention block %s" % (spec,))
        assert torch.equal(got, got0), "temporal attention block: destination %s differs from the contiguous one" % (spec,)


def test_linear_attention_fused_out_rows_wider_than_payload(backend):
    dev = backend
    nf, c, hw = 5, 64, 4
    x = (rnd(nf * hw, c, seed=1) * 2 + 0.3).to(dev)
    wf, wo, bo = rnd(768, c, seed=3, scale=1.0 / math.sqrt(c)), rnd(c, 256, seed=4, scale=1.0 / 16), rnd(c, seed=5).to(dev)
    wp, wop = ops.pack_linattn_weights(wf).to(dev), ops.pack_linattn_out_weight(wo).to(dev)
    got0 = ops.linear_attention_fused_out_cl(x, wp, wop, bo, nf, hw).cpu()
    no_nan(got0, "linear attention block")
    out, chk = _out(nf * hw, c, dev, (12, 4))
    got = ops.linear_attention_fused_out_cl(x, wp, wop, bo, nf, hw, out=out).cpu().contiguous()
    chk("linear attention block, wide destination")
    assert torch.equal(got, got0), "linear attention block: the wide destination differs from the contiguous one"
    for spec in ((4, 1), (1, 0)):                   # float4 stores: refused as before, nothing written
        out, chk = _out(nf * hw, c, dev, spec)
        with pytest.raises(RuntimeError, match="lfdm_linear_attention_fused_out_cl_f32 failed"):
            ops.linear_attention_fused_out_cl(x, wp, wop, bo, nf, hw, out=out)
        chk("linear attention block refused")
        assert bool(torch.isnan(out).all()), "a refused call wrote into its output"


# ------------------------------------------------------------------------------------------ no stale line across a launch boundary
@pytest.mark.gpu
def test_replayed_chain_rewrites_the_same_lines():
    """Winograd conv -> GroupNorm (statistics pass + apply) -> Winograd conv captured as one graph on 1 152 + 16 pixels x 64 channels (ten
    Winograd workgroups, several XCDs write and read every tensor), replayed 200 times while the input alternates between two tensors
    through an in-graph copy: the same arena lines are rewritten with other values on every replay, and every replay must equal the
    eager result for its input bit for bit.  A consumer that saw an old line of its producer would differ."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvpr23_lfdm_amd import _native
    _native._set_library_for_tests(None)
    dev = "cuda"
    c, h, w = 64, 8, 146          # 1168 pixels = 292 tiles
    wts = [rnd(c, c, 3, 3, seed=10 + i, scale=1.0 / math.sqrt(9 * c)) for i in range(2)]
    wd = [ops.pack_conv_weight(t).to(dev) for t in wts]
    ww = [ops.pack_wino_weight(t.to(dev)) for t in wts]
    bias = [rnd(c, seed=20 + i).to(dev) for i in range(2)]
    gamma, beta = (rnd(c, seed=30) + 1.0).to(dev), rnd(c, seed=31).to(dev)
    inputs = [rnd(h * w, c, seed=40 + i).to(dev) for i in range(2)]
    stage, x = torch.empty_like(inputs[0]), torch.empty_like(inputs[0])
    a, g, y = (torch.empty(h * w, c, device=dev) for _ in range(3))
    ws = torch.empty(ops._lib().lfdm_groupnorm_ws_bytes(1, h * w, c) // 4 + 4, device=dev)

    def chain():
        x.copy_(stage)
        pp, _ = ops.conv_params(x, wd[0], c, 3, 3, 1, h, w, bias=bias[0], weight_wino=ww[0], ksplit=1, out=a)
        assert ops.conv_schedule(pp) == 2
        ops.conv2d_cl(x, wd[0], c, 3, 3, 1, h, w, bias=bias[0], weight_wino=ww[0], ksplit=1, out=a)
        ops.groupnorm_silu_cl(a, 1, gamma, beta, out=g, ws=ws)
        ops.conv2d_cl(g, wd[1], c, 3, 3, 1, h, w, bias=bias[1], weight_wino=ww[1], ksplit=1, out=y)

    want = []
    for t in inputs:              # eager results (and the warm-up in front of the capture)
        stage.copy_(t)
        chain()
        want.append(y.clone())
    assert not torch.equal(want[0], want[1]) and bool(torch.isfinite(want[0]).all())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    for i in range(200):
        stage.copy_(inputs[i & 1])
        graph.replay()
        bad += (y.view(torch.int32) != want[i & 1].view(torch.int32)).sum()
    assert int(bad) == 0, "%d words of the replayed chain differ from the eager results" % int(bad)
