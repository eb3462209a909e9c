"""Operand layouts: every strided, offset and aliased layout the C ABI (include/lfdm_hip.h) accepts, per entry point.

The parity tests (test_ops_parity.py, test_train_ops.py) walk every SHAPE dispatch edge with contiguous, 256-byte aligned operands.
These tests walk the LAYOUT dispatch: the same small shapes on both backends, each operand inside a NaN-filled buffer (tests/layout.py):

  L0  contiguous - what the suite already covers; here only the comparison partner.
  L1  wide:   every row operand has its own row stride (ld_extra 4 / 12) and column offset (0 / 4); all 16-byte aligned, ld % 4 == 0.
  L2  alias:  `out` is the residual's (or x's) own view wherever the header allows it or the package does it.
  L3  ragged: the fallback side of each alignment gate - ld % 4 != 0, or a pointer one float into an aligned buffer.

Each comparison asserts (a) the entry point's own parity bar against its own reference (TOL forward, 2e-4 backward - no new tolerance),
(b) bit identity with the L0 run whenever the library reports the same plan (only addresses differ then), (c) `check()` on every
windowed operand - nothing outside a window was written - and (d) no NaN in the result - nothing outside a window was read into it.
Refusals: the call raises, the message names the entry point, nothing was written.
"""
import ast
import ctypes
import functools
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from cvpr23_lfdm_amd import ops
from layout import LayoutCase, aligned16, no_nan, window, window_batched
from util import assert_close, from_cl, to_cl, unet_from_cl, unet_to_cl

TOL = 1e-4            # test_ops_parity.py
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# which test covers which entry point under which layout (the coverage test below reads it)
CASE_TABLE = []


def covers(entry, layout, operands, expect):
    def deco(fn):
        CASE_TABLE.append(LayoutCase(entry, layout, dict(operands), expect, fn.__name__))
        return fn
    return deco


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------ convolution
# The smallest shape of the existing tests that reaches each schedule (test_conv2d, test_conv_pointwise, test_conv2d_winograd,
# test_conv_winograd_splitk_reduced_in_launch, test_conv2d_winograd4).  sched = what the library must plan for the aligned layouts.
CONV_CASES = {
    "s0_fast_simple": dict(cin=32, cout=64, k=3, n=2, h=8, w=8, sched=0),
    "s0_fast_upsample_reflect": dict(cin=32, cout=32, k=3, n=2, h=4, w=4, upsample=True, reflect=True, sched=0),
    "s0_generic": dict(cin=3, cout=64, k=7, n=1, h=12, w=12, sched=0),
    "s0_cout3": dict(cin=64, cout=3, k=7, n=1, h=10, w=10, act=2, sched=0),
    "s0_two_sources": dict(cin=64, cout=64, k=3, n=2, h=8, w=8, split_src=32, residual=True, sched=0),
    "s0_splitk3": dict(cin=64, cout=64, k=3, n=2, h=8, w=8, ksplit=3, residual=True, act=1, sched=0),
    "s1_ksw": dict(cin=64, cout=64, k=3, n=5, h=8, w=8, residual=True, act=1, sched=1),
    "s1_ksw_strided": dict(cin=32, cout=32, k=4, n=5, h=16, w=16, stride=2, pad=1, env={"LFDM_PW": "0"}, sched=1),
    "s1_ksw_splitk": dict(cin=96, cout=128, k=3, n=3, h=8, w=10, split_src=32, ksplit=2, sched=1),
    "s2_wino": dict(cin=32, cout=64, k=3, n=2, h=8, w=8, wino=True, sched=2),
    "s2_wino_upsample": dict(cin=32, cout=64, k=3, n=2, h=4, w=6, upsample=True, act=1, wino=True, sched=2),
    "s2_wino_splitk_reduce_pass": dict(cin=128, cout=32, k=3, n=1, h=4, w=4, ksplit=2, act=1, wino=True, sched=2),
    "s2_wino_reduced_in_launch": dict(cin=64, cout=64, k=3, n=16, h=4, w=4, ksplit=2, wino=True, counters=True, gn=(2, 8), sched=2),
    "s2_wino_gn": dict(cin=64, cout=64, k=3, n=8, h=8, w=8, wino=True, gn=(2, 8), sched=2),
    "s3_pointwise": dict(cin=64, cout=128, k=1, n=3, h=5, w=7, env={"LFDM_PW": "2"}, sched=3),
    "s3_pointwise_two_sources": dict(cin=96, cout=64, k=1, n=2, h=3, w=3, split_src=32, act=3, env={"LFDM_PW": "2"}, sched=3),
    "s4_wino4_direct": dict(cin=32, cout=32, k=3, n=2, h=8, w=8, wino=True, wino4=True, env={"LFDM_WINO4": "1", "LFDM_WINO4_MIN": "1"}, sched=4),
    "s4_wino4_staged": dict(cin=64, cout=40, k=3, n=3, h=16, w=32, residual=True, act=1, wino=True, wino4=True,
                            env={"LFDM_WINO4": "1", "LFDM_WINO4_MIN": "1"}, sched=4),
}

# (ld_extra, col_off) per operand.  L1: every row operand its own stride and offset, 16-byte aligned, ld % 4 == 0.
L1 = dict(src0=(4, 0), src1=(12, 4), out=(12, 4), res=(4, 4))
# L3: ONE operand on the fallback side of its gate, the others as in L1
L3_OUT = {            # -> planner's vec_ok false: no ksw / Winograd / pointwise schedule, no in-launch reduction; scalar epilogue and reduce pass
    "ldo_mod4": dict(out=(1, 0)),
    "out_plus1": dict(out=(4, 1)),
    "ldr_mod4": dict(res=(1, 0)),
    "res_plus1": dict(res=(4, 1)),
    "bias_plus1": dict(bias=(4, 1)),
}
L3_SRC = {            # -> pl.fast false: generic load path of schedule 0
    "ld0_mod4": dict(src0=(1, 0)),
    "src0_plus1": dict(src0=(4, 1)),
}


@functools.lru_cache(maxsize=None)
def _conv_problem(name, residual):
    """Inputs and the float64 reference of one convolution case, computed once and shared (never modified)."""
    case = CONV_CASES[name]
    cin, cout, k, n, h, w = (case[x] for x in ("cin", "cout", "k", "n", "h", "w"))
    stride, pad = case.get("stride", 1), case.get("pad", k // 2)
    x = rnd(n, cin, h, w, seed=1)
    wt = rnd(cout, cin, k, k, seed=2, scale=1.0 / math.sqrt(cin * k * k))
    bias = rnd(cout, seed=3)
    xin = x.double()
    if case.get("upsample"):
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    if case.get("reflect"):
        conv = F.conv2d(F.pad(xin, (pad,) * 4, mode="reflect"), wt.double(), bias.double(), stride=stride)
    else:
        conv = F.conv2d(xin, wt.double(), bias.double(), stride=stride, padding=pad)
    ref, res = conv, None
    if residual:
        res = rnd(*conv.shape, seed=4)
        ref = ref + res.double()
    act = case.get("act", 0)
    ref = {0: lambda v: v, 1: F.relu, 2: torch.sigmoid, 3: F.silu}[act](ref)
    return dict(x=to_cl(x), wt=wt, bias=bias, res=None if res is None else to_cl(res), ref=ref.float(), conv=conv.float(),
                ho=conv.shape[2], wo=conv.shape[3])


def _place(t, spec, dev):
    """An operand under a layout: spec None = contiguous (L0), else (ld_extra, col_off)."""
    if spec is None:
        return t.to(dev).clone().contiguous(), None
    v, chk = window(t.to(dev), ld_extra=spec[0], col_off=spec[1], guard_rows=1)
    return v, chk


def _conv_run(dev, name, lay, *, residual, alias=False, refused=None, monkeypatch):
    """One launch of case `name` under layout `lay` (operand -> (ld_extra, col_off); {} = L0).  Returns the result rows (a contiguous
    copy), the plan the library reported and the GroupNorm partial sums; asserts (c) and (d) itself.
    refused = a word of the expected error: the launch must raise, name its entry point, and write nothing."""
    case = CONV_CASES[name]
    for k_, v_ in case.get("env", {}).items():
        monkeypatch.setenv(k_, v_)
    if case.get("wino"):
        monkeypatch.setenv("LFDM_WINO", "1")
    pr = _conv_problem(name, residual)
    cin, cout, k, n, h, w = (case[x] for x in ("cin", "cout", "k", "n", "h", "w"))
    checks = []

    def put(t, key):
        v, chk = _place(t, lay.get(key), dev)
        if chk is not None:
            checks.append((key, chk))
        return v

    xs = pr["x"]
    s = case.get("split_src")
    src0 = put(xs if not s else xs[:, :s], "src0")
    src1 = put(xs[:, s:], "src1") if s else None
    res = put(pr["res"], "res") if residual else None
    if "bias" in lay:
        bv, chk = window(pr["bias"].view(1, cout).to(dev), ld_extra=lay["bias"][0], col_off=lay["bias"][1], guard_rows=1)
        checks.append(("bias", chk))
        bias = bv[0]
    else:
        bias = pr["bias"].to(dev)
    rows_out = n * pr["ho"] * pr["wo"]
    if alias:
        out = res
    elif "out" in lay:
        out, chk = window((rows_out, cout), ld_extra=lay["out"][0], col_off=lay["out"][1], guard_rows=1, device=dev)
        checks.append(("out", chk))
    else:
        out = torch.full((rows_out, cout), float("nan"), device=dev)
    wtd = pr["wt"].to(dev)
    kw = dict(src1=src1, bias=bias, pad=(case.get("pad", k // 2),) * 2, stride=case.get("stride", 1), upsample=bool(case.get("upsample")),
              reflect=bool(case.get("reflect")), residual=res, act=case.get("act", 0), ksplit=case.get("ksplit", 1), out=out)
    if case.get("wino"):
        kw["weight_wino"] = ops.pack_wino_weight(wtd)
    if case.get("wino4"):
        kw["weight_wino4"] = ops.pack_wino4_weight(wtd)
    counters = None
    if case.get("counters"):
        counters = kw["tile_counters"] = torch.zeros(64, dtype=torch.int32, device=dev)
    wd = ops.pack_conv_weight(pr["wt"]).to(dev)
    pp, _ = ops.conv_params(src0, wd, cout, k, k, n, h, w, **kw)
    gn = case.get("gn")
    if gn:
        pp.gn_partial = 1
    tile_rows, ks = ops.conv_plan(pp)
    plan = dict(schedule=ops.conv_schedule(pp), tile_rows=tile_rows, ksplit=ks, slabs=ops.conv_plan_slabs(pp))
    need = ops.conv_partial_floats(pp)
    extra = {}
    if need > 0:          # the split-K slabs are an in/out workspace: windowed too (the library rounds its base up inside the buffer)
        pv, chk = window((1, need), ld_extra=8, col_off=4, guard_rows=1, device=dev)
        checks.append(("partial", chk))
        extra["partial"] = pv[0]
    partial_gn = None
    if gn:
        batch, groups = gn
        pixels = rows_out // batch
        if pixels % tile_rows == 0:
            partial_gn = torch.zeros(batch * (pixels // tile_rows), 2 * groups, device=dev)
            extra.update(gn_partial=partial_gn, gn_groups=groups, gn_pixels=pixels)
    if refused is not None:
        with pytest.raises(RuntimeError, match=r"lfdm_conv2d_cl_f32 failed.*%s" % refused):
            ops.conv2d_cl(src0, wd, cout, k, k, n, h, w, **kw, **extra)
        for key, chk in checks:
            chk("%s [%s] refused, operand %s" % (name, lay, key))
        assert bool(torch.isnan(out).all()), "a refused call wrote into its output"
        return None, plan, None
    for rep in range(2 if counters is not None else 1):          # second launch: the counters were left at zero
        if alias and rep:
            res.copy_(pr["res"])
        got = ops.conv2d_cl(src0, wd, cout, k, k, n, h, w, **kw, **extra)
    if dev == "cuda":
        torch.cuda.synchronize()
    if counters is not None:
        assert int(counters.abs().sum()) == 0, "tile counters not left at zero"
    for key, chk in checks:
        chk("%s [%s], operand %s" % (name, lay, key))
    got = got.cpu().contiguous()
    no_nan(got, "%s %s" % (name, lay))
    assert_close(from_cl(got, n, pr["ho"], pr["wo"]), pr["ref"], TOL, "%s %s" % (name, lay))
    if gn:          # the statistics describe conv + bias (before the residual), as test_conv2d_winograd checks them
        assert partial_gn is not None, "%s %s: plan %s cannot carry the case's GroupNorm statistics" % (name, lay, plan)
        y = pr["conv"].view(batch, n // batch, groups, cout // groups, pr["ho"], pr["wo"]).permute(0, 2, 1, 3, 4, 5).reshape(batch, groups, -1).double()
        tot = partial_gn.cpu().view(batch, -1, groups, 2).double().sum(dim=1)
        assert_close(tot[..., 0].float(), y.sum(-1).float(), TOL, "%s %s: gn sum" % (name, lay))
        assert_close(tot[..., 1].float(), (y * y).sum(-1).float(), TOL, "%s %s: gn sumsq" % (name, lay))
    return got, plan, None if partial_gn is None else partial_gn.cpu()


def _same_or_name_the_field(name, got, plan, got0, plan0, what):
    """(b): only addresses differ when the plans are equal - then the results are bit-identical."""
    differs = [f for f in plan if plan[f] != plan0[f]]
    assert not differs, "%s %s: the library planned differently from the contiguous layout: %s" % (
        name, what, ", ".join("%s %s -> %s" % (f, plan0[f], plan[f]) for f in differs))
    assert torch.equal(got, got0), "%s %s: same plan %s as the contiguous layout, but the result differs (max abs %.3e)" % (
        name, what, plan, float((got - got0).abs().max()))


@covers("lfdm_conv2d_cl_f32", "L1", L1, "the schedule of the contiguous layout, bit-identical")
@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_wide(backend, name, monkeypatch):
    """L1: src0 / src1 / out / residual each in a window of its own row stride and column offset."""
    case = CONV_CASES[name]
    residual = bool(case.get("residual"))
    got0, plan0, gn0 = _conv_run(backend, name, {}, residual=residual, monkeypatch=monkeypatch)
    assert plan0["schedule"] == case["sched"], (name, plan0)
    got, plan, gn = _conv_run(backend, name, L1, residual=residual, monkeypatch=monkeypatch)
    _same_or_name_the_field(name, got, plan, got0, plan0, "L1")
    if case.get("gn"):
        assert gn0 is not None and torch.equal(gn, gn0), "GroupNorm partial sums differ between the layouts"


@covers("lfdm_conv2d_cl_f32", "L2", dict(L1, out="residual's view"), "the schedule of the contiguous layout, bit-identical")
@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_out_aliases_residual(backend, name, monkeypatch):
    """L2: out IS the residual's window (cvpr23_lfdm_amd/unet.py runs the residual convolution in place on whichever schedule the planner
    picks): every schedule, both reduce passes and the in-launch reduction read each residual element before they overwrite it."""
    case = CONV_CASES[name]
    got0, plan0, _ = _conv_run(backend, name, {}, residual=True, monkeypatch=monkeypatch)
    assert plan0["schedule"] == case["sched"], (name, plan0)
    got, plan, _ = _conv_run(backend, name, L1, residual=True, alias=True, monkeypatch=monkeypatch)
    _same_or_name_the_field(name, got, plan, got0, plan0, "L2")
    got, plan, _ = _conv_run(backend, name, {}, residual=True, alias=True, monkeypatch=monkeypatch)        # ... and contiguous, as the UNet does it
    _same_or_name_the_field(name, got, plan, got0, plan0, "L2 contiguous")


@covers("lfdm_conv2d_cl_f32", "L3", L3_OUT, "schedule 0 (no ksw / Winograd / pointwise, no in-launch reduction), scalar epilogue / reduce pass")
@pytest.mark.parametrize("variant", sorted(L3_OUT))
@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_ragged_output_side(backend, name, variant, monkeypatch):
    """L3, output side: ldo / ldr not a multiple of 4, or out / residual / bias one float into an aligned buffer.  The planner must retreat
    to schedule 0 with the reduce pass (tile_rows 16 when K is split) and the scalar epilogue."""
    case = CONV_CASES[name]
    residual = bool(case.get("residual")) or variant in ("ldr_mod4", "res_plus1")
    lay = dict(L1, **L3_OUT[variant])
    # fused GroupNorm statistics exist in the float4 epilogues only (lfdm_hip.h): with an output that is not 16-byte addressable the request is refused
    refused = "fused GroupNorm statistics" if (case.get("gn") and variant in ("ldo_mod4", "out_plus1")) else None
    got, plan, _ = _conv_run(backend, name, lay, residual=residual, refused=refused, monkeypatch=monkeypatch)
    if case["cout"] % 4 == 0:
        assert plan["schedule"] == 0, "%s %s: the planner kept schedule %d for an output side that is not 16-byte addressable" % (
            name, variant, plan["schedule"])
        if plan["ksplit"] > 1:
            assert plan["tile_rows"] == 16, "%s %s: in-launch reduction kept" % (name, variant)


@covers("lfdm_conv2d_cl_f32", "L3", L3_SRC, "schedule 0, generic load path")
@pytest.mark.parametrize("variant", sorted(L3_SRC))
@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_ragged_source_side(backend, name, variant, monkeypatch):
    """L3, source side: ld0 not a multiple of 4, or src0 one float into an aligned buffer: pl.fast is false, the generic load path runs."""
    case = CONV_CASES[name]
    lay = dict(L1, **L3_SRC[variant])
    got, plan, _ = _conv_run(backend, name, lay, residual=bool(case.get("residual")), monkeypatch=monkeypatch)
    assert plan["schedule"] == 0, "%s %s: the planner kept schedule %d for a source that is not 16-byte addressable" % (name, variant, plan["schedule"])


def test_conv_cases_cover_both_sides_of_every_gate():
    """The table above has, for each alignment gate of make_plan, a case that starts on the fast side (so that the L3 run is a retreat)."""
    scheds = {c["sched"] for c in CONV_CASES.values()}
    assert scheds == {0, 1, 2, 3, 4}
    assert any(c["cout"] % 4 for c in CONV_CASES.values()) and any(c.get("counters") for c in CONV_CASES.values())
    assert any(c.get("ksplit", 1) > 1 and c["sched"] == s for c in CONV_CASES.values() for s in (0,)) and \
        any(c.get("ksplit", 1) > 1 and c["sched"] == 1 for c in CONV_CASES.values()) and \
        any(c.get("ksplit", 1) > 1 and c["sched"] == 2 for c in CONV_CASES.values())


# ------------------------------------------------------------------------------------------ refusals: raise, name the entry point, write nothing
def _refused(entry_word, fn, checks, outs=()):
    with pytest.raises(RuntimeError, match=entry_word):
        fn()
    for what, chk in checks:
        chk("refused %s, operand %s" % (entry_word, what))
    for o in outs:
        assert bool(torch.isnan(o).all()), "a refused %s call wrote into its output" % entry_word


def _nan_out(rows, c, dev, spec=None):
    """An output the kernel must fill: NaN everywhere, in a window when spec = (ld_extra, col_off)."""
    if spec is None:
        return torch.full((rows, c), float("nan"), device=dev), lambda what="": None
    return window((rows, c), ld_extra=spec[0], col_off=spec[1], guard_rows=1, device=dev)


# ------------------------------------------------------------------------------------------ GroupNorm
@functools.lru_cache(maxsize=None)
def _gn_problem(c):
    b, t, s = 2, 3, 4
    x = rnd(b, c, t, s, s, seed=1) * 2 + 0.5
    gamma, beta = rnd(c, seed=2) + 1.0, rnd(c, seed=3)
    ss = rnd(b, 2 * c, seed=4) * 0.5
    res = rnd(b, c, t, s, s, seed=5)
    ref = F.group_norm(x.double(), 8, gamma.double(), beta.double(), eps=1e-5)
    ref = F.silu(ref * (ss[:, :c].double().view(b, c, 1, 1, 1) + 1) + ss[:, c:].double().view(b, c, 1, 1, 1)) + res.double()
    xr = unet_to_cl(x)
    xg = xr.view(b, 3, (t * s * s) // 3, 8, c // 8).double()
    partial = torch.stack([xg.sum(dim=(2, 4)), (xg * xg).sum(dim=(2, 4))], dim=-1).float().contiguous().view(b * 3, 16)
    return dict(b=b, t=t, s=s, x=xr, gamma=gamma, beta=beta, ss=ss, res=unet_to_cl(res), ref=unet_to_cl(ref.float()), partial=partial)


def _gn_call(dev, form, pr, x, out, ss, res):
    if form == "silu":
        return ops.groupnorm_silu_cl(x, pr["b"], pr["gamma"].to(dev), pr["beta"].to(dev), scale_shift=ss, residual=res, out=out)
    return ops.groupnorm_apply_cl(x, pr["b"], pr["gamma"].to(dev), pr["beta"].to(dev), pr["partial"].to(dev), 3, scale_shift=ss, residual=res, out=out)


@covers("lfdm_groupnorm_silu_cl_f32", "L1+L2+L3", dict(scale_shift=[(12, 4), (5, 1)], out="x's buffer"), "one kernel pair; scale_shift read by scalar loads")
@covers("lfdm_groupnorm_apply_cl_f32", "L1+L2+L3", dict(scale_shift=[(12, 4), (5, 1)], out="x's buffer"), "one kernel; scale_shift read by scalar loads")
@pytest.mark.parametrize("form", ["silu", "apply"])
@pytest.mark.parametrize("c", [64, 128])
def test_groupnorm_layouts(backend, form, c):
    """x / out / residual are dense rows (the entry points take no row stride for them); scale_shift is a column window of a wider
    table (cvpr23_lfdm_amd/unet.py hands in ss[:, o:o + 2C]): aligned (L1), ragged (L3: odd stride, one float in - scalar loads,
    supported), and the normalisation in place (L2: out = x, as UNet._gn runs it)."""
    dev = backend
    pr = _gn_problem(c)
    out0 = _gn_call(dev, form, pr, pr["x"].to(dev).clone(), None, pr["ss"].to(dev), pr["res"].to(dev)).cpu()
    assert_close(out0, pr["ref"], TOL, "groupnorm %s, contiguous" % form)
    for spec in ((12, 4), (5, 1)):
        ss, chk = window(pr["ss"].to(dev), ld_extra=spec[0], col_off=spec[1], guard_rows=1)
        assert ss.stride(0) > 2 * c
        for inplace in (False, True):
            x = pr["x"].to(dev).clone()
            out = x if inplace else torch.full_like(x, float("nan"))
            got = _gn_call(dev, form, pr, x, out, ss, pr["res"].to(dev)).cpu()
            chk("groupnorm %s scale_shift %s" % (form, spec))
            no_nan(got, "groupnorm %s" % form)
            assert torch.equal(got, out0), "groupnorm %s: scale_shift window %s, in place %s: differs from the contiguous call" % (form, spec, inplace)


@covers("lfdm_groupnorm_silu_cl_f32", "refusal", dict(x="+1 float", out="+1 float", residual="+1 float"), "refused: float4 rows")
@covers("lfdm_groupnorm_apply_cl_f32", "refusal", dict(x="+1 float", out="+1 float", residual="+1 float"), "refused: float4 rows")
@covers("lfdm_layernorm_cl_f32", "refusal", dict(x="+1 float", out="+1 float", gamma="+1 float"), "refused: float4 rows")
@pytest.mark.parametrize("which", ["x", "out", "residual"])
@pytest.mark.parametrize("form", ["silu", "apply", "layernorm"])
def test_norms_refuse_rows_that_are_not_16_byte_aligned(backend, form, which):
    """GroupNorm and LayerNorm walk x / out / residual (LayerNorm: gamma) as float4 whatever the pointer: an operand that starts one float
    into an aligned buffer is refused (it was dereferenced as float4 before), and nothing is written."""
    dev = backend
    c = 64
    pr = _gn_problem(c)
    rows = pr["x"].shape[0]

    def dense_plus1(t):          # dense rows starting one float into an aligned buffer
        v, chk = window(t.reshape(1, -1).to(dev), ld_extra=8, col_off=1, guard_rows=1)
        return v[0].view(t.shape), chk

    x, out, res, gamma = pr["x"].to(dev).clone(), torch.full((rows, c), float("nan"), device=dev), pr["res"].to(dev), pr["gamma"].to(dev)
    checks = []
    if which == "x":
        x, chk = dense_plus1(pr["x"])
    elif which == "out":
        out, chk = dense_plus1(torch.full((rows, c), float("nan")))
    elif form == "layernorm":
        gamma, chk = dense_plus1(pr["gamma"])
    else:
        res, chk = dense_plus1(pr["res"])
    checks.append((which, chk))
    if form == "layernorm":
        _refused("lfdm_layernorm_cl_f32 failed.*layernorm", lambda: ops.layernorm_cl(x, gamma, out=out), checks, [out])
    else:
        word = "lfdm_groupnorm_silu_cl_f32 failed.*groupnorm" if form == "silu" else "lfdm_groupnorm_apply_cl_f32 failed.*groupnorm_apply"
        _refused(word, lambda: _gn_call(dev, form, pr, x, out, pr["ss"].to(dev), res), checks, [out])


# ------------------------------------------------------------------------------------------ small dense layers
@covers("lfdm_linear_small_f32", "L1+L3", dict(x=[(4, 0), (1, 0)], w=[(12, 4), (3, 1)], y=[(4, 4), (5, 1)]), "one scalar kernel")
@covers("lfdm_sinusoidal_f32", "L1+L3", dict(out=[(4, 4), (5, 1)]), "one scalar kernel")
@pytest.mark.parametrize("lay", ["wide", "ragged"])
def test_linear_small_and_sinusoidal_layouts(backend, lay):
    """linear_small (x / w / y each with its own row stride; the package passes column slices of the conditioning weight,
    UNet.cond_tables) and sinusoidal (ldo): scalar kernels, so the ragged layouts are supported and bit-identical."""
    dev = backend
    sx, sw, sy = ((4, 0), (12, 4), (4, 4)) if lay == "wide" else ((1, 0), (3, 1), (5, 1))
    b = 3
    t = torch.tensor([999, 500, 0], dtype=torch.int32)
    freqs = ops.sinusoidal_freqs(64, dev)
    emb0 = ops.sinusoidal(t.to(dev), freqs, b, 64).cpu()
    out, chk = _nan_out(b, 64, dev, sy)
    emb = ops.sinusoidal(t.to(dev), freqs, b, 64, out=out).cpu()
    chk("sinusoidal out")
    half = 32
    e = t.long()[:, None] * torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1)))[None, :]
    assert_close(emb, torch.cat((e.sin(), e.cos()), dim=-1), 2e-5, "sinusoidal")      # (test_linear_small_and_sinusoidal's bar)
    assert torch.equal(emb, emb0)
    x, w2, b2 = rnd(b, 1024, seed=3), rnd(130, 1024, seed=4, scale=0.05), rnd(130, seed=5)
    y0 = ops.linear_small(x.to(dev), w2.to(dev), b2.to(dev), act_in=ops.ACT_SILU).cpu()
    xv, cx = window(x.to(dev), ld_extra=sx[0], col_off=sx[1])
    wv, cw = window(w2.to(dev), ld_extra=sw[0], col_off=sw[1])
    yv, cy = _nan_out(b, 130, dev, sy)
    y = ops.linear_small(xv, wv, b2.to(dev), act_in=ops.ACT_SILU, out=yv).cpu()
    for c_ in (cx, cw, cy):
        c_("linear_small")
    no_nan(y, "linear_small")
    assert_close(y, F.linear(F.silu(x.double()), w2.double(), b2.double()).float(), TOL, "silu+linear")
    assert torch.equal(y, y0), "linear_small: same kernel, other addresses, other result"


@covers("lfdm_conv_planar_in_cl_f32", "L1+L3", dict(out=[(12, 4), (1, 0), (4, 1)], bias="+1 float", add_term="+1 float", x="batch window"),
        "float4 epilogue (L1) / scalar epilogue (L3)")
@pytest.mark.parametrize("lay", ["wide", "ldo_mod4", "out_plus1", "bias_plus1", "add_plus1"])
def test_conv_planar_in_layouts(backend, lay):
    """The stem convolution: ldo, and the scalar epilogue behind its alignment test (small.hip `vec`); the planar input in a batch window."""
    dev = backend
    b, t, s = 2, 2, 6
    x = rnd(b, 7, t, s, s, seed=1)
    wt, bias, add = rnd(64, 3, 1, 7, 7, seed=2, scale=0.1), rnd(64, seed=3), rnd(b, 64, s, s, seed=4)
    ref = F.conv3d(x[:, :3].double(), wt.double(), bias.double(), padding=(0, 3, 3)) + add.double().unsqueeze(2)
    wp = ops.pack_planar_in_weight(wt).to(dev)
    rows = b * t * s * s
    out0 = ops.conv_planar_in_cl(x.to(dev), b, 3, 7, t, s, s, wp, 7, 7, 64, bias=bias.to(dev), add_term=to_cl(add).to(dev)).cpu()
    checks = []
    out, chk = _nan_out(rows, 64, dev, {"wide": (12, 4), "ldo_mod4": (1, 0), "out_plus1": (4, 1)}.get(lay, (4, 0)))
    checks.append(chk)
    bv, av = bias.to(dev), to_cl(add).to(dev)
    if lay == "bias_plus1":
        v, chk = window(bias.view(1, -1).to(dev), ld_extra=4, col_off=1)
        bv = v[0]
        checks.append(chk)
    if lay == "add_plus1":
        v, chk = window(to_cl(add).reshape(1, -1).to(dev), ld_extra=4, col_off=1)
        av = v[0].view(b * s * s, 64)
        checks.append(chk)
    assert (lay == "wide") == (aligned16(out) and aligned16(bv) and aligned16(av) and out.stride(0) % 4 == 0), "the case is not on the side of the gate it names"
    got = ops.conv_planar_in_cl(x.to(dev), b, 3, 7, t, s, s, wp, 7, 7, 64, bias=bv, add_term=av, out=out).cpu()
    for chk in checks:
        chk("conv_planar_in %s" % lay)
    no_nan(got, "conv_planar_in")
    assert_close(unet_from_cl(got, b, t, s, s), ref.float(), TOL, "conv_planar_in %s" % lay)
    if lay == "wide":          # (the scalar epilogue is another variant: parity bar only)
        assert torch.equal(got, out0), "conv_planar_in: float4 epilogue in a window against the contiguous call"


@covers("lfdm_heads_cl_to_planar_f32", "L1+refusal", dict(y="[:, :C] / [:, C:] of one window (8, 4)"), "one kernel; ld % 4 / 16-byte refusals")
@covers("lfdm_heads_res_cl_to_planar_f32", "L1+refusal", dict(y="[:, :C] / [:, C:] of one window (8, 4)", x0=(4, 0), x1=(12, 4)), "one kernel; refusals")
@pytest.mark.parametrize("lay", ["wide", "ld_mod4", "y_plus1", "ld0_mod4", "x0_plus1"])
def test_heads_layouts(backend, lay):
    """The output heads read the two column halves of one (rows, 2C) buffer (UNet: y[:, :dim] / y[:, dim:]) plus, in the res form, two
    sources with their own strides.  Rows are read as float4: ld % 4 != 0 and pointers that are not 16-byte aligned are refused."""
    dev = backend
    b, t, s, c, c0, c1 = 2, 2, 6, 64, 32, 16
    rows = b * t * s * s
    yf, yo = rnd(b, c, t, s, s, seed=5), rnd(b, c, t, s, s, seed=6)
    wf, bf, wo, bo = rnd(2, c, seed=7, scale=0.2), rnd(2, seed=8), rnd(1, c, seed=9, scale=0.2), rnd(1, seed=10)
    x0, x1, we = rnd(rows, c0, seed=11), rnd(rows, c1, seed=12), rnd(3, c0 + c1, seed=13, scale=0.2)
    ref = torch.cat((F.conv3d(yf.double(), wf.double().view(2, c, 1, 1, 1), bf.double()), F.conv3d(yo.double(), wo.double().view(1, c, 1, 1, 1), bo.double())), dim=1)
    extra = (torch.cat((x0, x1), dim=1).double() @ we.double().t()).view(b, t, s * s, 3).permute(0, 3, 1, 2).reshape(b, 3, t, s, s)
    y2 = torch.cat((unet_to_cl(yf), unet_to_cl(yo)), dim=1)
    wd = [v.to(dev) for v in (wf, bf, wo, bo)]
    spec_y = {"ld_mod4": (1, 0), "y_plus1": (8, 1)}.get(lay, (8, 4))
    yw, cy = window(y2.to(dev), ld_extra=spec_y[0], col_off=spec_y[1])
    x0w, c0k = window(x0.to(dev), ld_extra={"ld0_mod4": 1}.get(lay, 4), col_off={"x0_plus1": 1}.get(lay, 0))
    x1w, c1k = window(x1.to(dev), ld_extra=12, col_off=4)
    checks = [("y", cy), ("x0", c0k), ("x1", c1k)]
    plain = lambda o: ops.heads_cl_to_planar(yw[:, :c], yw[:, c:], *wd, b, t, s * s, out=o)
    withres = lambda o: ops.heads_res_cl_to_planar(yw[:, :c], yw[:, c:], *wd, x0w, x1w, we.to(dev), b, t, s * s, out=o)
    if lay == "wide":
        o1 = torch.full((b, 3, t, s * s), float("nan"), device=dev)
        o2 = torch.full((b, 3, t, s * s), float("nan"), device=dev)
        plain(o1), withres(o2)
        for what, chk in checks:
            chk("heads, operand %s" % what)
        no_nan(o1, "heads"), no_nan(o2, "heads_res")
        assert_close(o1.cpu().reshape(b, 3, t, s, s), ref.float(), TOL, "heads")
        assert_close(o2.cpu().reshape(b, 3, t, s, s), (ref + extra).float(), TOL, "heads_res")
        yc = y2.to(dev)
        assert torch.equal(o1, ops.heads_cl_to_planar(yc[:, :c], yc[:, c:], *wd, b, t, s * s))
        assert torch.equal(o2, ops.heads_res_cl_to_planar(yc[:, :c], yc[:, c:], *wd, x0.to(dev), x1.to(dev), we.to(dev), b, t, s * s))
        return
    if lay in ("ld_mod4", "y_plus1"):
        o = torch.full((b, 3, t, s * s), float("nan"), device=dev)
        _refused("lfdm_heads_cl_to_planar_f32 failed.*heads", lambda: plain(o), checks, [o])
    o = torch.full((b, 3, t, s * s), float("nan"), device=dev)
    _refused("lfdm_heads_res_cl_to_planar_f32 failed.*heads_res", lambda: withres(o), checks, [o])


# ------------------------------------------------------------------------------------------ element-wise / layout helpers
@covers("lfdm_affine_act_cl_f32", "L1+L2+refusal", dict(x=[(4, 0), (1, 0), (4, 1)], out=[(12, 4), (1, 0), (4, 1)]), "one float4 kernel; refusals")
@pytest.mark.parametrize("lay", ["wide", "inplace", "ldx_mod4", "ldo_mod4", "x_plus1", "out_plus1", "a_plus1"])
def test_affine_act_layouts(backend, lay):
    dev = backend
    n, c, h, w = 2, 32, 6, 6
    x = rnd(n, c, h, w, seed=1)
    a, bb = rnd(c, seed=2), rnd(c, seed=3)
    ref = F.relu(x * a.view(1, c, 1, 1) + bb.view(1, c, 1, 1))
    out0 = ops.affine_act_cl(to_cl(x).to(dev), a.to(dev), bb.to(dev), ops.ACT_RELU).cpu()
    xv, cx = window(to_cl(x).to(dev), ld_extra={"ldx_mod4": 1}.get(lay, 4), col_off={"x_plus1": 1}.get(lay, 0))
    ov, co = _nan_out(n * h * w, c, dev, {"ldo_mod4": (1, 0), "out_plus1": (4, 1)}.get(lay, (12, 4)))
    av, ca = window(a.view(1, c).to(dev), ld_extra=4, col_off=1 if lay == "a_plus1" else 0)
    checks = [("x", cx), ("out", co), ("a", ca)]
    if lay in ("wide", "inplace"):
        got = ops.affine_act_cl(xv, av[0], bb.to(dev), ops.ACT_RELU, out=xv if lay == "inplace" else ov).cpu()
        for what, chk in checks:
            chk("affine_act %s" % what)
        no_nan(got, "affine_act")
        assert_close(from_cl(got, n, h, w), ref, TOL, "affine")
        assert torch.equal(got, out0)
    else:
        _refused("lfdm_affine_act_cl_f32 failed.*affine_act", lambda: ops.affine_act_cl(xv, av[0], bb.to(dev), ops.ACT_RELU, out=ov), checks, [ov])


@covers("lfdm_planar_to_cl_f32", "L1+L3", dict(out=[(12, 4), (1, 0), (4, 1)]), "one scalar kernel")
@covers("lfdm_cl_to_planar_f32", "L1+L3", dict(x=[(12, 4), (1, 0), (4, 1)]), "one scalar kernel")
@pytest.mark.parametrize("spec", [(12, 4), (1, 0), (4, 1)], ids=["wide", "ld_mod4", "plus1"])
def test_planar_cl_transposes_layouts(backend, spec):
    dev = backend
    n = 2
    y = rnd(n, 40, 7 * 5, seed=4)
    out, chk = _nan_out(n * 35, 40, dev, spec)
    cl = ops.planar_to_cl(y.to(dev), n, 40, 35, out=out)
    chk("planar_to_cl")
    assert torch.equal(cl.cpu(), y.permute(0, 2, 1).reshape(n * 35, 40))
    back = ops.cl_to_planar(cl, n, 40, 35)          # reads the windowed rows: a gap read would show as NaN / a wrong value
    chk("cl_to_planar")
    assert torch.equal(back.cpu(), y)


@covers("lfdm_cfg_combine_f32", "L2", dict(out="cond_eps / null_eps"), "one kernel")
@pytest.mark.parametrize("alias", ["cond", "null"])
def test_cfg_combine_in_place(backend, alias):
    """out may alias an input (lfdm_hip.h): both inputs, odd length."""
    dev = backend
    n = 3 * 5 * 7 * 7 + 3
    ce, ne = rnd(n, seed=1), rnd(n, seed=2)
    ref = ne.double() + (ce.double() - ne.double()) * 2.5
    a, b_ = ce.to(dev).clone(), ne.to(dev).clone()
    out0 = ops.cfg_combine(a, b_, 2.5, torch.empty(n, device=dev)).cpu()
    got = ops.cfg_combine(a, b_, 2.5, a if alias == "cond" else b_).cpu()
    assert_close(got, ref.float(), TOL, "cfg_combine")
    assert torch.equal(got, out0)


# ------------------------------------------------------------------------------------------ wrappers: a leading dimension needs adjacent columns
@pytest.mark.parametrize("family", ["conv", "groupnorm", "linear_small", "affine_act", "heads", "cl_to_planar", "colsum", "attention_fused"])
def test_wrappers_refuse_transposed_operands(backend, family):
    """Every wrapper hands .stride(0) to the library as a leading dimension; a transposed (column-strided) tensor would be read as
    something else.  One call per wrapper family: ValueError before anything reaches the library."""
    dev = backend
    sq = rnd(64, 64, seed=1).to(dev)
    tr = sq.t()
    assert tr.stride(1) != 1
    from cvpr23_lfdm_amd import train_ops
    calls = {
        "conv": lambda: ops.conv_params(tr, ops.pack_conv_weight(rnd(64, 64, 1, 1)).to(dev), 64, 1, 1, 1, 8, 8),
        "groupnorm": lambda: ops.groupnorm_silu_cl(tr, 1, sq[0], sq[1]),
        "linear_small": lambda: ops.linear_small(tr, sq),
        "affine_act": lambda: ops.affine_act_cl(tr, sq[0], sq[1]),
        "heads": lambda: ops.heads_gn_res_cl_to_planar(tr, sq, 1, sq[0], sq[1], sq[:2, :32], sq[0, :2], sq[:1, :32], sq[0, :1], sq, None, sq[:3].contiguous(), 1, 1, 64),
        "cl_to_planar": lambda: ops.cl_to_planar(tr, 1, 64, 64),
        "colsum": lambda: train_ops.colsum(tr),
        "attention_fused": lambda: ops.linear_attention_fused_cl(tr, torch.zeros(3, 8, 8, 64, 4, device=dev), 1, 64),
    }
    with pytest.raises(ValueError, match="adjacent columns|contiguous tensor is needed"):
        calls[family]()


# ------------------------------------------------------------------------------------------ UNet: the fused res_gn path is decided up front
def _resblock_setup(dev):
    import synth
    from cvpr23_lfdm_amd.unet import Unet3D
    u = Unet3D(dim=64, channels=259, out_grid_dim=2, out_conf_dim=1, use_bert_text_cond=True)
    u.load_state_dict(synth.unet_state())
    u.to(dev).eval()
    batch, frames, s = 1, 2, 8          # 128 pixels per sample: one 128-row tile of fused GroupNorm statistics
    x = (rnd(batch * frames * s * s, 64, seed=31) * 0.7).to(dev)
    run = lambda: u._resblock(u.packed(), "downs.1.0.", x.clone(), None, batch, frames, s, None, 128, "t.out").clone()
    return u, run


def _spy_conv_launch(monkeypatch, fail_on_res_gn=False):
    """Records whether each lfdm_conv2d_cl_f32 launch of the package carried res_gn_*; optionally fails exactly those."""
    seen = []
    real = ops.conv_launch

    def launch(p):
        seen.append(bool(p.res_gn_partial))
        if fail_on_res_gn and p.res_gn_partial:
            raise RuntimeError("lfdm_conv2d_cl_f32 failed (-2): injected launch failure")
        return real(p)

    monkeypatch.setattr(ops, "conv_launch", launch)
    return seen


def test_resblock_fused_res_gn_failure_propagates(backend, monkeypatch):
    """A failure of the fused res_gn launch is an error of the step: it is no longer swallowed and silently recomputed on the two-launch path."""
    u, run = _resblock_setup(backend)
    seen = _spy_conv_launch(monkeypatch, fail_on_res_gn=True)
    with pytest.raises(RuntimeError, match="injected launch failure"):
        run()
    assert seen[-1] is True


def test_resblock_outside_the_pointwise_schedule_takes_two_launches(backend, monkeypatch):
    """Where lfdm_conv2d_schedule does not answer 3 (here: LFDM_PW=0) the block runs GroupNorm + res_conv as two launches without ever
    trying the fused one - no exception is raised and caught on the way - and equals the fused result at the parity bar."""
    import cvpr23_lfdm_amd.unet as unet_mod
    u, run = _resblock_setup(backend)
    seen = _spy_conv_launch(monkeypatch)
    fused = run()
    assert seen == [False, False, True], "the fused res_gn launch was not taken where schedule 3 is available: %s" % seen
    del seen[:]
    monkeypatch.setenv("LFDM_PW", "0")
    two = run()
    assert seen == [False, False, False], "a res_gn launch was tried outside schedule 3: %s" % seen
    del seen[:]
    monkeypatch.delenv("LFDM_PW")
    monkeypatch.setattr(unet_mod, "_RES_GN", False)
    plain = run()
    assert seen == [False, False, False]
    no_nan(fused, "resblock")
    assert_close(fused, plain, TOL, "ResnetBlock: fused res_gn launch against GroupNorm + res_conv")
    assert_close(two, plain, TOL, "ResnetBlock, LFDM_PW=0 against LFDM_RES_GN=0")


# ------------------------------------------------------------------------------------------ oracle/make_golden.py --full
def test_make_golden_full_choices_all_dispatch():
    """Every `choices` value of make_golden.py --full is a key of the dispatch table (read from the source: no generator runs, the
    reference is not imported)."""
    with open(os.path.join(REPO, "oracle", "make_golden.py")) as f:
        tree = ast.parse(f.read())
    choices, keys = None, None
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument" and node.args and \
                isinstance(node.args[0], ast.Constant) and node.args[0].value == "--full":
            choices = [ast.literal_eval(e) for kw in node.keywords if kw.arg == "choices" for e in kw.value.elts]
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and getattr(node.targets[0], "id", "") == "full" and isinstance(node.value, ast.Dict):
            keys = [ast.literal_eval(k) for k in node.value.keys]
            assert all(isinstance(v, ast.Lambda) for v in node.value.values), "dispatch entries are deferred calls"
    assert choices and keys, "could not find --full's choices / dispatch table"
    assert len(set(keys)) == len(keys)
    assert sorted(choices) == sorted(keys), "--full choices without a dispatch entry: %s; entries without a choice: %s" % (
        sorted(set(choices) - set(keys)), sorted(set(keys) - set(choices)))


# ------------------------------------------------------------------------------------------ pointwise schedule: res_gn with out aliasing the residual
@covers("lfdm_conv2d_cl_f32", "L1+L2+refusal", dict(src0=(4, 0), src1=(12, 4), out="residual's view (4, 4)"), "schedule 3 with res_gn_*; refused off schedule 3")
@pytest.mark.parametrize("lay", ["contiguous", "wide", "ldo_mod4", "out_plus1", "ld0_mod4", "src0_plus1"])
def test_conv_pointwise_res_gn_in_place(backend, lay, monkeypatch):
    """lfdm_conv_params.res_gn_* (h + res_conv(x) with block2's GroupNorm + SiLU in the epilogue) with out = residual, as the sampler runs
    it: in windows (bit-identical to the contiguous call), and refused - nothing written - for a layout schedule 3 cannot take."""
    dev = backend
    c0, c1, cout, b, t, h, w, nchunk, groups = 32, 64, 128, 2, 2, 4, 4, 2, 8
    n, pixels = b * t, t * h * w
    x = rnd(n, c0 + c1, h, w, seed=1)
    wt = rnd(cout, c0 + c1, 1, 1, seed=2, scale=1.0 / math.sqrt(c0 + c1))
    bias, gamma, beta = rnd(cout, seed=3), rnd(cout, seed=4) * 0.3 + 1, rnd(cout, seed=5) * 0.3
    raw = rnd(n * h * w, cout, seed=6) * 1.5 + 0.2
    rs = raw.double().view(b, pixels, cout)
    act = F.silu(F.group_norm(rs.permute(0, 2, 1), groups, gamma.double(), beta.double(), eps=1e-5).permute(0, 2, 1)).reshape(n * h * w, cout)
    ref = (to_cl(F.conv2d(x.double(), wt.double(), bias.double())) + act).float()
    rg = rs.view(b, nchunk, pixels // nchunk, groups, cout // groups)
    partial = torch.stack([rg.sum(dim=(2, 4)), (rg * rg).sum(dim=(2, 4))], dim=-1).float().contiguous().view(b * nchunk, 2 * groups)
    xs = to_cl(x)
    wd = ops.pack_conv_weight(wt).to(dev)
    res_gn = dict(partial=partial.to(dev), nchunk=nchunk, pixels=pixels, gamma=gamma.to(dev), beta=beta.to(dev), groups=groups)

    def launch(src0, src1, out):
        kw = dict(src1=src1, bias=bias.to(dev), residual=out, out=out, res_gn=res_gn)
        pp, _ = ops.conv_params(src0, wd, cout, 1, 1, n, h, w, **kw)
        sched = ops.conv_schedule(pp)
        return sched, (lambda: ops.conv2d_cl(src0, wd, cout, 1, 1, n, h, w, **kw))

    out0 = raw.clone().to(dev)
    sched, go = launch(xs[:, :c0].contiguous().to(dev), xs[:, c0:].contiguous().to(dev), out0)
    assert sched == 3
    got0 = go().cpu()
    assert_close(got0, ref, TOL, "res_gn in place, contiguous")
    if lay == "contiguous":
        return
    s0 = {"ld0_mod4": (1, 0), "src0_plus1": (4, 1)}.get(lay, (4, 0))
    so = {"ldo_mod4": (1, 0), "out_plus1": (4, 1)}.get(lay, (4, 4))
    src0, k0 = window(xs[:, :c0].to(dev), ld_extra=s0[0], col_off=s0[1])
    src1, k1 = window(xs[:, c0:].to(dev), ld_extra=12, col_off=4)
    out, ko = window(raw.to(dev), ld_extra=so[0], col_off=so[1])
    sched, go = launch(src0, src1, out)
    if lay == "wide":
        assert sched == 3
        got = go().cpu()
        for k_ in (k0, k1, ko):
            k_("res_gn in place")
        no_nan(got, "res_gn in place")
        assert torch.equal(got, got0), "schedule 3 in both layouts, other result"
    else:
        assert sched != 3, "schedule 3 kept for %s" % lay
        with pytest.raises(RuntimeError, match="lfdm_conv2d_cl_f32 failed.*res_gn"):
            go()
        for k_ in (k0, k1, ko):
            k_("res_gn refused")
        assert torch.equal(out.cpu(), raw), "the refused call changed its in/out operand"


# ------------------------------------------------------------------------------------------ fused attention forms (ldx, ldo)
def _plus1_table(t, dev):
    """A dense table starting one float into an aligned buffer."""
    v, chk = window(t.reshape(1, -1).to(dev), ld_extra=8, col_off=1)
    return v[0].view(t.shape), chk


@functools.lru_cache(maxsize=None)
def _tattn_problem(c, frames, b, s):
    import lfdm_oracle as O
    from test_ops_parity import _attention_ref
    hw = s * s
    x = rnd(b, c, frames, s, s, seed=1) * 2 + 0.5
    gamma = rnd(1, c, 1, 1, 1, seed=2) * 0.3 + 1
    wq = rnd(768, c, seed=3, scale=1.0 / math.sqrt(c))
    bias = O.rel_pos_bias(rnd(32, 8, seed=4), frames).contiguous()
    cos, sin = O.rotary_tables(1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)), frames)
    normed = O.channel_layernorm(x, gamma)
    tokens = normed.permute(0, 3, 4, 2, 1).reshape(b, hw, frames, c)
    ref = _attention_ref(tokens @ wq.t(), bias, (cos, sin)).permute(0, 2, 1, 3).reshape(-1, 256)
    tokens1 = normed.permute(0, 2, 3, 4, 1).reshape(b, frames, hw, c)
    ref1 = _attention_ref(tokens1 @ wq.t(), None, None).reshape(-1, 256)
    wf = (wq * gamma.reshape(1, -1)).contiguous()
    return dict(x=unet_to_cl(x), wf=wf, wsum=wf.double().sum(dim=1).float(), bias=bias, cos=cos[:, 0::2].contiguous(), sin=sin[:, 0::2].contiguous(),
                ref=ref, ref_spatial=ref1, hw=hw)


@covers("lfdm_temporal_attention_fused_cl_f32", "L1+L3+refusal", dict(x=[(4, 0), (12, 4), (1, 0), (4, 1)], bias="+1 float"),
        "bias_vec (aligned table, L % 4 == 0) / scalar bias loads; ldx % 4, x & 15 refused")
@covers("lfdm_temporal_attention_fused_out_cl_f32", "L1+L3+refusal", dict(x=[(4, 0), (12, 4), (1, 0), (4, 1)], out=[(12, 4), (1, 0), (4, 1)], bias="+1 float"),
        "scalar output stores: any ldo; ldx % 4, x & 15 refused")
@covers("lfdm_attention_lowres_cl_f32", "L1+refusal", dict(x=[(4, 0), (12, 4), (1, 0), (4, 1)], out="+1 float"), "one kernel; refusals")
@pytest.mark.parametrize("lay", ["wide", "wide_off", "bias_plus1", "ldx_mod4", "x_plus1", "out_ragged"])
def test_temporal_attention_fused_layouts(backend, lay):
    """The three fused temporal-attention forms on row slices (ldx, ldo): C = 64, 4 frames (L % 4 == 0, so the bias table's alignment alone
    decides between float4 and scalar bias loads)."""
    dev = backend
    c, frames, b, s = 64, 4, 2, 2
    pr = _tattn_problem(c, frames, b, s)
    hw, rows = pr["hw"], pr["x"].shape[0]
    tab = dict(bias=pr["bias"].to(dev), rot_cos=pr["cos"].to(dev), rot_sin=pr["sin"].to(dev))
    wf, wsum = pr["wf"].to(dev), pr["wsum"].to(dev)
    wo = rnd(c, 256, seed=9, scale=1.0 / 16)
    wqp, wop = (t.to(dev) for t in ops.pack_tattn_weights(pr["wf"], wo))
    ref_out = pr["x"] + pr["ref"] @ wo.t()
    x0 = pr["x"].to(dev)
    base = [ops.temporal_attention_fused_cl(x0, wf, b, frames, hw, **tab).cpu(),
            ops.temporal_attention_fused_out_cl(x0, wqp, wop, b, frames, hw, **tab).cpu(),
            ops.attention_lowres_cl(x0, wf, wsum, b, frames, hw, 0, **tab).cpu()]
    for got, ref, what in zip(base, (pr["ref"], ref_out, pr["ref"]), ("fused", "fused_out", "lowres")):
        assert_close(got, ref, TOL, "temporal attention %s, contiguous" % what)
    sx = {"wide": (4, 0), "wide_off": (12, 4), "ldx_mod4": (1, 0), "x_plus1": (4, 1)}.get(lay, (4, 0))
    xv, cx = window(x0, ld_extra=sx[0], col_off=sx[1])
    checks = [("x", cx)]
    if lay == "bias_plus1":
        tab["bias"], cb = _plus1_table(pr["bias"], dev)
        checks.append(("bias", cb))
    ov, co = _nan_out(rows, c, dev, {"out_ragged": (1, 0)}.get(lay, (12, 4)))
    checks.append(("out", co))
    calls = [lambda: ops.temporal_attention_fused_cl(xv, wf, b, frames, hw, **tab),
             lambda: ops.temporal_attention_fused_out_cl(xv, wqp, wop, b, frames, hw, out=ov, **tab),
             lambda: ops.attention_lowres_cl(xv, wf, wsum, b, frames, hw, 0, **tab)]
    names = ["lfdm_temporal_attention_fused_cl_f32", "lfdm_temporal_attention_fused_out_cl_f32", "lfdm_attention_lowres_cl_f32"]
    if lay in ("ldx_mod4", "x_plus1"):
        for call, name in zip(calls, names):
            _refused(name + " failed", call, checks, [ov])
        return
    for call, want, name in zip(calls, base, names):
        got = call().cpu()
        for what, chk in checks:
            chk("%s %s, operand %s" % (name, lay, what))
        no_nan(got, name)
        if lay == "bias_plus1":          # (scalar instead of float4 bias loads: another variant of the kernel - parity bar only)
            assert_close(got, ref_out if name.endswith("fused_out_cl_f32") else pr["ref"], TOL, "%s %s" % (name, lay))
        else:
            assert torch.equal(got, want), "%s %s: differs from the contiguous call (max abs %.3e)" % (name, lay, float((got - want).abs().max()))
    if lay == "wide":           # lowres: out one float in is refused (float4 stores)
        o1, c1 = _plus1_table(torch.full((rows, 256), float("nan")), dev)
        _refused("lfdm_attention_lowres_cl_f32 failed.*attention_lowres", lambda: ops.attention_lowres_cl(x0, wf, wsum, b, frames, hw, 0, out=o1, **tab),
                 [("out", c1)], [o1])


@covers("lfdm_linear_attention_fused_cl_f32", "L1+refusal", dict(x=[(4, 0), (12, 4), (1, 0), (4, 1)]), "one kernel chain; ldx % 4, x & 15 refused")
@covers("lfdm_linear_attention_fused_out_cl_f32", "L1+refusal", dict(x=[(4, 0), (12, 4), (1, 0), (4, 1)], out=[(12, 4), (1, 0), (4, 1)]),
        "one kernel chain; ldx / ldo % 4, x / out & 15 refused")
@covers("lfdm_linear_attention_lowres_cl_f32", "L1+refusal", dict(x=[(4, 0), (12, 4), (1, 0), (4, 1)]), "one kernel; refusals")
@pytest.mark.parametrize("lay", ["wide", "wide_off", "ldx_mod4", "x_plus1", "ldo_mod4", "out_plus1"])
def test_linear_attention_fused_layouts(backend, lay):
    dev = backend
    nf, c, hw = 2, 64, 16
    x = rnd(nf, hw, c, seed=1) * 2 + 0.3
    gamma = rnd(c, seed=2) * 0.3 + 1
    wq = rnd(768, c, seed=3, scale=1.0 / math.sqrt(c))
    xd = x.double()
    normed = (xd - xd.mean(dim=-1, keepdim=True)) / (xd.var(dim=-1, unbiased=False, keepdim=True) + 1e-5).sqrt() * gamma.double()
    qkv = normed @ wq.double().t()
    q, k, v = [z.reshape(nf, hw, 8, 32).permute(0, 2, 3, 1) for z in qkv.chunk(3, dim=-1)]
    q, k = q.softmax(dim=-2) * (32 ** -0.5), k.softmax(dim=-1)
    ref = torch.einsum("bhde,bhdn->bhen", torch.einsum("bhdn,bhen->bhde", k, v), q).permute(0, 3, 1, 2).reshape(nf * hw, 256)
    wo, bo = rnd(c, 256, seed=4, scale=1.0 / 16), rnd(c, seed=5)
    ref2 = (xd.reshape(-1, c) + ref @ wo.double().t() + bo.double()).float()
    wf = (wq * gamma.reshape(1, -1)).contiguous()
    wsum = wf.double().sum(dim=1).float().to(dev)
    wp, wop = ops.pack_linattn_weights(wf).to(dev), ops.pack_linattn_out_weight(wo).to(dev)
    x0 = x.reshape(-1, c).to(dev)
    base = [ops.linear_attention_fused_cl(x0, wp, nf, hw).cpu(), ops.linear_attention_fused_out_cl(x0, wp, wop, bo.to(dev), nf, hw).cpu(),
            ops.linear_attention_lowres_cl(x0, wf.to(dev), wsum, nf, hw).cpu()]
    for got, r, what in zip(base, (ref.float(), ref2, ref.float()), ("fused", "fused_out", "lowres")):
        assert_close(got, r, TOL, "linear attention %s, contiguous" % what)
    sx = {"wide_off": (12, 4), "ldx_mod4": (1, 0), "x_plus1": (4, 1)}.get(lay, (4, 0))
    xv, cx = window(x0, ld_extra=sx[0], col_off=sx[1])
    ov, co = _nan_out(nf * hw, c, dev, {"ldo_mod4": (1, 0), "out_plus1": (4, 1)}.get(lay, (12, 4)))
    checks = [("x", cx), ("out", co)]
    calls = [lambda: ops.linear_attention_fused_cl(xv, wp, nf, hw), lambda: ops.linear_attention_fused_out_cl(xv, wp, wop, bo.to(dev), nf, hw, out=ov),
             lambda: ops.linear_attention_lowres_cl(xv, wf.to(dev), wsum, nf, hw)]
    names = ["lfdm_linear_attention_fused_cl_f32", "lfdm_linear_attention_fused_out_cl_f32", "lfdm_linear_attention_lowres_cl_f32"]
    for i, (call, want, name) in enumerate(zip(calls, base, names)):
        if lay in ("ldx_mod4", "x_plus1") or (i == 1 and lay in ("ldo_mod4", "out_plus1")):
            _refused(name + " failed", call, checks, [ov])
            continue
        got = call().cpu()
        for what, chk in checks:
            chk("%s %s, operand %s" % (name, lay, what))
        no_nan(got, name)
        assert torch.equal(got, want), "%s %s: differs from the contiguous call" % (name, lay)


# ------------------------------------------------------------------------------------------ warp
@covers("lfdm_warp_cl_f32", "L1+refusal", dict(src=[(4, 0), (1, 0), (4, 1)], prev=[(12, 4), (1, 0), (4, 1)], out=[(4, 4), (1, 0), (4, 1)], flow="batch window"),
        "warp_cl_kernel<R> float4 rows; ld % 4 / 16-byte refusals")
@pytest.mark.parametrize("lay", ["wide", "ld_src_mod4", "src_plus1", "ld_prev_mod4", "prev_plus1", "ld_out_mod4", "out_plus1"])
def test_warp_cl_layouts(backend, lay):
    """Generator.apply_optical on channel slices: src / prev / out each with its own row stride, the flow / occlusion maps read in place
    from a batch-strided planar prediction."""
    import lfdm_oracle as O
    from test_ops_parity import _flow_case
    dev = backend
    b, t, c, res, fs = 2, 3, 8, 8, 8
    pred = _flow_case(b, t, fs, seed=c)
    src, prev = rnd(b, c, res, res, seed=1), rnd(b * t, c, res, res, seed=2)
    occ = (pred[:, 2:3] + 1) * 0.5
    ref = torch.cat([O.apply_optical(prev[bi * t + ti:bi * t + ti + 1], src[bi:bi + 1], pred[bi:bi + 1, :2, ti].permute(0, 2, 3, 1), occ[bi:bi + 1, :, ti])
                     for bi in range(b) for ti in range(t)], dim=0)
    pd0 = pred.to(dev)
    out0 = ops.warp_cl(to_cl(src).to(dev), b, t, res, res, pd0[:, 0], pd0[:, 1], pd0[:, 2], fs, fs, 3 * t * fs * fs, fs * fs,
                       prev=to_cl(prev).to(dev), occ_scale=0.5, occ_bias=0.5).cpu()
    assert_close(from_cl(out0, b * t, res, res), ref, TOL, "warp_cl blend, contiguous")
    pd, cp = window_batched(pred.to(dev), batch_extra=12, lead=4)
    sv, cs = window(to_cl(src).to(dev), ld_extra={"ld_src_mod4": 1}.get(lay, 4), col_off={"src_plus1": 1}.get(lay, 0))
    sp = {"ld_prev_mod4": (1, 0), "prev_plus1": (4, 1)}.get(lay, (12, 4))
    pv, cv = window(to_cl(prev).to(dev), ld_extra=sp[0], col_off=sp[1])
    ov, co = _nan_out(b * t * res * res, c, dev, {"ld_out_mod4": (1, 0), "out_plus1": (4, 1)}.get(lay, (4, 4)))
    checks = [("flow", cp), ("src", cs), ("prev", cv), ("out", co)]
    call = lambda: ops.warp_cl(sv, b, t, res, res, pd[:, 0], pd[:, 1], pd[:, 2], fs, fs, pd.stride(0), fs * fs, prev=pv, occ_scale=0.5, occ_bias=0.5, out=ov)
    if lay != "wide":
        _refused("lfdm_warp_cl_f32 failed.*warp_cl", call, checks, [ov])
        return
    got = call().cpu()
    for what, chk in checks:
        chk("warp_cl, operand %s" % what)
    no_nan(got, "warp_cl")
    assert torch.equal(got, out0), "warp_cl: windows against the contiguous call"


@covers("lfdm_warp_planar_f32", "L1+L3", dict(prev=[(4, 0), (1, 0), (4, 1)], flow="batch window", src="+1 float (many planes: unstaged kernel)"),
        "pixel kernel (c = 3); plane kernel staged (aligned src) / unstaged (src one float in)")
@pytest.mark.parametrize("lay", ["wide", "ld_prev_mod4", "prev_plus1", "planes_staged", "planes_src_plus1"])
def test_warp_planar_layouts(backend, lay):
    import lfdm_oracle as O
    from test_ops_parity import _flow_case
    dev = backend
    b, t = 2, 3
    res, fs, c = (8, 4, 400) if lay.startswith("planes") else (16, 8, 3)
    pred = _flow_case(b, t, fs, seed=res)
    src = torch.rand(b, c, res, res, generator=torch.Generator().manual_seed(5))
    occ = (pred[:, 2:3] + 1) * 0.5
    pd, cp = window_batched(pred.to(dev), batch_extra=12, lead=4)
    fsb, fst = pd.stride(0), fs * fs
    if lay.startswith("planes"):          # the LDS-staged plane kernel and, behind its alignment test, the unstaged one
        sv, cs = (src.to(dev), lambda what="": None) if lay == "planes_staged" else _plus1_table(src, dev)
        assert aligned16(sv) == (lay == "planes_staged")
        p0 = pred.to(dev)
        out0 = ops.warp_planar(src.to(dev), t, p0[:, 0], p0[:, 1], None, fs, fs, 3 * t * fs * fs, fst).cpu()
        ov = torch.full((b, c, t, res, res), float("nan"), device=dev)
        p = ops._warp_params(sv, ov, b, t, res, res, c, pd[:, 0], pd[:, 1], None, fs, fs, fsb, fst, None, 1.0, 0.0, 0, 0, 0, False)
        lib = ops._lib()
        lib.check(lib.lfdm_warp_planar_f32(ctypes.byref(p), ops._stream(lib)), "lfdm_warp_planar_f32")
        got = ov.cpu()
        cs("warp_planar src"), cp("warp_planar flow")
        no_nan(got, "warp_planar")
        ref = torch.stack([O.deform_input(src, pred[:, :2, ti].permute(0, 2, 3, 1)) for ti in range(t)], dim=2)
        assert_close(got, ref, TOL, "warp_planar deform, %s" % lay)
        if lay == "planes_staged":          # (the unstaged kernel is another variant: parity bar only)
            assert torch.equal(got, out0), "staged plane kernel: batch-strided maps against the contiguous call"
        return
    prev = torch.rand(b * t * res * res, 4, generator=torch.Generator().manual_seed(6))
    prev_nchw = from_cl(prev[:, :3].contiguous(), b * t, res, res).reshape(b, t, 3, res, res)
    ref2 = torch.stack([O.apply_optical(prev_nchw[:, ti], src, pred[:, :2, ti].permute(0, 2, 3, 1), occ[:, :, ti]) for ti in range(t)], dim=2)
    pv, cv = window(prev.to(dev), ld_extra={"ld_prev_mod4": 1}.get(lay, 4), col_off={"prev_plus1": 1}.get(lay, 0))
    got = ops.warp_planar(src.to(dev), t, pd[:, 0], pd[:, 1], pd[:, 2], fs, fs, fsb, fst, prev=pv, prev_is_cl=True, occ_scale=0.5, occ_bias=0.5).cpu()
    cv("warp_planar prev"), cp("warp_planar flow")
    no_nan(got, "warp_planar")
    assert_close(got, ref2, TOL, "warp_planar blend, %s" % lay)


# ------------------------------------------------------------------------------------------ small-N convolution, column sums, weight gradient
@covers("lfdm_conv2d_smalln_cl_f32", "L1+L3+refusal", dict(x=[(4, 0), (12, 4), (1, 0), (4, 1)], out=[(0, 0), (5, 1)]),
        "one kernel, scalar stores of `cout` columns only; ldx % 4, x & 15 refused")
@pytest.mark.parametrize("lay", ["wide", "out_ragged", "ldx_mod4", "x_plus1"])
def test_conv2d_smalln_layouts(backend, lay):
    """The generator's final 64 -> 3 convolution writes 3 of 4 columns (generator.py): the fourth column is a gap like any other - never
    written - and the output may sit at any 4-byte aligned address."""
    dev = backend
    cin, k, h, w, n = 16, 7, 20, 18, 2
    x = rnd(n, cin, h, w, seed=1)
    wt, bias = rnd(3, cin, k, k, seed=2, scale=1.0 / math.sqrt(cin * k * k)), rnd(3, seed=3)
    ref = torch.sigmoid(F.conv2d(x.double(), wt.double(), bias.double(), padding=k // 2)).float()
    wp, b4 = (v.to(dev) for v in ops.pack_smalln_weight(wt, bias))
    out0 = ops.conv2d_smalln_cl(to_cl(x).to(dev), wp, b4, 3, k, n, h, w, act=ops.ACT_SIGMOID)[:, :3].cpu()
    xv, cx = window(to_cl(x).to(dev), ld_extra={"ldx_mod4": 1, "wide": 12}.get(lay, 4), col_off={"x_plus1": 1, "wide": 4}.get(lay, 0))
    ov, co = window((n * h * w, 3), ld_extra=5 if lay == "out_ragged" else 1, col_off=1 if lay == "out_ragged" else 0, device=dev)
    call = lambda: ops.conv2d_smalln_cl(xv, wp, b4, 3, k, n, h, w, act=ops.ACT_SIGMOID, out=ov)
    if lay in ("ldx_mod4", "x_plus1"):
        _refused("lfdm_conv2d_smalln_cl_f32 failed.*conv2d_smalln", call, [("x", cx), ("out", co)], [ov])
        return
    got = call().cpu()
    cx("smalln x"), co("smalln out: only `cout` columns of a row are written")
    no_nan(got, "conv2d_smalln")
    assert_close(from_cl(got.contiguous(), n, h, w), ref, TOL, "conv2d_smalln %s" % lay)
    assert torch.equal(got, out0)


@covers("lfdm_colsum_f32", "L1+L3", dict(x=[(12, 4), (1, 0), (4, 1)]), "vector / scalar column walk")
@covers("lfdm_conv2d_wgrad_cl_f32", "L1+refusal", dict(x=[(4, 0), (1, 0), (4, 1)], dy=[(12, 4), (1, 0), (4, 1)]), "one kernel chain; ld % 4 / 16-byte refusals")
@pytest.mark.parametrize("lay", ["wide", "ldx_mod4", "x_plus1", "lddy_mod4", "dy_plus1"])
def test_conv_wgrad_and_colsum_layouts(backend, lay):
    """Weight and bias gradient on channel slices (autograd.py hands in column slices of a concatenated activation): ldx, lddy, ci_off, dbias."""
    from cvpr23_lfdm_amd import train_ops
    dev = backend
    n, cin, cout, k, res = 3, 8, 12, 3, 6
    x = rnd(n, cin, res, res, seed=1)
    wt = (rnd(cout, cin, k, k, seed=2) * 0.1).requires_grad_(True)
    y = F.conv2d(x, wt, padding=1)
    dy = rnd(*y.shape, seed=3)
    y.backward(dy)
    scale, ref_db = float(wt.grad.abs().max()), dy.sum(dim=(0, 2, 3))
    xc, dyc = to_cl(x).to(dev), to_cl(dy).to(dev)
    db0 = train_ops.colsum(dyc).cpu()
    out0, dbw0 = torch.full((cout, cin, k, k), float("nan"), device=dev), torch.full((cout,), float("nan"), device=dev)
    train_ops.conv_wgrad(xc, dyc, n, res, res, res, res, k, k, out=out0, dbias=dbw0)
    xv, cx = window(xc, ld_extra={"ldx_mod4": 1}.get(lay, 4), col_off={"x_plus1": 1}.get(lay, 0))
    sd = {"lddy_mod4": (1, 0), "dy_plus1": (4, 1)}.get(lay, (12, 4))
    dv, cd = window(dyc, ld_extra=sd[0], col_off=sd[1])
    # colsum has a scalar form: every layout is supported
    assert (aligned16(dv) and dv.stride(0) % 4 == 0) == (lay not in ("lddy_mod4", "dy_plus1")), "colsum4_kernel / colsum_kernel: the case is not on the side it names"
    db = train_ops.colsum(dv).cpu()
    cd("colsum")
    no_nan(db, "colsum")
    sc = float(ref_db.abs().max())
    assert_close(db / sc, ref_db / sc, 2e-4, "bias grad %s" % lay)         # (test_train_ops.py's bar)
    if lay == "wide":
        assert torch.equal(db, db0), "colsum: same walk, other addresses"
    out, dbw = torch.full((cout, cin, k, k), float("nan"), device=dev), torch.full((cout,), float("nan"), device=dev)
    c0 = 4
    call = lambda: (train_ops.conv_wgrad(xv[:, :c0], dv, n, res, res, res, res, k, k, out=out, ci_off=0, dbias=dbw),
                    train_ops.conv_wgrad(xv[:, c0:], dv, n, res, res, res, res, k, k, out=out, ci_off=c0))
    if lay != "wide":
        _refused("lfdm_conv2d_wgrad_cl_f32 failed.*wgrad", call, [("x", cx), ("dy", cd)], [out, dbw])
        return
    call()
    cx("wgrad x"), cd("wgrad dy")
    no_nan(out, "wgrad")
    assert_close(out.cpu() / scale, wt.grad / scale, 2e-4, "conv wgrad, two channel slices of a window")
    assert_close(dbw.cpu() / sc, ref_db / sc, 2e-4, "bias grad from the wgrad pass")


# ------------------------------------------------------------------------------------------ coverage of the header's leading dimensions
LD_NAMES = {"ld0", "ld1", "ldo", "ldr", "ss_ld", "dss_ld", "ldx", "ldy", "ldw", "lddy", "lddx", "ldadd", "ldh", "ld_src", "ld_out", "ld_prev", "ld",
            "stride_a", "stride_b", "batch_stride", "ld_o"}
RESERVED_FIELDS = {"gn_in_ss_ld"}          # "RESERVED, must be NULL / 0" (lfdm_conv_params): not an operand


def _header_entry_points_with_a_leading_dimension():
    with open(os.path.join(REPO, "include", "lfdm_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    ident = lambda body: set(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", body))
    structs = {m.group(2): ident(m.group(1)) for m in re.finditer(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S)}
    ld_structs = {name for name, fields in structs.items() if (fields & LD_NAMES) - RESERVED_FIELDS}
    owners = set()
    for m in re.finditer(r"\b(?:int|size_t)\s+(lfdm_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        name, params = m.group(1), ident(m.group(2))
        if "lfdm_stream_t" not in params:          # queries (plan, schedule, *_bytes) enqueue nothing
            continue
        if (params & LD_NAMES) or (params & ld_structs):
            owners.add(name)
    return owners


def test_layout_case_table_covers_the_header():
    """Every entry point of include/lfdm_hip.h that takes a leading dimension (as a parameter or through its parameter struct) has a case in
    this module's table.  There is no exemption list: the package calls every one of them."""
    owners = _header_entry_points_with_a_leading_dimension()
    assert len(owners) >= 40, sorted(owners)
    covered = {c.entry for c in CASE_TABLE}
    import sys
    tests_here = {n for n in dir(sys.modules[__name__]) if n.startswith("test_")}
    assert all(c.test in tests_here and c.expect and c.operands for c in CASE_TABLE)
    missing = owners - covered
    assert not missing, "entry points with a leading dimension and no layout case: %s" % sorted(missing)
    # (cases without a leading dimension of their own: aliasing, alignment and which-kernel-ran cases)
    stale = covered - owners - {"lfdm_cfg_combine_f32", "lfdm_layernorm_cl_f32", "lfdm_sum_leading_f32", "lfdm_layernorm_bwd_add_cl_f32", "lfdm_multi_linear_f32",
                                "lfdm_multi_linear_bwd_f32", "lfdm_adam_step_f32", "lfdm_adam_guarded_step_f32", "lfdm_grad_sumsq_f32", "lfdm_optim_plan_f32"}
    assert not stale, "not (or no longer) entry points with a leading dimension: %s" % sorted(stale)


# ------------------------------------------------------------------------------------------ LFAE predictor tails (ldh)
@covers("lfdm_lfae_region_stats_f32", "L1+L3", dict(logits=[(12, 4), (1, 0), (4, 1)]), "one scalar kernel")
@covers("lfdm_lfae_motion_combine_f32", "L1+L3", dict(heads=[(12, 4), (1, 0), (4, 1)]), "one scalar kernel")
@pytest.mark.parametrize("spec", [(12, 4), (1, 0), (4, 1)], ids=["wide", "ldh_mod4", "plus1"])
def test_lfae_predictor_tails_layouts(backend, spec):
    """The region predictor's and the pixelwise flow predictor's tails read K (+2) columns of the head convolutions' wider channels-last rows."""
    dev = backend
    n, k, h, w, temp = 2, 5, 6, 8, 0.1
    logits = rnd(n * h * w, k, seed=1)
    lg = logits.double().view(n, h * w, k).permute(0, 2, 1) / temp
    heat = lg.softmax(dim=-1).view(n, k, h, w)
    gx = (2 * (torch.arange(w, dtype=torch.float64) / (w - 1)) - 1).view(1, 1, 1, w)
    gy = (2 * (torch.arange(h, dtype=torch.float64) / (h - 1)) - 1).view(1, 1, h, 1)
    shift = torch.stack(((heat * gx).sum(dim=(2, 3)), (heat * gy).sum(dim=(2, 3))), dim=-1)
    base = ops.lfae_region_stats(logits.to(dev), n, k, h, w, temp)
    assert_close(base["heatmap"].cpu(), heat.float(), TOL, "region heatmap")
    assert_close(base["shift"].cpu(), shift.float(), TOL, "region shift")
    lv, cl = window(logits.to(dev), ld_extra=spec[0], col_off=spec[1])
    got = ops.lfae_region_stats(lv, n, k, h, w, temp)
    cl("region_stats logits")
    for key in base:
        no_nan(got[key], "region_stats " + key)
        assert torch.equal(got[key].cpu(), base[key].cpu()), "region_stats %s: window against the contiguous call" % key
    heads, sparse = rnd(n * h * w, k + 2, seed=2), rnd(n, k + 1, h, w, 2, seed=3)
    m = heads[:, :k + 1].double().view(n, h, w, k + 1).softmax(dim=-1)
    flow = (m.permute(0, 3, 1, 2).unsqueeze(-1) * sparse.double()).sum(dim=1)
    occ = torch.sigmoid(heads[:, k + 1].double()).view(n, 1, h, w)
    f0, o0 = ops.lfae_motion_combine(heads.to(dev), sparse.to(dev), True)
    assert_close(f0.cpu(), flow.float(), TOL, "motion combine flow")
    assert_close(o0.cpu(), occ.float(), TOL, "motion combine occlusion")
    hv, ch = window(heads.to(dev), ld_extra=spec[0], col_off=spec[1])
    f1, o1 = ops.lfae_motion_combine(hv, sparse.to(dev), True)
    ch("motion_combine heads")
    no_nan(f1, "motion_combine"), no_nan(o1, "motion_combine")
    assert torch.equal(f1.cpu(), f0.cpu()) and torch.equal(o1.cpu(), o0.cpu()), "motion_combine: window against the contiguous call"


@covers("lfdm_im2col_cl_f32", "L1+refusal", dict(x=[(4, 0), (12, 4), (1, 0), (4, 1)]), "one float4 kernel; ldx % 4, x & 15 refused")
@pytest.mark.parametrize("spec", [(4, 0), (12, 4), (1, 0), (4, 1)], ids=["wide", "wide_off", "ldx_mod4", "x_plus1"])
def test_im2col_layouts(backend, spec):
    from cvpr23_lfdm_amd import train_ops
    dev = backend
    n, c, h, w, k, pad = 2, 8, 5, 6, 3, 1
    x = rnd(n, c, h, w, seed=1)
    cols = F.unfold(x, k, padding=pad).view(n, c, k * k, h * w).permute(0, 3, 2, 1).reshape(n * h * w, k * k * c)      # column tap * c + ch
    base = train_ops.im2col_cl(to_cl(x).to(dev), n, h, w, k, pad).cpu()
    assert torch.equal(base, cols), "im2col is a copy"
    xv, cx = window(to_cl(x).to(dev), ld_extra=spec[0], col_off=spec[1])
    if spec in ((1, 0), (4, 1)):
        _refused("lfdm_im2col_cl_f32 failed.*im2col_cl", lambda: train_ops.im2col_cl(xv, n, h, w, k, pad), [("x", cx)])
        return
    got = train_ops.im2col_cl(xv, n, h, w, k, pad).cpu()
    cx("im2col x")
    assert torch.equal(got, cols)


# ------------------------------------------------------------------------------------------ BatchNorm (training) on channel slices
@covers("lfdm_batchnorm_train_fwd_cl_f32", "L1+refusal", dict(x=[(12, 4), (1, 0), (4, 1)]), "one kernel chain; ldx % 4, x & 15 refused")
@covers("lfdm_batchnorm_train_bwd_cl_f32", "L1+refusal", dict(x=[(12, 4), (1, 0), (4, 1)], dy=[(4, 0), (1, 0), (4, 1)], dx_add=[(4, 4), (1, 0), (4, 1)]),
        "one kernel chain; ld % 4 / 16-byte refusals")
@pytest.mark.parametrize("lay", ["wide", "ldx_mod4", "x_plus1", "lddy_mod4", "dy_plus1", "ldadd_mod4", "add_plus1"])
def test_batchnorm_train_layouts(backend, lay):
    """The LFAE BatchNorm reads its input, the gradient and the skip path's gradient where they lie - the channel halves of a torch.cat
    (row stride > C): against torch's batch_norm autograd, and bit-identical to the dense call."""
    from cvpr23_lfdm_amd import lfae_ops as L
    dev = backend
    n, c, h, w = 3, 16, 6, 5
    x = (rnd(n, c, h, w, seed=1) * 1.7 + 0.3).requires_grad_(True)
    g, b = (rnd(c, seed=2) * 0.3 + 1.0).requires_grad_(True), (rnd(c, seed=3) * 0.2).requires_grad_(True)
    dy, add = rnd(n, c, h, w, seed=6), rnd(n, c, h, w, seed=7)
    y = F.relu(F.batch_norm(x, None, None, g, b, True, 0.1, 1e-5))
    y.backward(dy)
    gd, bd = g.detach().to(dev), b.detach().to(dev)

    def run(xr, dyr, addr):
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        yk, stat = L.batchnorm_train_fwd(xr, gd, bd, rm, rv, 0.1, 1e-5, True)
        dg, db = torch.full((c,), float("nan"), device=dev), torch.full((c,), float("nan"), device=dev)
        dx = L.batchnorm_train_bwd(xr, dyr, gd, bd, stat, True, dgamma=dg, dbeta=db, dx_add=addr)
        return [t.cpu() for t in (yk, dx, dg, db)]

    base = run(to_cl(x.detach()).to(dev), to_cl(dy).to(dev), to_cl(add).to(dev))
    assert_close(from_cl(base[0], n, h, w), y.detach(), TOL, "bn y")
    sc = float(x.grad.abs().max())
    assert_close((from_cl(base[1], n, h, w) - add) / sc, x.grad / sc, 2e-4, "bn dx (+ dx_add)")
    assert_close(base[2] / float(g.grad.abs().max()), g.grad / float(g.grad.abs().max()), 2e-4, "bn dgamma")
    assert_close(base[3] / float(b.grad.abs().max()), b.grad / float(b.grad.abs().max()), 2e-4, "bn dbeta")
    sx = {"ldx_mod4": (1, 0), "x_plus1": (4, 1)}.get(lay, (12, 4))
    sd = {"lddy_mod4": (1, 0), "dy_plus1": (4, 1)}.get(lay, (4, 0))
    sa = {"ldadd_mod4": (1, 0), "add_plus1": (4, 1)}.get(lay, (4, 4))
    xv, cx = window(to_cl(x.detach()).to(dev), ld_extra=sx[0], col_off=sx[1])
    dv, cd = window(to_cl(dy).to(dev), ld_extra=sd[0], col_off=sd[1])
    av, ca = window(to_cl(add).to(dev), ld_extra=sa[0], col_off=sa[1])
    checks = [("x", cx), ("dy", cd), ("dx_add", ca)]
    if lay != "wide":
        _refused("lfdm_batchnorm_train_(fwd|bwd)_cl_f32 failed.*batchnorm_train", lambda: run(xv, dv, av), checks)
        return
    got = run(xv, dv, av)
    for what, chk in checks:
        chk("batchnorm, operand %s" % what)
    for a_, b_, what in zip(got, base, ("y", "dx", "dgamma", "dbeta")):
        no_nan(a_, "batchnorm " + what)
        assert torch.equal(a_, b_), "batchnorm %s: windows against the dense call" % what
    assert int(L._state(torch.device(dev) if dev == "cpu" else xv.device)["tickets"].abs().max()) == 0


# ------------------------------------------------------------------------------------------ convolution: the forms outside CONV_CASES
def _conv_special_form_in_place(dev, form):
    """out = residual's window for the deconv4 (with and without split-K), grouped and bf16-operand launches: bit-identical to the same launch
    with a separate contiguous output; pool2 with a residual is refused."""
    n, c, h, w = 2, 32, 4, 4
    x = rnd(n, c, h, w, seed=1)
    bias = rnd(64, seed=3).to(dev)
    if form.startswith("deconv4"):
        cout, ho, wo = c, 2 * h, 2 * w
        wt = rnd(c, cout, 4, 4, seed=2, scale=1.0 / math.sqrt(c * 4))
        conv = F.conv_transpose2d(x.double(), wt.double(), bias[:cout].cpu().double(), stride=2, padding=1)
        w4 = ops.pack_deconv4_weight(wt).to(dev)
        run = lambda src, res, out: ops.conv2d_cl(src, w4[0], cout, 2, 2, n, h, w, bias=bias[:cout], pad=(1, 1), hq=h, wq=w, ho=ho, wo=wo, out_scale=2, deconv4=w4,
                                                  ksplit=3 if form == "deconv4_splitk" else 1, residual=res, out=out)
    elif form == "grouped":
        g, og = 2, 32
        cout, ho, wo = g * og, h, w
        wt = rnd(cout, c // g, 3, 3, seed=2, scale=1.0 / math.sqrt(c // g * 9))
        conv = F.conv2d(x.double(), wt.double(), bias.cpu().double(), padding=1, groups=g)
        ww = ops.pack_wino_weight_grouped([wt[i * og:(i + 1) * og].to(dev) for i in range(g)])
        run = lambda src, res, out: ops.conv2d_cl(src, ww, cout, 3, 3, n, h, w, bias=bias, weight_wino=ww, groups=g, residual=res, out=out)
    else:
        cout, ho, wo = 64, h, w
        wt = rnd(cout, c, 3, 3, seed=2, scale=1.0 / math.sqrt(c * 9))
        conv = None if form == "bf16" else F.conv2d(x.double(), wt.double(), bias.cpu().double(), padding=1)
        wd, ww = ops.pack_conv_weight(wt).to(dev), ops.pack_wino_weight(wt.to(dev))
        if form == "pool2":
            res = torch.zeros(n * (h // 2) * (w // 2), cout, device=dev)
            with pytest.raises(RuntimeError, match="pool2"):
                ops.conv2d_cl(to_cl(x).to(dev), wd, cout, 3, 3, n, h, w, bias=bias, act=1, weight_wino=ww, pool2=True, residual=res, out=res)
            assert float(res.abs().max()) == 0.0
            return
        wb = ops.pack_wino_weight_bf16(wt.to(dev))
        run = lambda src, res, out: ops.conv2d_cl(src, wd, cout, 3, 3, n, h, w, bias=bias, weight_wino=ww, weight_wino_bf16=wb, residual=res, out=out)
    rows = n * ho * wo
    res = rnd(rows, cout, seed=4)
    base = run(to_cl(x).to(dev), res.to(dev), torch.full((rows, cout), float("nan"), device=dev)).cpu()
    if conv is not None:
        assert_close(from_cl(base, n, ho, wo), (conv + from_cl(res, n, ho, wo).double()).float(), TOL, "%s + residual, contiguous" % form)
    sv, cs = window(to_cl(x).to(dev), ld_extra=4, col_off=0)
    rv, cr = window(res.to(dev), ld_extra=12, col_off=4)
    got = run(sv, rv, rv).cpu().contiguous()
    cs("%s in place, src0" % form), cr("%s in place, out = residual" % form)
    no_nan(got, form)
    assert torch.equal(got, base), "%s: out aliasing the residual against a separate output" % form


@covers("lfdm_conv2d_cl_f32", "L1+L2+L3", dict(src0=(4, 0), out=[(12, 4), (1, 0), "residual's view"]), "deconv4 / grouped / pool2 / bf16 operands: same plan as contiguous; grouped, pool2 and bf16 refused off the Winograd schedule")
@covers("lfdm_conv2d_cl_wino_bf16", "L1+refusal", dict(src0=(4, 0), out=[(12, 4), (1, 0)]), "schedule 2 on bf16 operands; refused where the plan leaves schedule 2")
@pytest.mark.parametrize("ragged", [False, True, "alias"], ids=["wide", "ldo_mod4", "alias"])
@pytest.mark.parametrize("form", ["deconv4", "deconv4_splitk", "grouped", "pool2", "bf16"])
def test_conv_special_forms_layouts(backend, form, ragged, monkeypatch):
    """ConvTranspose as one launch (deconv4, with and without split-K), the grouped and the pooled Winograd launches and the bf16-operand
    launch, in windows: bit-identical to the contiguous call.  With an output row stride that is no multiple of 4 the deconvolution retreats
    to the scalar epilogue / reduce pass; the three Winograd-only forms are refused and write nothing."""
    dev = backend
    monkeypatch.setenv("LFDM_WINO", "1")
    if ragged == "alias":          # L2: out is the residual's window (pool2 takes no residual: lfdm_hip.h)
        _conv_special_form_in_place(dev, form)
        return
    n, c, h, w = 2, 32, 4, 4
    x = rnd(n, c, h, w, seed=1)
    bias = rnd(64, seed=3)
    spec_o = (1, 0) if ragged else (12, 4)
    if form.startswith("deconv4"):
        cout, ho, wo = c, 2 * h, 2 * w
        wt = rnd(c, cout, 4, 4, seed=2, scale=1.0 / math.sqrt(c * 4))
        ref = F.conv_transpose2d(x.double(), wt.double(), bias[:cout].double(), stride=2, padding=1).float()
        w4 = ops.pack_deconv4_weight(wt).to(dev)
        run = lambda src, out: ops.conv2d_cl(src, w4[0], cout, 2, 2, n, h, w, bias=bias[:cout].to(dev), pad=(1, 1), hq=h, wq=w, ho=ho, wo=wo, out_scale=2,
                                             deconv4=w4, ksplit=3 if form == "deconv4_splitk" else 1, out=out)
    elif form == "grouped":
        g, og = 2, 32
        cout, ho, wo = g * og, h, w
        wt = rnd(cout, c // g, 3, 3, seed=2, scale=1.0 / math.sqrt(c // g * 9))
        ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1, groups=g).float()
        ww = ops.pack_wino_weight_grouped([wt[i * og:(i + 1) * og].to(dev) for i in range(g)])
        run = lambda src, out: ops.conv2d_cl(src, ww, cout, 3, 3, n, h, w, bias=bias.to(dev), weight_wino=ww, groups=g, out=out)
    else:
        cout = 64
        wt = rnd(cout, c, 3, 3, seed=2, scale=1.0 / math.sqrt(c * 9))
        conv = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
        wd, ww = ops.pack_conv_weight(wt).to(dev), ops.pack_wino_weight(wt.to(dev))
        if form == "pool2":
            ho, wo = h // 2, w // 2
            ref = F.avg_pool2d(F.relu(conv), 2).float()
            run = lambda src, out: ops.conv2d_cl(src, wd, cout, 3, 3, n, h, w, bias=bias.to(dev), act=1, weight_wino=ww, pool2=True, out=out)
        else:
            ho, wo, ref = h, w, None          # (the bf16 form's own accuracy bar lives in tests/test_conv_wino_bf16.py; here: same plan, same bits)
            wb = ops.pack_wino_weight_bf16(wt.to(dev))
            run = lambda src, out: ops.conv2d_cl(src, wd, cout, 3, 3, n, h, w, bias=bias.to(dev), weight_wino=ww, weight_wino_bf16=wb, out=out)
    rows = n * ho * wo
    base = run(to_cl(x).to(dev), torch.full((rows, cout), float("nan"), device=dev)).cpu()
    if ref is not None:
        assert_close(from_cl(base, n, ho, wo), ref, TOL, "%s, contiguous" % form)
    sv, cs = window(to_cl(x).to(dev), ld_extra=4, col_off=0)
    ov, co = window((rows, cout), ld_extra=spec_o[0], col_off=spec_o[1], device=dev)
    checks = [("src0", cs), ("out", co)]
    if ragged and not form.startswith("deconv4"):
        with pytest.raises(RuntimeError):          # (ops.WinogradUnavailable or the library's refusal: both are RuntimeError)
            run(sv, ov)
        for what, chk in checks:
            chk("%s refused, operand %s" % (form, what))
        assert bool(torch.isnan(ov).all())
        return
    got = run(sv, ov).cpu().contiguous()
    for what, chk in checks:
        chk("%s, operand %s" % (form, what))
    no_nan(got, form)
    if ragged:
        assert_close(from_cl(got, n, ho, wo), ref, TOL, "%s, ldo %% 4 != 0" % form)
    else:
        assert torch.equal(got, base), "%s: windows against the contiguous call" % form


@covers("lfdm_conv2d_cl_f32", "refusal", dict(residual=[(1, 0), (4, 1)], bias="+1 float", out=[(1, 0), (4, 1)]), "ln_wsum exists in the float4 epilogue only: refused")
@pytest.mark.parametrize("pw", ["0", "2"], ids=["staged", "pointwise"])
@pytest.mark.parametrize("lay", ["wide", "alias", "ldr_mod4", "res_plus1", "bias_plus1", "ldo_mod4", "out_plus1"])
def test_conv_fused_layernorm_layouts(backend, lay, pw, monkeypatch):
    """The LayerNorm fold (lfdm_conv_params.ln_wsum) is finished in the float4 epilogue; the scalar epilogue has no such step.  A residual,
    bias or output that would send the launch there is refused (before, residual / bias were not checked and the result silently lacked the
    normalisation)."""
    import lfdm_oracle as O
    dev = backend
    monkeypatch.setenv("LFDM_PW", pw)          # 0: the LDS-staged schedule; 2: the pointwise schedule (3) wherever it is eligible
    b, t, s, c, cout = 2, 2, 4, 64, 96
    x = rnd(b, c, t, s, s, seed=1) * 2 + 0.7
    gamma = rnd(1, c, 1, 1, 1, seed=2) * 0.3 + 1
    wt, bias = rnd(cout, c, seed=3, scale=1.0 / math.sqrt(c)), rnd(cout, seed=4)
    res = rnd(b * t * s * s, cout, seed=5)
    ref = unet_to_cl(torch.einsum("oc,bcthw->bothw", wt.double(), O.channel_layernorm(x.double(), gamma.double()))) + bias.double() + res.double()
    packed, wsum = ops.pack_ln_conv_weight(wt, gamma.reshape(-1))
    sr = {"ldr_mod4": (1, 0), "res_plus1": (4, 1)}.get(lay, (4, 4))
    so = {"ldo_mod4": (1, 0), "out_plus1": (4, 1)}.get(lay, (12, 4))
    xv, cx = window(unet_to_cl(x).to(dev), ld_extra=4, col_off=0)
    rv, cr = window(res.to(dev), ld_extra=sr[0], col_off=sr[1])
    ov, co = window((b * t * s * s, cout), ld_extra=so[0], col_off=so[1], device=dev)
    bv, cb = window(bias.view(1, -1).to(dev), ld_extra=4, col_off=1 if lay == "bias_plus1" else 0)
    checks = [("x", cx), ("residual", cr), ("out", co), ("bias", cb)]
    if lay == "alias":          # L2: out is the residual's window
        ov = rv
    kw = dict(ln_wsum=wsum.to(dev), residual=rv, bias=bv[0], out=ov)
    pp, _ = ops.conv_params(xv, packed.to(dev), cout, 1, 1, b * t, s, s, **kw)
    sched = ops.conv_schedule(pp)
    call = lambda: ops.conv2d_cl(xv, packed.to(dev), cout, 1, 1, b * t, s, s, **kw)
    if lay not in ("wide", "alias"):
        assert sched != 3, "the pointwise schedule was kept for %s" % lay
        _refused("lfdm_conv2d_cl_f32 failed.*fused LayerNorm", call, checks, [ov])
        return
    assert (sched == 3) == (pw == "2"), "schedule %d with LFDM_PW=%s" % (sched, pw)
    r0 = res.to(dev).clone()
    got0 = ops.conv2d_cl(unet_to_cl(x).to(dev), packed.to(dev), cout, 1, 1, b * t, s, s, ln_wsum=wsum.to(dev), residual=r0, bias=bias.to(dev)).cpu()
    got = call().cpu()
    assert torch.equal(got, got0), "LayerNorm fold, schedule %d: windows against the contiguous call" % sched
    for what, chk in checks:
        chk("fused LayerNorm conv, operand %s" % what)
    no_nan(got, "fused LayerNorm conv")
    assert_close(got, ref.float(), TOL, "fused layernorm + 1x1 conv + bias + residual in windows")


# ------------------------------------------------------------------------------------------ weight packers (ld_o) and GroupNorm backward (ss_ld)
@covers("lfdm_pack_wino_weight_f32", "L1", dict(w="input-channel slice [:, 16:48] of a (Cout, 64 + 2, 3, 3) NaN-filled filter"), "one kernel (also dgrad)")
@covers("lfdm_pack_wino4_weight_f32", "L1", dict(w="input-channel slice"), "one kernel")
@covers("lfdm_pack_wino_weight_bf16", "L1", dict(w="input-channel slice"), "one kernel")
@covers("lfdm_pack_wino_weights_multi_f32", "L1", dict(w="input-channel slice"), "one kernel, per-job ld_o")
def test_weight_packers_read_a_channel_slice_only(backend):
    """The Winograd packers take an input-channel slice of a wider filter as pointer + ld_o (a convolution over cat(x0, x1) packs its two halves
    separately): everything of the filter outside the slice is NaN, the packs equal those of the slice's contiguous copy bit for bit."""
    dev = backend
    cout, lo, hi, tot = 32, 16, 48, 66
    w = rnd(cout, hi - lo, 3, 3, seed=1, scale=0.2)
    full, chk = window(w.reshape(cout, -1).to(dev), ld_extra=(tot - (hi - lo)) * 9, col_off=lo * 9)
    wv = full.as_strided((cout, hi - lo, 3, 3), (tot * 9, 9, 3, 1), full.storage_offset())
    wc = w.to(dev)
    for what, fn in (("wino", ops.pack_wino_weight), ("wino dgrad", lambda t: ops.pack_wino_weight(t, dgrad=True)), ("wino4", ops.pack_wino4_weight),
                     ("wino bf16", ops.pack_wino_weight_bf16)):
        a, b_ = fn(wv), fn(wc)
        no_nan(a.float(), what)
        assert torch.equal(a, b_), "pack %s: slice of a wider filter against its contiguous copy" % what
    o1, o2 = torch.full_like(ops.pack_wino_weight(wc), float("nan")), torch.full_like(ops.pack_wino_weight(wc, dgrad=True), float("nan"))
    ops.pack_wino_weights_multi([(wv, o1, False), (wv, o2, True)])
    assert torch.equal(o1, ops.pack_wino_weight(wc)) and torch.equal(o2, ops.pack_wino_weight(wc, dgrad=True))
    chk("weight packers")


@covers("lfdm_groupnorm_silu_bwd_cl_f32", "L1+L3", dict(scale_shift=[(12, 4), (5, 1)]), "one kernel chain; scale_shift read by scalar loads (dss_ld = 2C from the wrapper)")
@pytest.mark.parametrize("spec", [(12, 4), (5, 1)], ids=["wide", "ragged"])
def test_groupnorm_bwd_scale_shift_window(backend, spec):
    from cvpr23_lfdm_amd import train_ops
    dev = backend
    b, t, s, c = 2, 3, 4, 32
    x = rnd(b, c, t, s, s, seed=1).requires_grad_(True)
    gamma, beta = (1 + 0.2 * rnd(c, seed=2)).requires_grad_(True), (0.1 * rnd(c, seed=3)).requires_grad_(True)
    ss = (0.3 * rnd(b, 2 * c, seed=4)).requires_grad_(True)
    y = F.silu(F.group_norm(x, 8, gamma, beta, eps=1e-5) * (ss[:, :c].view(b, c, 1, 1, 1) + 1) + ss[:, c:].view(b, c, 1, 1, 1))
    dy = rnd(*y.shape, seed=5)
    y.backward(dy)
    rows = lambda v: unet_to_cl(v.detach()).to(dev)
    gd, bd = gamma.detach().to(dev), beta.detach().to(dev)

    def run(ssv):
        yk, partial, nchunk = train_ops.groupnorm_silu_train(rows(x), b, gd, bd, scale_shift=ssv)
        return [yk.cpu()] + [v.cpu() for v in train_ops.groupnorm_silu_bwd(rows(x), rows(dy), b, gd, bd, partial, nchunk, scale_shift=ssv)]

    base = run(ss.detach().to(dev))
    for got, want, what in zip(base[1:], (unet_to_cl(x.grad), gamma.grad, beta.grad, ss.grad), ("dx", "dgamma", "dbeta", "dscale_shift")):
        sc = max(1.0, float(want.abs().max())) if what == "dx" else float(want.abs().max())
        assert_close(got / sc, want / sc, 2e-4, "gn " + what)
    ssv, chk = window(ss.detach().to(dev), ld_extra=spec[0], col_off=spec[1])
    got = run(ssv)
    chk("groupnorm backward scale_shift")
    for a, b_, what in zip(got, base, ("y", "dx", "dgamma", "dbeta", "dscale_shift")):
        no_nan(a, "gn bwd " + what)
        assert torch.equal(a, b_), "groupnorm backward %s: scale_shift window against the dense table" % what


# ------------------------------------------------------------------------------------------ batch-strided grids (flow colours, flow metrics)
@covers("lfdm_flow_color_u8", "L1", dict(grid="first two channels of a NaN-padded (B, 3, T, s, s) latent, batch window (12, 4)"), "one kernel")
@covers("lfdm_flow_metrics", "L1", dict(grid_a="batch window (12, 4)", grid_b="batch window (4, 0) of a 3-channel latent"), "one kernel, stride_a != stride_b")
def test_flow_grids_batch_strides(backend):
    """The grid is read in place from the latent (B, 3, T, s, s): its third channel and the padding between batch items are NaN here.
    Two different batch strides in one flow_metrics call; results bit-identical to the contiguous calls, and against their definitions."""
    dev = backend
    b, t, s = 2, 3, 8
    ga, gb = rnd(b, 2, t, s, s, seed=1) * 0.4, rnd(b, 2, t, s, s, seed=2) * 0.4
    item = 3 * t * s * s
    la, ca = window((b, item), ld_extra=12, col_off=4, device=dev)          # whole latents left at the sentinel: the third channel is NaN
    lb, cb = window((b, item), ld_extra=4, col_off=0, device=dev)
    va = la.as_strided((b, 2, t, s, s), (la.stride(0), t * s * s, s * s, s, 1), la.storage_offset())
    vb = lb.as_strided((b, 2, t, s, s), (lb.stride(0), t * s * s, s * s, s, 1), lb.storage_offset())
    va.copy_(ga), vb.copy_(gb)
    assert va.stride(0) != vb.stride(0)
    col0 = ops.flow_to_color_u8(ga.to(dev))
    col = ops.flow_to_color_u8(va)
    assert torch.equal(col, col0)
    m0 = ops.flow_metrics(ga.to(dev), gb.to(dev)).cpu()
    m = ops.flow_metrics(va, vb).cpu()
    ca("flow grid a"), cb("flow grid b")
    no_nan(m, "flow_metrics")
    assert torch.equal(m, m0)
    epe = (ga.double() - gb.double()).pow(2).sum(dim=1).sqrt().mean(dim=(2, 3))
    assert_close(m[..., 0], epe, TOL, "flow end-point error")


@covers("lfdm_heads_gn_res_cl_to_planar_f32", "L1+refusal", dict(y=[(8, 4), (1, 0), (8, 1)], x0=[(4, 0), (1, 0), (4, 1)], x1=(12, 4)), "one kernel; ld % 4 / 16-byte refusals")
@pytest.mark.parametrize("lay", ["wide", "ld_mod4", "y_plus1", "ld0_mod4", "x0_plus1"])
def test_heads_with_groupnorm_layouts(backend, lay):
    dev = backend
    b, t, s, nchunk, ch, c0, c1, groups = 1, 2, 4, 1, 64, 64, 64, 16
    pixels = t * s * s
    y = rnd(b * pixels, 2 * ch, seed=1) * 1.7 + 0.4
    x0, x1 = rnd(b * pixels, c0, seed=2), rnd(b * pixels, c1, seed=3)
    gamma, beta = rnd(2 * ch, seed=4) * 0.3 + 1, rnd(2 * ch, seed=5) * 0.3
    wf, bf, wo, bo = rnd(2, ch, seed=7, scale=0.2), rnd(2, seed=8), rnd(1, ch, seed=9, scale=0.2), rnd(1, seed=10)
    we = rnd(3, c0 + c1, seed=11, scale=0.1)
    ys = y.double().view(b, pixels, 2 * ch)
    yn = F.silu(F.group_norm(ys.permute(0, 2, 1), groups, gamma.double(), beta.double(), eps=1e-5).permute(0, 2, 1)).reshape(b * pixels, 2 * ch)
    xe = torch.cat((x0, x1), dim=1).double()
    wfd, wod, wed = wf.double(), wo.double(), we.double()
    ref = torch.stack((yn[:, :ch] @ wfd[0] + bf[0] + xe @ wed[0], yn[:, :ch] @ wfd[1] + bf[1] + xe @ wed[1], yn[:, ch:] @ wod[0] + bo[0] + xe @ wed[2]), dim=1)
    ref = ref.view(b, t, s * s, 3).permute(0, 3, 1, 2).float()
    yg = ys.view(b, nchunk, pixels // nchunk, groups, 2 * ch // groups)
    partial = torch.stack([yg.sum(dim=(2, 4)), (yg * yg).sum(dim=(2, 4))], dim=-1).float().contiguous().view(b * nchunk, 2 * groups).to(dev)
    small = [v.to(dev) for v in (gamma, beta, wf, bf, wo, bo)]
    base = ops.heads_gn_res_cl_to_planar(y.to(dev), partial, nchunk, *small, x0.to(dev), x1.to(dev), we.to(dev), b, t, s * s, groups=groups).cpu()
    assert_close(base, ref, TOL, "heads with the last GroupNorm folded in, contiguous")
    sy = {"ld_mod4": (1, 0), "y_plus1": (8, 1)}.get(lay, (8, 4))
    s0 = {"ld0_mod4": (1, 0), "x0_plus1": (4, 1)}.get(lay, (4, 0))
    yv, cy = window(y.to(dev), ld_extra=sy[0], col_off=sy[1])
    x0v, k0 = window(x0.to(dev), ld_extra=s0[0], col_off=s0[1])
    x1v, k1 = window(x1.to(dev), ld_extra=12, col_off=4)
    checks = [("y", cy), ("x0", k0), ("x1", k1)]
    out = torch.full((b, 3, t, s * s), float("nan"), device=dev)
    call = lambda: ops.heads_gn_res_cl_to_planar(yv, partial, nchunk, *small, x0v, x1v, we.to(dev), b, t, s * s, groups=groups, out=out)
    if lay != "wide":
        _refused("lfdm_heads_gn_res_cl_to_planar_f32 failed.*heads_gn_res", call, checks, [out])
        return
    got = call().cpu()
    for what, chk in checks:
        chk("heads_gn_res, operand %s" % what)
    no_nan(got, "heads_gn_res")
    assert torch.equal(got, base)


@covers("lfdm_absmax_f32", "L1+L3", dict(x=[(12, 4), (1, 0), (4, 1)]), "float4 walk (16 B, ld % 4, C % 4) / scalar walk")
@pytest.mark.parametrize("spec", [(12, 4), (1, 0), (4, 1)], ids=["wide", "ld_mod4", "plus1"])
def test_absmax_layouts(backend, spec):
    """max |x| over a window.  A NaN never wins the kernel's comparison, so the gaps hold FLT_MAX here instead: a gap read is the result."""
    dev = backend
    rows, c = 37, 8
    x = rnd(rows, c, seed=1) * 3
    xv, chk = window(x.to(dev), ld_extra=spec[0], col_off=spec[1], sentinel=0x7F7FFFFF)
    assert (aligned16(xv) and xv.stride(0) % 4 == 0) == (spec == (12, 4)), "the case is not on the side of the gate it names"
    lib = ops._lib()
    bits = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.check(lib.lfdm_absmax_f32(ops._p(xv), rows, c, xv.stride(0), ops._p(bits), ops._stream(lib)), "lfdm_absmax_f32")
    chk("absmax")
    assert float(bits.view(torch.float32).cpu()) == float(x.abs().max())


# ------------------------------------------------------------------------------------------ warp backward + fixed-point finalize
def _warp_bwd_run(dev, sr, pr, dr, m, n, h, w, c, dprev, dsrc):
    """lfdm_absmax_f32 + lfdm_warp_bwd_f32 (channels-last) + lfdm_fix_finalize_f32 exactly as lfae_ops.ApplyOpticalCL.backward chains them, on the
    given row operands: src (ld_src), prev (ld_prev), dout (ld_dout), dprev (ld_dprev) and the finalized dsrc (ld)."""
    from cvpr23_lfdm_amd import lfae_ops as L
    from cvpr23_lfdm_amd._native import WarpBwdParams
    lib = ops._lib()
    st = L._state(torch.device(dev))
    p = WarpBwdParams()
    L._warp_bwd_common(p, m, n, h, w, c)
    p.layout_cl, p.n_div = 1, 1
    p.src, p.ld_src, p.dout, p.ld_dout = sr.data_ptr(), sr.stride(0), dr.data_ptr(), dr.stride(0)
    p.prev, p.ld_prev, p.dprev, p.ld_dprev = pr.data_ptr(), pr.stride(0), dprev.data_ptr(), dprev.stride(0)
    dmaps = torch.full((n, 3, h, w), float("nan"), device=dev)
    p.dmaps = dmaps.data_ptr()
    acc = L._fix_acc(torch.device(dev), n * h * w * c)
    p.dsrc_fix, p.amax_bits = acc.data_ptr(), st["amax"].data_ptr()
    lib.check(lib.lfdm_absmax_f32(ops._p(dr), n * h * w, c, dr.stride(0), ops._p(st["amax"]), ops._stream(lib)), "lfdm_absmax_f32")
    try:
        lib.check(lib.lfdm_warp_bwd_f32(ctypes.byref(p), ops._stream(lib)), "lfdm_warp_bwd_f32")
    except RuntimeError:
        st["amax"].zero_()          # (the refused launch leaves the max word of the absmax pass: hand the state back as the finalize would)
        raise
    lib.check(lib.lfdm_fix_finalize_f32(ops._p(acc), ops._p(dsrc), n * h * w, c, dsrc.stride(0), ops._p(st["amax"]), 4 * h * w,
                                        ctypes.c_void_p(st["amax"].data_ptr() + 4), ops._stream(lib)), "lfdm_fix_finalize_f32")
    assert int(st["fix"].abs().max()) == 0 and int(st["amax"].abs().max()) == 0, "the scatter workspace was not handed back zeroed"
    return dmaps


@covers("lfdm_warp_bwd_f32", "L1+refusal", dict(src=[(4, 0), (1, 0), (4, 1)], prev=[(12, 4), (1, 0), (4, 1)], dout=[(4, 4), (1, 0), (4, 1)],
                                                  dprev=[(12, 0), (1, 0), (4, 1)]), "warp_bwd_cl_kernel; ld % 4 / 16-byte refusals per operand")
@covers("lfdm_fix_finalize_f32", "L1+L3", dict(out=[(4, 4), (1, 0), (4, 1)]), "one scalar kernel")
@pytest.mark.parametrize("lay", ["wide", "dsrc_ld_mod4", "dsrc_plus1", "ld_src_mod4", "src_plus1", "ld_prev_mod4", "prev_plus1", "ld_dout_mod4", "dout_plus1",
                                 "ld_dprev_mod4", "dprev_plus1"])
def test_warp_bwd_layouts(backend, lay):
    """Backward of Generator.apply_optical on channel slices: against torch autograd (test_lfae_ops.py's reference and bar) and bit-identical to
    the dense call (the scatter is a fixed-point sum: order-free)."""
    from test_lfae_ops import _apply_optical_ref, _flow
    dev = backend
    n, c, h, w, fh, fw = 2, 16, 8, 6, 4, 3
    src, prev = rnd(n, c, h, w, seed=1).requires_grad_(True), rnd(n, c, h, w, seed=2).requires_grad_(True)
    flow = _flow(n, fh, fw, 3, amp=0.6).requires_grad_(True)
    occ = torch.sigmoid(rnd(n, 1, fh, fw, seed=4)).requires_grad_(True)
    ref = _apply_optical_ref(src, prev, flow, occ)
    dy = rnd(*ref.shape, seed=5)
    ref.backward(dy)
    m = torch.cat((flow.detach().permute(0, 3, 1, 2), occ.detach()), dim=1).contiguous().to(dev)
    rows = n * h * w
    dense = lambda t: to_cl(t.detach()).to(dev)
    nan = lambda: torch.full((rows, c), float("nan"), device=dev)
    dprev0, dsrc0 = nan(), nan()
    dmaps0 = _warp_bwd_run(dev, dense(src), dense(prev), dense(dy), m, n, h, w, c, dprev0, dsrc0)
    for got, want, what in ((dsrc0, src.grad, "dsrc"), (dprev0, prev.grad, "dprev")):
        sc = float(want.abs().max())
        assert_close(from_cl(got.cpu(), n, h, w) / sc, want / sc, 2e-4, "apply_optical " + what)
    spec = lambda key, default: {"ld_%s_mod4" % key: (1, 0), "%s_plus1" % key: (4, 1)}.get(lay, default)
    sv, k_s = window(dense(src), ld_extra=spec("src", (4, 0))[0], col_off=spec("src", (4, 0))[1])
    pv, k_p = window(dense(prev), ld_extra=spec("prev", (12, 4))[0], col_off=spec("prev", (12, 4))[1])
    dv, k_d = window(dense(dy), ld_extra=spec("dout", (4, 4))[0], col_off=spec("dout", (4, 4))[1])
    qv, k_q = window((rows, c), ld_extra=spec("dprev", (12, 0))[0], col_off=spec("dprev", (12, 0))[1], device=dev)
    so = {"dsrc_ld_mod4": (1, 0), "dsrc_plus1": (4, 1)}.get(lay, (4, 4))
    ov, k_o = window((rows, c), ld_extra=so[0], col_off=so[1], device=dev)
    checks = [("src", k_s), ("prev", k_p), ("dout", k_d), ("dprev", k_q), ("dsrc", k_o)]
    call = lambda: _warp_bwd_run(dev, sv, pv, dv, m, n, h, w, c, qv, ov)
    if lay not in ("wide", "dsrc_ld_mod4", "dsrc_plus1"):
        _refused("lfdm_warp_bwd_f32 failed.*warp_bwd", call, checks, [qv, ov])
        return
    dmaps = call()
    for what, chk in checks:
        chk("warp_bwd %s, operand %s" % (lay, what))
    for got, want, what in ((ov, dsrc0, "dsrc"), (qv, dprev0, "dprev"), (dmaps, dmaps0, "dmaps")):
        no_nan(got, "warp_bwd " + what)
        assert torch.equal(got.cpu(), want.cpu()), "warp_bwd %s: windows against the dense call" % what


# ------------------------------------------------------------------------------------------ motion inputs (output rows of ld floats)
@covers("lfdm_lfae_motion_inputs_f32", "L1+refusal", dict(rows=[(4, 4), (1, 0), (4, 1)]),
        "one kernel; DELIBERATE: columns 4(K+1) ... ld-1 of every row are written as zero (the hourglass reads ld channels); ld % 4, rows & 15 refused")
@pytest.mark.parametrize("lay", ["wide", "ld_mod4", "rows_plus1"])
def test_lfae_motion_inputs_layouts(backend, lay):
    """The hourglass input rows: `ld` is the consumer's channel count, so the header's stated exception holds - the columns from 4 (K + 1) up to ld
    are zeroed, exactly those - and nothing before or after the row block is touched."""
    dev = backend
    b, frames, k, h, w = 1, 2, 3, 6, 8
    n, used = b * frames, 4 * (k + 1)
    img = rnd(b, 3, h, w, seed=1).abs().to(dev)
    drv = dict(shift=(rnd(n, k, 2, seed=2) * 0.4).to(dev))
    srcd = dict(shift=(rnd(b, k, 2, seed=3) * 0.4).to(dev))
    rows0, sparse0 = ops.lfae_motion_inputs(img, drv, srcd, None, frames, region_var=0.01, revert_axis_swap=False, use_covar=False, pad_to=4)
    assert rows0.shape == (n * h * w, used)
    ld = used + {"wide": 16, "ld_mod4": 1, "rows_plus1": 16}[lay]
    raw, chk = window((1, n * h * w * ld), ld_extra=8, col_off=1 if lay == "rows_plus1" else 4, device=dev)
    rv = raw[0].view(n * h * w, ld)
    sparse = torch.full((n, k + 1, h, w, 2), float("nan"), device=dev)
    lib = ops._lib()
    call = lambda: lib.check(lib.lfdm_lfae_motion_inputs_f32(ops._p(img), ops._p(drv["shift"]), None, None, ops._p(srcd["shift"]), None, None, None, 0.01, 0, b,
                                                             frames, k, h, w, ops._p(rv), ld, ops._p(sparse), ops._stream(lib)), "lfdm_lfae_motion_inputs_f32")
    if lay != "wide":
        _refused("lfdm_lfae_motion_inputs_f32 failed.*lfae_motion_inputs", call, [("rows", chk)], [rv, sparse])
        return
    call()
    chk("motion_inputs rows")
    assert torch.equal(rv[:, :used].cpu(), rows0.cpu()) and torch.equal(sparse.cpu(), sparse0.cpu())
    assert float(rv[:, used:].abs().max()) == 0.0, "the padding columns of a row are written as zero (lfdm_hip.h)"


# ------------------------------------------------------------------------------------------ sum_leading, colsum: which side of the gate ran
@covers("lfdm_sum_leading_f32", "L3", dict(out="n % 4 != 0; +1 float"), "sum_leading4_kernel (n % 4 == 0, 16 B) / sum_leading_kernel")
@pytest.mark.parametrize("n,plus1", [(12, False), (13, False), (12, True)], ids=["vec", "n_mod4", "out_plus1"])
def test_sum_leading_layouts(backend, n, plus1):
    """out[i] = sum_s in[s * n + i]: the float4 form (n % 4 == 0, both pointers 16 B) and the scalar form behind it."""
    from cvpr23_lfdm_amd import train_ops
    dev = backend
    s = 5
    x = rnd(s, n, seed=1)
    xv, cx = window(x.reshape(1, -1).to(dev), ld_extra=8, col_off=4)
    ov, co = window((1, n), ld_extra=8, col_off=1 if plus1 else 4, device=dev)
    vec = n % 4 == 0 and aligned16(xv) and aligned16(ov)
    assert vec == (n == 12 and not plus1), "the case is not on the side of the gate it names"
    got = train_ops.sum_leading(xv[0], s, n, out=ov[0]).cpu()
    cx("sum_leading in"), co("sum_leading out")
    no_nan(got, "sum_leading")
    assert_close(got, x.double().sum(dim=0).float(), 2e-4, "sum_leading")
    want = x[0].clone()
    for i in range(1, s):          # s in fixed order
        want += x[i]
    assert torch.equal(got, want), "sum_leading adds the s slabs in order"


# ------------------------------------------------------------------------------------------ backward norms: dense float4 rows
@covers("lfdm_groupnorm_silu_bwd_cl_f32", "refusal", dict(x="+1 float", dy="+1 float", dx="+1 float"), "refused: float4 rows")
@covers("lfdm_layernorm_bwd_add_cl_f32", "refusal", dict(x="+1 float", dy="+1 float", dx="+1 float", gamma="+1 float", dx_add="+1 float"), "refused: float4 rows")
@pytest.mark.parametrize("form,which", [("groupnorm_bwd", o) for o in ("x", "dy", "dx")] + [("layernorm_bwd", o) for o in ("x", "dy", "dx", "gamma", "dx_add")])
def test_backward_norms_refuse_rows_that_are_not_16_byte_aligned(backend, form, which):
    """lfdm_groupnorm_silu_bwd_cl_f32 and lfdm_layernorm_bwd(_add)_cl_f32 read x / dy (gamma, dx_add) and write dx as float4 in every kernel:
    one call per operand that starts one float into an aligned buffer - refused, nothing written."""
    dev = backend
    lib = ops._lib()
    rows, c, b = 32, 64, 2
    t = dict(x=rnd(rows, c, seed=1), dy=rnd(rows, c, seed=2), dx=torch.full((rows, c), float("nan")), gamma=rnd(c, seed=3) + 1, dx_add=rnd(rows, c, seed=4))
    d = {k_: v.to(dev) for k_, v in t.items()}
    d[which], chk = _plus1_table(t[which], dev)
    assert not aligned16(d[which])
    beta = rnd(c, seed=5).to(dev)
    if form == "layernorm_bwd":
        dgamma = torch.full((c,), float("nan"), device=dev)
        nbytes = lib.lfdm_layernorm_bwd_ws_bytes(rows, c)
        ws = torch.empty(nbytes // 4 + 4, device=dev)
        call = lambda: lib.check(lib.lfdm_layernorm_bwd_add_cl_f32(ops._p(d["x"]), ops._p(d["dy"]), ops._p(d["dx_add"]), ops._p(d["dx"]), rows, c, ops._p(d["gamma"]),
                                                                   1e-5, ops._p(dgamma), ops._p(ws), nbytes, ops._stream(lib)), "lfdm_layernorm_bwd_add_cl_f32")
        _refused("lfdm_layernorm_bwd_add_cl_f32 failed.*layernorm_bwd", call, [(which, chk)], [d["dx"], dgamma])
    else:
        partial = torch.zeros(b * 1, 16, device=dev)
        dgb = torch.full((2, c), float("nan"), device=dev)
        nbytes = lib.lfdm_groupnorm_bwd_ws_bytes(b, rows // b, c)
        ws = torch.empty(nbytes // 4 + 4, device=dev)
        call = lambda: lib.check(lib.lfdm_groupnorm_silu_bwd_cl_f32(ops._p(d["x"]), ops._p(d["dy"]), ops._p(d["dx"]), b, rows // b, c, 8, ops._p(d["gamma"]), ops._p(beta),
                                                                    None, 0, 1e-5, 1, ops._p(partial), 1, ops._p(dgb), None, 0, ops._p(ws), nbytes, ops._stream(lib)),
                                 "lfdm_groupnorm_silu_bwd_cl_f32")
        _refused("lfdm_groupnorm_silu_bwd_cl_f32 failed.*groupnorm_bwd", call, [(which, chk)], [d["dx"], dgb])


@covers("lfdm_layernorm_cl_f32", "L1", dict(rows=">= 4096: small kernel; < 4096: generic kernel"), "both sides of the row-count gate, 16 B")
@pytest.mark.parametrize("rows", [4096 + 7, 96], ids=["small_kernel", "generic_kernel"])
def test_layernorm_both_kernels_in_a_window(backend, rows):
    """lfdm_layernorm_cl_f32 at C = 64: from 4096 rows on the several-rows-per-wavefront kernel runs, below it the generic one.  Both with x and out as
    dense row blocks inside NaN-filled buffers (16-byte aligned: the only layout the entry point takes), a ragged last row group."""
    dev = backend
    c = 64
    x, gamma = rnd(rows, c, seed=1) * 2 + 0.3, rnd(c, seed=2) * 0.3 + 1
    xd = x.double()
    ref = ((xd - xd.mean(dim=1, keepdim=True)) / (xd.var(dim=1, unbiased=False, keepdim=True) + 1e-5).sqrt() * gamma.double()).float()
    xv, cx = window(x.reshape(1, -1).to(dev), ld_extra=8, col_off=4)
    ov, co = window((1, rows * c), ld_extra=8, col_off=4, device=dev)
    got = ops.layernorm_cl(xv[0].view(rows, c), gamma.to(dev), out=ov[0].view(rows, c)).cpu()
    cx("layernorm x"), co("layernorm out")
    no_nan(got, "layernorm")
    assert_close(got, ref, TOL, "layernorm, %d rows" % rows)


# ------------------------------------------------------------------------------------------ refusals: multi_linear, optimizer kernels
@covers("lfdm_multi_linear_f32", "refusal", dict(x="+1 float", w="+1 float", k="k % 4 != 0"), "refused")
@covers("lfdm_multi_linear_bwd_f32", "refusal", dict(x="+1 float", w="+1 float", dw="+1 float", k="k % 4 != 0"), "refused")
@pytest.mark.parametrize("bad", ["x_plus1", "w_plus1", "k_mod4", "dw_plus1"])
def test_multi_linear_refusals(backend, bad):
    """train_linear.hip: x, every weight and every dw are read / written as float4 (k % 4 == 0): one call per violated condition."""
    from cvpr23_lfdm_amd import train_ops
    dev = backend
    rows, k, n = 3, 6 if bad == "k_mod4" else 8, 5
    x, w = rnd(rows, k, seed=1), rnd(n, k, seed=2)
    xd, wd, checks = x.to(dev), w.to(dev), []
    if bad == "x_plus1":
        xd, chk = _plus1_table(x, dev)
        checks.append(("x", chk))
    if bad == "w_plus1":
        wd, chk = _plus1_table(w, dev)
        checks.append(("w", chk))
    if bad == "dw_plus1":
        dw, chk = _plus1_table(torch.full((n, k), float("nan")), dev)
        _refused("lfdm_multi_linear_bwd_f32 failed.*multi_linear_bwd", lambda: train_ops.multi_linear_bwd(xd, [wd], [rnd(rows, n, seed=3).to(dev)], dws=[dw]),
                 [("dw", chk)], [dw])
        return
    _refused("lfdm_multi_linear_f32 failed.*multi_linear", lambda: train_ops.multi_linear(xd, [wd], [None]), checks)
    _refused("lfdm_multi_linear_bwd_f32 failed.*multi_linear", lambda: train_ops.multi_linear_bwd(xd, [wd], [rnd(rows, n, seed=3).to(dev)]), checks)


_OPTIM_OPERANDS = {"adam_step": ("param", "grad", "exp_avg", "exp_avg_sq"), "adam_guarded_step": ("param", "grad", "exp_avg", "exp_avg_sq", "ema", "plan"),
                   "grad_sumsq": ("grad",), "optim_plan": ("plan",)}


@covers("lfdm_adam_step_f32", "refusal", dict(buffers="+1 float each"), "refused")
@covers("lfdm_adam_guarded_step_f32", "refusal", dict(buffers="+1 float each", plan="+1 float"), "refused")
@covers("lfdm_grad_sumsq_f32", "refusal", dict(grad="+1 float"), "refused")
@covers("lfdm_optim_plan_f32", "refusal", dict(plan="+1 float"), "refused")
@pytest.mark.parametrize("entry,bad", [(e, o) for e, ops_ in _OPTIM_OPERANDS.items() for o in ops_])
def test_optimizer_kernels_refuse_misaligned_buffers(backend, entry, bad):
    """optim.hip: the flat parameter / gradient / moment / EMA buffers and the plan record are float4 (resp. 16-byte) operands: one call per buffer that
    starts one float into an aligned block - refused, the buffers keep their bits."""
    from cvpr23_lfdm_amd._native import OPTIM_PLAN_BYTES
    dev = backend
    lib = ops._lib()
    n = 64
    buf, checks = {}, []
    for i, name in enumerate(("param", "grad", "exp_avg", "exp_avg_sq", "ema")):
        src = rnd(n, seed=i).abs()
        if name == bad:
            buf[name], chk = _plus1_table(src, dev)
            checks.append((name, chk))
        else:
            buf[name] = src.to(dev)
    plan_f = torch.zeros(OPTIM_PLAN_BYTES // 4 + 8)
    if bad == "plan":
        plan, chk = _plus1_table(plan_f[:OPTIM_PLAN_BYTES // 4], dev)
        checks.append(("plan", chk))
    else:
        plan = plan_f[:OPTIM_PLAN_BYTES // 4].to(dev)
    before = {k_: v.clone() for k_, v in buf.items()}
    P, s = ops._p, ops._stream(lib)
    if entry == "adam_step":
        call = lambda: lib.check(lib.lfdm_adam_step_f32(P(buf["param"]), P(buf["grad"]), P(buf["exp_avg"]), P(buf["exp_avg_sq"]), n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, s),
                                 "lfdm_adam_step_f32")
    elif entry == "adam_guarded_step":
        call = lambda: lib.check(lib.lfdm_adam_guarded_step_f32(P(buf["param"]), P(buf["grad"]), P(buf["exp_avg"]), P(buf["exp_avg_sq"]), P(buf["ema"]), n, 1e-3, 0.9, 0.999,
                                                                1e-8, 0.0, 1.0, P(plan), s), "lfdm_adam_guarded_step_f32")
    elif entry == "grad_sumsq":
        nbytes = lib.lfdm_grad_sumsq_ws_bytes(n)
        part = torch.zeros(nbytes // 4 + 4, device=dev)
        call = lambda: lib.check(lib.lfdm_grad_sumsq_f32(P(buf["grad"]), n, P(part), nbytes, s), "lfdm_grad_sumsq_f32")
    else:
        call = lambda: lib.check(lib.lfdm_optim_plan_f32(None, 0, P(plan), OPTIM_PLAN_BYTES, 0.0, 0.0, 0, 0.9, 0.999, 0.0, 1, s), "lfdm_optim_plan_f32")
    _refused("lfdm_%s_f32 failed" % entry, call, checks)
    for k_ in buf:
        assert torch.equal(buf[k_], before[k_]), "a refused %s call changed %s" % (entry, k_)


@pytest.mark.parametrize("spec", [(12, 4), (5, 1)], ids=["wide", "ragged"])
def test_groupnorm_bwd_dscale_shift_window(backend, spec):
    """dss_ld: the scale/shift gradient written into a column window of a wider table (the Python wrapper always passes a dense one): only the
    2C columns of each row are written, bit-identical to the dense call."""
    from cvpr23_lfdm_amd import train_ops
    dev = backend
    lib = ops._lib()
    b, pixels, c = 2, 48, 32
    x, dy = rnd(b * pixels, c, seed=1).to(dev), rnd(b * pixels, c, seed=5).to(dev)
    gamma, beta, ss = (1 + 0.2 * rnd(c, seed=2)).to(dev), (0.1 * rnd(c, seed=3)).to(dev), (0.3 * rnd(b, 2 * c, seed=4)).to(dev)
    _, partial, nchunk = train_ops.groupnorm_silu_train(x, b, gamma, beta, scale_shift=ss)
    dx0, _, _, dss0 = train_ops.groupnorm_silu_bwd(x, dy, b, gamma, beta, partial, nchunk, scale_shift=ss)
    dssv, chk = window((b, 2 * c), ld_extra=spec[0], col_off=spec[1], device=dev)
    dx, dgb = torch.full_like(x, float("nan")), torch.full((2, c), float("nan"), device=dev)
    nbytes = lib.lfdm_groupnorm_bwd_ws_bytes(b, pixels, c)
    ws = torch.empty(nbytes // 4 + 4, device=dev)
    lib.check(lib.lfdm_groupnorm_silu_bwd_cl_f32(ops._p(x), ops._p(dy), ops._p(dx), b, pixels, c, 8, ops._p(gamma), ops._p(beta), ops._p(ss), ss.stride(0), 1e-5, 1,
                                                 ops._p(partial), nchunk, ops._p(dgb), ops._p(dssv), dssv.stride(0), ops._p(ws), nbytes, ops._stream(lib)),
              "lfdm_groupnorm_silu_bwd_cl_f32")
    chk("groupnorm backward dscale_shift")
    no_nan(dssv, "dscale_shift")
    assert torch.equal(dssv.cpu(), dss0.cpu()) and torch.equal(dx.cpu(), dx0.cpu())
