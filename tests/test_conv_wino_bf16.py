"""The opt-in bf16-operand Winograd F(2x2,3x3) launch (lfdm_conv2d_cl_wino_bf16, conv_wino.hip BF) and its filter pack
(lfdm_pack_wino_weight_bf16) against an exact model of where it rounds:

    V = B^T d B in fp32 (the kernel's own sequence of fp32 additions), rounded once to bf16 (nearest even);
    U = the fp32 pack (lfdm_pack_wino_weight_f32), rounded once to bf16 (nearest even);
    M = sum_c U V in fp64;  Y = A^T M A in fp64, then bias / residual / activation.

(A model that forms V in fp64 and rounds it to fp32 differs from the kernel's fp32 V by an ulp in a few elements; near a bf16 rounding
boundary that flips the bf16 operand by a whole bf16 ulp, ~1e-3 of the output scale - far above the bar here.  The fp32 sequence is
part of the contract: it is the fp32 schedule's own input transform.)"""
import math

import pytest
import torch
import torch.nn.functional as F

from cvpr23_lfdm_amd import ops
from util import from_cl, to_cl

BAR = 1e-4              # kernel against the exact bf16 model, relative to max(1, max|ref|)
SANITY = 1.5e-2         # bf16 against fp32 F.conv2d: at most this, relative to max|ref| ...
DIFFERS = 1e-4          # ... and more than this (the bf16 operands were really used)


def big(dev):
    return dev == "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def unpack_f32(ww):
    """fp32 pack [pos][chunk][half j][n][kh][4] (k % 16 = 8 kh + 4 j + e) -> [16][K][coutp]"""
    p, nch, coutp = ww.shape[0], ww.shape[1], ww.shape[2]
    return ww.reshape(p, nch, 2, coutp, 2, 4).permute(0, 1, 4, 2, 5, 3).reshape(p, nch * 16, coutp)


def unpack_bf16(wwb):
    """bf16 pack [pos][chunk][n][kh][8] (k % 16 = 8 kh + s) -> [16][K][coutp]"""
    p, nch, coutp = wwb.shape[0], wwb.shape[1], wwb.shape[2]
    return wwb.permute(0, 1, 3, 2).reshape(p, nch * 16, coutp)


def input_transform_f32(x):
    """V = B^T d B of every 4x4 patch (stride 2, zero pad 1) in the order of conv_wino.hip xform_part: rows first, then columns, each step one
    fp32 addition.  x: (n, c, H, W) fp32 -> (n, c, H/2, W/2, 16), position 4 i + j."""
    d = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)             # (n, c, th, tw, 4 rows, 4 cols)
    d0, d1, d2, d3 = d[..., 0, :], d[..., 1, :], d[..., 2, :], d[..., 3, :]
    rows = (d0 - d2, d1 + d2, d2 - d1, d1 - d3)
    v = []
    for r in rows:
        r0, r1, r2, r3 = r[..., 0], r[..., 1], r[..., 2], r[..., 3]
        v += [r0 - r2, r1 + r2, r2 - r1, r1 - r3]
    return torch.stack(v, dim=-1)


AT = torch.tensor([[1., 1., 1., 0.], [0., 1., -1., -1.]], dtype=torch.float64)


def bf16_model(x, ww, cout, bias=None, residual=None, act=0, upsample=False, groups=1):
    """The exact model of the bf16 launch (module docstring).  x: (n, cin, h, w) fp32; ww: the fp32 pack (grouped: (G, 16, ...)) on the
    device the model runs on.  Returns (n, cout, H, W) fp64."""
    dev = ww.device
    x = x.to(dev)
    if upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    n, cin, H, W = x.shape
    packs = [ww] if groups == 1 else list(ww)
    cg, og = cin // groups, cout // groups
    ys = []
    for i0 in range(0, n, 8):                                              # (bounded memory at the full-size shapes)
        xv = x[i0:i0 + 8]
        outs = []
        for g, pk in enumerate(packs):
            v = input_transform_f32(xv[:, g * cg:(g + 1) * cg]).to(torch.bfloat16).double()      # (b, c, th, tw, 16)
            u = unpack_f32(pk)[:, :, :og].to(torch.bfloat16).double()                            # (16, c, o)
            m = torch.einsum("bcyxp,pco->boyxp", v, u).reshape(*v.shape[:1], og, v.shape[2], v.shape[3], 4, 4)
            y = torch.einsum("ai,noyxij,cj->noyxac", AT.to(dev), m, AT.to(dev))                   # (b, o, th, tw, 2, 2)
            outs.append(y.permute(0, 1, 2, 4, 3, 5).reshape(y.shape[0], og, H, W))
        ys.append(torch.cat(outs, dim=1))
    y = torch.cat(ys, dim=0)
    if bias is not None:
        y = y + bias.to(dev).double().view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.to(dev).double()
    if act == ops.ACT_RELU:
        y = torch.relu(y)
    elif act == ops.ACT_SILU:
        y = y * torch.sigmoid(y)
    return y


def check(got, model, fp32_ref, what):
    """The bar against the model, and the two bounds against the fp32 convolution."""
    got, model, fp32_ref = got.double().cpu(), model.cpu(), fp32_ref.double().cpu()
    err = float((got - model).abs().max())
    scale = max(1.0, float(model.abs().max()))
    assert err <= BAR * scale, "%s: %.3e against the exact bf16 model (bar %.3e)" % (what, err, BAR * scale)
    drift = float((got - fp32_ref).abs().max())
    ref_max = float(fp32_ref.abs().max())
    assert drift > DIFFERS * ref_max, "%s: %.3e from the fp32 convolution - the bf16 operands did not run" % (what, drift)
    assert drift <= SANITY * ref_max, "%s: %.3e from the fp32 convolution (bound %.3e)" % (what, drift, SANITY * ref_max)


# ------------------------------------------------------------------------------------------
def test_pack_wino_weight_bf16_is_the_rounded_fp32_pack(backend):
    """Every element of lfdm_pack_wino_weight_bf16 is the round-to-nearest-even bf16 of the element lfdm_pack_wino_weight_f32 holds - bit for bit,
    ragged coutp included, with two exact ties (position 0 of the transform is the corner tap alone: U = g[0][0])."""
    dev = backend
    cout, cin = 40, 48
    wt = rnd(cout, cin, 3, 3, seed=1)
    wt[0, 0, 0, 0] = 1.0 + 2.0 ** -8           # halfway between 1 and 1 + 2^-7: even is 1
    wt[1, 0, 0, 0] = 1.0 + 3 * 2.0 ** -8       # halfway between 1 + 2^-7 and 1 + 2^-6: even is 1 + 2^-6 (truncation gives 1 + 2^-7)
    wd = wt.to(dev)
    ww, wwb = ops.pack_wino_weight(wd), ops.pack_wino_weight_bf16(wd)
    assert wwb.dtype == torch.bfloat16 and tuple(wwb.shape) == tuple(ww.shape) == (16, cin // 16, 64, 16)
    u32, u16 = unpack_f32(ww.cpu()), unpack_bf16(wwb.cpu())
    assert float(u32[0, 0, 0]) == 1.0 + 2.0 ** -8 and float(u32[0, 0, 1]) == 1.0 + 3 * 2.0 ** -8
    assert float(u16[0, 0, 0]) == 1.0 and float(u16[0, 0, 1]) == 1.0 + 2.0 ** -6
    assert torch.equal(u16.view(torch.int16), u32.to(torch.bfloat16).view(torch.int16))
    assert not u16[:, :, cout:].float().abs().any()


def test_pack_wino_weight_grouped_bf16(backend):
    dev = backend
    ws = [rnd(32, 16, 3, 3, seed=s).to(dev) for s in (2, 3)]
    g32, g16 = ops.pack_wino_weight_grouped(ws), ops.pack_wino_weight_grouped_bf16(ws)
    assert tuple(g16.shape) == tuple(g32.shape) == (2, 16, 1, 32, 16) and g16.dtype == torch.bfloat16
    for i in range(2):
        assert torch.equal(unpack_bf16(g16[i].cpu()).view(torch.int16), unpack_f32(g32[i].cpu()).to(torch.bfloat16).view(torch.int16))


CASES = [
    dict(cin=32, cout=64, n=2, h=8, w=8),
    dict(cin=64, cout=40, n=3, h=6, w=10, residual=True, act=1),               # ragged tile block, cout not /32
    dict(cin=48, cout=64, n=2, h=8, w=8, split_src=16, residual=True),         # fused concat
    dict(cin=128, cout=32, n=1, h=4, w=4, ksplit=2, act=1),                    # split-K slabs + reduce pass
    dict(cin=32, cout=256, n=1, h=4, w=4),                                      # filters outweigh the input: XCD k owns column tile k
    dict(cin=80, cout=512, n=1, h=4, w=2, ksplit=2),                            # ... with split-K and two column tiles per XCD
    dict(cin=32, cout=64, n=2, h=4, w=6, upsample=True, act=3),                  # virtual nearest x2 upsample, SiLU
    dict(cin=48, cout=32, n=3, h=3, w=4, upsample=True, split_src=32, act=1),    # ... fused concat, odd physical height
    dict(cin=256, cout=128, n=40, h=32, w=32, upsample=True, act=1, gpu_only=True),
    dict(cin=16, cout=32, n=1, h=4, w=32, residual=True),                        # two row segments per workgroup
    dict(cin=32, cout=40, n=3, h=6, w=16, split_src=16, residual=True, act=1),    # ragged second workgroup
    dict(cin=16, cout=64, n=2, h=8, w=16, gn=True),                               # GN partial sums, halves in different samples
    dict(cin=32, cout=32, n=1, h=4, w=16, ksplit=2),
    dict(cin=64, cout=64, n=8, h=8, w=8, gn=True, act=3),
    dict(cin=64, cout=64, n=40, h=32, w=32, gpu_only=True, gn=True),
    dict(cin=512, cout=512, n=40, h=4, w=4, gpu_only=True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join("%s%s" % (k, v) for k, v in c.items()))
@pytest.mark.parametrize("bn", ["32", "64"], ids=["n32", "n64"])
def test_conv2d_winograd_bf16(backend, case, bn, monkeypatch):
    """The geometries of test_conv2d_winograd on bf16 operands, 32- and 64-column workgroups: against the exact bf16 model at 1e-4, away from the
    fp32 result by more than 1e-4 and less than 1.5e-2 of its scale; the fused GroupNorm partial sums describe the bf16 result."""
    dev = backend
    if case.get("gpu_only") and not big(dev):
        pytest.skip("full-size shapes run on the GPU")
    monkeypatch.setenv("LFDM_WINO", "1")
    monkeypatch.setenv("LFDM_WINO_BN", bn)
    cin, cout, n, h, w = (case[x] for x in ("cin", "cout", "n", "h", "w"))
    x = rnd(n, cin, h, w, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=1.0 / math.sqrt(cin * 9))
    bias = rnd(cout, seed=3)
    up = bool(case.get("upsample"))
    act = case.get("act", 0)
    fp32_ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest") if up else x, wt, bias, padding=1)
    ho, wo = fp32_ref.shape[2], fp32_ref.shape[3]
    res = rnd(n, cout, ho, wo, seed=4) if case.get("residual") else None
    if res is not None:
        fp32_ref = fp32_ref + res
    fp32_ref = F.relu(fp32_ref) if act == 1 else (F.silu(fp32_ref) if act == 3 else fp32_ref)
    xs = to_cl(x).to(dev)
    src0, src1 = xs, None
    if case.get("split_src"):
        s = case["split_src"]
        src0, src1 = xs[:, :s].contiguous(), xs[:, s:].contiguous()
    wd, ww, wwb = ops.pack_conv_weight(wt).to(dev), ops.pack_wino_weight(wt.to(dev)), ops.pack_wino_weight_bf16(wt.to(dev))
    kw = dict(src1=src1, bias=bias.to(dev), residual=None if res is None else to_cl(res).to(dev), act=act,
              ksplit=case.get("ksplit", 1), weight_wino=ww, upsample=up)
    pp, _ = ops.conv_params(src0, wd, cout, 3, 3, n, h, w, **kw)
    assert ops.conv_schedule(pp) == 2
    rows, ks = ops.conv_plan(pp)
    partial = None
    if case.get("gn") and ks == 1:
        pixels = h * w * n // 2
        partial = torch.zeros(2 * (pixels // rows), 16, device=dev)
        kw.update(gn_partial=partial, gn_groups=8, gn_pixels=pixels)
    out = ops.conv2d_cl(src0, wd, cout, 3, 3, n, h, w, weight_wino_bf16=wwb, **kw)
    model = bf16_model(x, ww, cout, bias, res, act, up)
    check(from_cl(out.cpu(), n, ho, wo), model, fp32_ref, "bf16 winograd conv")
    if partial is not None:
        conv = bf16_model(x, ww, cout, bias, None, 0, up).cpu()
        y = conv.view(2, n // 2, 8, cout // 8, h, w).permute(0, 2, 1, 3, 4, 5).reshape(2, 8, -1)
        got = partial.cpu().view(2, pixels // rows, 8, 2).double().sum(dim=1)
        for k, ref in ((0, y.sum(-1)), (1, (y * y).sum(-1))):
            assert float((got[..., k] - ref).abs().max()) <= BAR * max(1.0, float(ref.abs().max())), "gn partial %d" % k


@pytest.mark.parametrize("case", [dict(n=2, cg=16, og=32, g=2, h=4, w=8, gn=False), dict(n=4, cg=32, og=32, g=3, h=8, w=8, gn=True),
                                  dict(n=40, cg=64, og=64, g=2, h=32, w=32, gn=True, gpu_only=True)],
                         ids=lambda c: "-".join("%s%s" % kv for kv in c.items()))
def test_conv2d_winograd_bf16_grouped(backend, case):
    """Grouped heads (lfdm_conv_params.groups, the output heads' block2) on bf16 operands, with the epilogue's GroupNorm partial sums."""
    dev = backend
    if case.get("gpu_only") and not big(dev):
        pytest.skip("full-size shapes run on the GPU")
    n, cg, og, g, h, w = (case[k] for k in ("n", "cg", "og", "g", "h", "w"))
    x = rnd(n, cg * g, h, w, seed=1)
    wt = rnd(og * g, cg, 3, 3, seed=2, scale=1.0 / math.sqrt(cg * 9))
    bias = rnd(og * g, seed=3)
    parts = [wt[i * og:(i + 1) * og].to(dev) for i in range(g)]
    ww, wwb = ops.pack_wino_weight_grouped(parts), ops.pack_wino_weight_grouped_bf16(parts)
    kw = dict(bias=bias.to(dev), weight_wino=ww, groups=g)
    partial, ngn = None, 8 * g
    if case["gn"]:
        pixels = h * w * n // 2
        partial = torch.zeros(2 * (pixels // 128), 2 * ngn, device=dev)
        kw.update(gn_partial=partial, gn_groups=ngn, gn_pixels=pixels)
    out = ops.conv2d_cl(to_cl(x).to(dev), ww, og * g, 3, 3, n, h, w, weight_wino_bf16=wwb, **kw)
    model = bf16_model(x, ww, og * g, bias, groups=g)
    check(from_cl(out.cpu(), n, h, w), model, F.conv2d(x, wt, bias, padding=1, groups=g), "grouped bf16 winograd conv")
    if partial is not None:
        y = model.cpu().view(2, n // 2, ngn, og * g // ngn, h, w).permute(0, 2, 1, 3, 4, 5).reshape(2, ngn, -1)
        got = partial.cpu().view(2, pixels // 128, ngn, 2).double().sum(dim=1)
        assert float((got[..., 0] - y.sum(-1)).abs().max()) <= BAR * max(1.0, float(y.sum(-1).abs().max()))


@pytest.mark.parametrize("case", [
    dict(t=8, s=4, cin=64, cout=64, ksplit=2, residual=True),              # in-launch reduction (tile_counters)
    dict(t=8, s=4, cin=96, cout=512, ksplit=3),                            # 64-channel groups over two column tiles
    dict(t=40, s=4, cin=512, cout=512, balanced=True),                     # 640 jobs: the balanced launch (halved slices)
    dict(t=40, s=8, cin=256, cout=256, balanced=True, gpu_only=True),
    dict(t=40, s=32, cin=64, cout=64, balanced=True, gpu_only=True),
    dict(t=40, s=32, cin=128, cout=64, c1=64, balanced=True, gpu_only=True),
], ids=lambda c: "-".join("%s%s" % (k, v) for k, v in c.items()))
def test_conv2d_winograd_bf16_fused_reduce_deterministic(backend, case):
    """Split-K slabs reduced inside the launch and the balanced 640-job launch on bf16 operands: the plan is the fp32 launch's, counters end at
    zero, the result matches the exact model and is bit-identical from launch to launch; GroupNorm statistics describe it."""
    dev = backend
    if case.get("gpu_only") and not big(dev):
        pytest.skip("full-size shapes run on the GPU")
    t, s, cin, cout = (case[k] for k in ("t", "s", "cin", "cout"))
    c1 = case.get("c1", 0)
    x = rnd(t, cin, s, s, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=1.0 / math.sqrt(9 * cin))
    bias = rnd(cout, seed=3)
    res = rnd(t, cout, s, s, seed=7) if case.get("residual") or case.get("balanced") else None
    xs = to_cl(x).to(dev)
    src0, src1 = (xs, None) if not c1 else (xs[:, :cin - c1].contiguous(), xs[:, cin - c1:].contiguous())
    w, ww, wwb = ops.pack_conv_weight(wt).to(dev), ops.pack_wino_weight(wt.to(dev)), ops.pack_wino_weight_bf16(wt.to(dev))
    counters = torch.zeros(1024, dtype=torch.int32, device=dev)
    kw = dict(src1=src1, bias=bias.to(dev), weight_wino=ww, residual=None if res is None else to_cl(res).to(dev), tile_counters=counters)
    if "ksplit" in case:
        kw["ksplit"] = case["ksplit"]
    pp, _ = ops.conv_params(src0, w, cout, 3, 3, t, s, s, **kw)
    assert ops.conv_schedule(pp) == 2
    pp.gn_partial = 1
    rows, ks = ops.conv_plan(pp)
    slabs = ops.conv_plan_slabs(pp)
    assert rows == 128 and (slabs > ks if case.get("balanced") else ks == case["ksplit"] > 1), (rows, ks, slabs)
    pixels, groups = t * s * s, 8
    nchunk = pixels // 128 * max(1, cout // groups // 32)
    outs = []
    for rep in range(2):
        partial = torch.zeros(nchunk, 2 * groups, device=dev)
        y = ops.conv2d_cl(src0, w, cout, 3, 3, t, s, s, gn_partial=partial, gn_groups=groups, gn_pixels=pixels, weight_wino_bf16=wwb, **kw)
        assert int(counters.abs().sum()) == 0
        outs.append((y.clone(), partial.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "bf16 launches must repeat bit for bit"
    fp32_ref = F.conv2d(x, wt, bias, padding=1) + (0 if res is None else res)
    model = bf16_model(x, ww, cout, bias, res)
    check(from_cl(outs[0][0].cpu(), t, s, s), model, fp32_ref, "bf16 split-K reduced in the launch")


def test_conv2d_winograd_bf16_refuses_other_schedules(backend):
    """lfdm_conv2d_cl_wino_bf16 runs the Winograd F(2x2) schedule only: a geometry the plan gives to another schedule (LFDM_WINO=0 here, a 1x1
    filter in the library's view) and the pooled form are refused with the library's error, never run in fp32 or on other operands."""
    dev = backend
    n, c, s = 2, 32, 8
    x = to_cl(rnd(n, c, s, s, seed=1)).to(dev)
    wt = rnd(c, c, 3, 3, seed=2, scale=0.05)
    w, ww, wwb = ops.pack_conv_weight(wt).to(dev), ops.pack_wino_weight(wt.to(dev)), ops.pack_wino_weight_bf16(wt.to(dev))
    with pytest.raises(ops.WinogradUnavailable):
        ops.conv2d_cl(x, w, c, 3, 3, n, s, s, weight_wino=ww, weight_wino_bf16=wwb, pool2=True, act=ops.ACT_RELU)
    p, _ = ops.conv_params(x, w, c, 3, 3, n, s, s, weight_wino=ww, stride=2)
    assert ops.conv_schedule(p) != 2
    with pytest.raises(RuntimeError, match="wino_bf16"):
        ops.conv_launch_wino_bf16(p, wwb)
    with pytest.raises(TypeError):
        ops.conv2d_cl(x, w, c, 3, 3, n, s, s, weight_wino=ww, weight_wino_bf16=ww)
