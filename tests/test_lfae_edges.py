"""The LFAE kernels - the forward warp (csrc/warp.hip), the predictor glue (csrc/lfae_aux.hip) and stage-1 training (csrc/train_lfae.hip) - at
the edges of their launch plans, against float64 torch on the CPU: the ATen graph the reference model builds, or the closed formula for the
predictor kernels.  tests/test_lfae_ops.py and tests/test_lfae_predictors.py pin the shapes the shipped configuration uses (inflated to
workload size on the device); this file takes the branches next to them: non-power-of-two lane groups, unstaged and ragged frame blocks,
one-pixel images, maps larger than the image, chunk counts on both sides of a ticket group and of a block cap, K = 1 and K = 32 regions.
The shapes are the smallest that reach each branch and are the same on both backends ("emu": index logic on a GPU-less machine; "hip":
what only the device shows - 64-bit integer atomics, ticketed folds that read partials past the L2s, xor-shuffle sums over lane groups,
LDS-staged planes).

Bars are the project's own: test_lfae_ops.TOL for kernel entry points (gradients divided by the reference's largest magnitude), 1e-5 for
the blur, 1e-6 for the pooling family, 1e-4 / 5e-4 for the SVD.  Where a case is ill-conditioned on purpose (BatchNorm on mean >> std, or on
two rows) the bar is max(TOL, 2 x the error of the fp32 ATen op against float64 on the same inputs).  Every destination is handed over NaN-filled - through
the wrapper's `out=` or by calling the entry point through ops._lib() - a row a kernel forgot to write stays NaN instead of holding a
previous call's values.  The cases marked `twice` run a second time on the same inputs and must give the same bits, and the persistent
words (BatchNorm tickets, the scatter's max word and accumulator) must be zero after every run.  Nothing is excluded from a comparison:
where a premise is needed (a singular-value gap, no ReLU pre-activation next to zero, no sampling position on a pixel centre) the inputs
are built so that it holds everywhere and the premise is asserted.  The coverage table is in tests/test_ops_parity.py."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from cvpr23_lfdm_amd import lfae_ops as L
from cvpr23_lfdm_amd import ops
from cvpr23_lfdm_amd import params as P
from cvpr23_lfdm_amd._native import WarpBwdParams
from test_lfae_ops import TOL, _antialias_ref, _apply_optical_ref, _flow
from util import assert_close, record_margin, rnd

NAN = float("nan")


def _nan(shape, dev):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device=dev)


def _written(t, what):
    assert not bool(torch.isnan(t).any()), "%s: NaN left in the destination (elements the kernel never wrote)" % what


def _untouched(t, what):
    assert bool(torch.isnan(t).all()), "%s: written although it lies outside the destination (or the call was refused)" % what


def _scaled(got, ref, what, tol=TOL):
    """a gradient: compared relative to the reference's largest magnitude (an all-zero reference is compared as it stands)"""
    sc = float(ref.abs().max()) or 1.0
    assert_close(got.cpu() / sc, ref / sc, tol, what)


def _same_bits(first, second, what):
    for i, (a, b) in enumerate(zip(first, second)):
        if a is not None:
            assert torch.equal(a, b), "%s: output %d differs between two runs on the same inputs" % (what, i)


def _state_clean(dev, what):
    st = L._state(torch.device(dev))
    assert int(st["tickets"].abs().max()) == 0, what + ": BatchNorm ticket words not handed back zeroed"
    assert int(st["amax"].abs().max()) == 0, what + ": max word / finalize ticket / L1 ticket not handed back zeroed"
    assert st["fix"] is None or int(st["fix"].abs().max()) == 0, what + ": fixed-point accumulator not handed back zeroed"


def _call(name, *args):
    lib = ops._lib()
    lib.check(getattr(lib, name)(*args, ops._stream(lib)), name)


def _rows(x):
    """(N, C, H, W) -> channels-last rows (N*H*W, C)"""
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def _unrows(r, n, h, w):
    return r.reshape(n, h, w, r.shape[1]).permute(0, 3, 1, 2)


def _wide(rows, ld, dev, fill=NAN):
    """`rows` as the first columns of a (rows, ld) buffer whose other columns hold `fill`: the operand and the whole buffer"""
    buf = torch.full((rows.shape[0], ld), fill, dtype=torch.float32)
    buf[:, :rows.shape[1]] = rows
    buf = buf.to(dev)
    return buf[:, :rows.shape[1]], buf


def _sample_positions_clear(flow, h, w, what, resize=True):
    """the premise of a comparison of map gradients: the gradient of a bilinear tap set jumps where a sampling position crosses a pixel
    centre, so no position (of the float64 reference) may lie within 1e-5 of one.  (h, w): the sampled image."""
    f = flow.detach()
    if resize and (f.shape[1] != h or f.shape[2] != w):
        f = F.interpolate(f.permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    ix, iy = ((f[..., 0] + 1) * w - 1) / 2, ((f[..., 1] + 1) * h - 1) / 2
    d = torch.minimum((ix - ix.round()).abs().min(), (iy - iy.round()).abs().min())
    assert float(d) > 1e-5, "%s: a sampling position lies on a pixel centre (%.2e): the case does not hold its premise" % (what, float(d))


# ------------------------------------------------------------------------------------------------------------------------------------
# 1.  lfdm_warp_cl_f32: warp_cl_kernel<R> with R = 4 (C % 16 == 0), 2 (C % 8 == 0), 1; g = C / (4 R) lanes per pixel

# (c, h, w, fh, fw, ld): (12: R 1, g 3 - `idx / g`) (24: R 2, g 3) (40: R 2, g 5, maps shrunk in x and stretched in y) (48: R 4, g 3)
# (20: R 1, g 5) (64: R 4, g 4 - the shift) (4: one lane, one pixel) (24 in rows of 32 / 36 / 40 floats)
WARP_CL_CASES = [(12, 5, 7, 5, 7, 0), (24, 6, 10, 3, 5, 0), (40, 9, 7, 4, 9, 0), (48, 3, 3, 2, 2, 0), (20, 8, 8, 8, 8, 0), (64, 7, 5, 7, 5, 0),
                 (4, 1, 1, 1, 1, 0), (24, 5, 3, 2, 4, 8)]


@pytest.mark.parametrize("c,h,w,fh,fw,ld", WARP_CL_CASES)
@pytest.mark.parametrize("mode", ["deform", "mask", "blend"])
def test_warp_cl_lane_groups(backend, c, h, w, fh, fw, ld, mode):
    dev = backend
    b, t = 2, 3
    n = b * t
    src, prev = rnd(b, c, h, w, seed=1), rnd(n, c, h, w, seed=2)
    flow = _flow(n, fh, fw, 3, amp=0.6)                                   # large enough that taps leave the image
    occ = torch.sigmoid(rnd(n, 1, fh, fw, seed=4))
    ref = _apply_optical_ref(src.double().repeat_interleave(t, 0), prev.double() if mode == "blend" else None, flow.double(),
                             None if mode == "deform" else occ.double())
    fx, fy = flow[..., 0].contiguous().to(dev), flow[..., 1].contiguous().to(dev)
    od = None if mode == "deform" else occ.contiguous().to(dev)
    if ld:
        sd, _ = _wide(_rows(src), c + ld, dev)
        pd, _ = _wide(_rows(prev), c + ld + 4, dev)
        out, whole = _wide(torch.full((n * h * w, c), NAN), c + ld + 8, dev)
    else:
        sd, pd, out = _rows(src).to(dev), _rows(prev).to(dev), _nan((n * h * w, c), dev)
    got = ops.warp_cl(sd, b, t, h, w, fx, fy, od, fh, fw, t * fh * fw, fh * fw, prev=pd if mode == "blend" else None, out=out)
    _written(got, "warp_cl")
    if ld:
        _untouched(whole[:, c:], "warp_cl: the columns behind the row")
    assert_close(_unrows(got.cpu(), n, h, w), ref, TOL, "lfdm_warp_cl_f32 out")


# ------------------------------------------------------------------------------------------------------------------------------------
# 2.  lfdm_warp_planar_f32: warp_planar_kernel<STAGED> over blocks of fpb frames, warp_planar_pixel_kernel below 2048 planes

# (b, c, t, h, w, fh, fw): (1030 x 2 planes of 3x3: unstaged, hw % 4 != 0, fpb 4 > frames) (520 x 2 x 2 of 5x7: unstaged) (700 x 3 of 4x4:
# staged, fpb 4, last block one frame) (300 x 7 x 2: staged, fpb 8 against 7 frames) (2 x 1025 frames: blocks of 4, one frame left)
# (5 channels: pixel kernel, second channel quad one channel) (one pixel)
WARP_PLANAR_CASES = [(1, 1030, 2, 3, 3, 3, 3), (2, 520, 2, 5, 7, 2, 3), (1, 700, 3, 4, 4, 4, 4), (2, 300, 7, 6, 6, 3, 3), (1, 2, 1025, 2, 2, 2, 2),
                     (1, 5, 3, 9, 9, 4, 4), (1, 3, 1, 1, 1, 1, 1)]


@pytest.mark.parametrize("b,c,t,h,w,fh,fw", WARP_PLANAR_CASES)
@pytest.mark.parametrize("mode", ["deform", "mask", "blend", "blend_cl"])
def test_warp_planar_frame_blocks(backend, b, c, t, h, w, fh, fw, mode):
    dev = backend
    n = b * t
    src, prev = rnd(b, c, h, w, seed=1), rnd(n, c, h, w, seed=2)
    flow = _flow(n, fh, fw, 3, amp=0.6)
    occ = torch.sigmoid(rnd(n, 1, fh, fw, seed=4))
    blend = mode in ("blend", "blend_cl")
    ref = _apply_optical_ref(src.double().repeat_interleave(t, 0), prev.double() if blend else None, flow.double(),
                             None if mode == "deform" else occ.double())
    ref = ref.view(b, t, c, h, w).permute(0, 2, 1, 3, 4)
    fx, fy = flow[..., 0].contiguous().to(dev), flow[..., 1].contiguous().to(dev)
    od = None if mode == "deform" else occ.contiguous().to(dev)
    kw = {}
    if mode == "blend":
        kw = dict(prev=prev.view(b, t, c, h, w).permute(0, 2, 1, 3, 4).contiguous().to(dev))
    elif mode == "blend_cl":
        pd, _ = _wide(_rows(prev), (c + 3) // 4 * 4 + 4, dev)            # channels of wider channels-last rows: ld_prev > c
        kw = dict(prev=pd, prev_is_cl=True)
    got = ops.warp_planar(src.to(dev), t, fx, fy, od, fh, fw, t * fh * fw, fh * fw, out=_nan((b, c, t, h, w), dev), **kw)
    _written(got, "warp_planar")
    assert_close(got.cpu(), ref, TOL, "lfdm_warp_planar_f32 out")


# ------------------------------------------------------------------------------------------------------------------------------------
# 3.  ApplyOpticalCL / ApplyOpticalImage: lfdm_warp_cl_f32 | lfdm_warp_planar_f32, lfdm_absmax_f32, lfdm_warp_bwd_f32,
#     lfdm_fix_finalize_f32, lfdm_resize_adjoint_f32 chained as lfae_ops chains them, on destinations of the test's own

# (c, h, w, fh, fw): g = 1 at map resolution, square and not | maps smaller | maps LARGER than the image in one or both directions (the
# adjoint's other regime) | g = 64 over 15 pixels | several ragged workgroups | a single map pixel | a single map row | one pixel
OPTICAL_CASES = [(4, 8, 8, 8, 8), (4, 5, 7, 5, 7), (8, 9, 7, 5, 3), (8, 8, 6, 3, 7), (8, 8, 8, 11, 5), (16, 6, 10, 12, 20), (256, 3, 5, 2, 2),
                 (64, 17, 19, 4, 4), (8, 2, 2, 1, 1), (8, 7, 9, 1, 4), (4, 1, 1, 1, 1)]
OPTICAL_TWICE = ((8, 9, 7, 5, 3), (64, 17, 19, 4, 4))
OPTICAL_SUBSETS = ["all", "src_const", "no_prev", "prev_const", "no_occ"]


def _optical_cl(dev, sr, pr, dr, maps, n, h, w, c, want_dsrc, want_dprev):
    """forward and backward of lfae_ops.ApplyOpticalCL on row operands -> (out, dsrc, dprev, dmaps at map resolution)"""
    fh, fw, planes = maps.shape[2], maps.shape[3], maps.shape[1]
    st = L._state(torch.device(dev))
    out = ops.warp_cl(sr, n, 1, h, w, maps[:, 0], maps[:, 1], maps[:, 2] if planes == 3 else None, fh, fw, planes * fh * fw, 0, prev=pr,
                      out=_nan((n * h * w, c), dev))
    p = WarpBwdParams()
    L._warp_bwd_common(p, maps, n, h, w, c)
    p.layout_cl, p.n_div = 1, 1
    p.src, p.ld_src, p.dout, p.ld_dout = sr.data_ptr(), sr.stride(0), dr.data_ptr(), dr.stride(0)
    dprev = dsrc = None
    if pr is not None:
        p.prev, p.ld_prev = pr.data_ptr(), pr.stride(0)
        if want_dprev:
            dprev = _nan((n * h * w, c), dev)
            p.dprev, p.ld_dprev = dprev.data_ptr(), c
    dmaps = _nan((n, 3, h, w), dev)
    p.dmaps = dmaps.data_ptr()
    if want_dsrc:
        acc = L._fix_acc(torch.device(dev), n * h * w * c)
        p.dsrc_fix, p.amax_bits = acc.data_ptr(), st["amax"].data_ptr()
        _call("lfdm_absmax_f32", ops._p(dr), n * h * w, c, dr.stride(0), ops._p(st["amax"]))
    _call("lfdm_warp_bwd_f32", C.byref(p))
    if want_dsrc:
        dsrc = _nan((n * h * w, c), dev)
        _call("lfdm_fix_finalize_f32", ops._p(acc), ops._p(dsrc), n * h * w, c, c, ops._p(st["amax"]), 4 * h * w,
              C.c_void_p(st["amax"].data_ptr() + 4))
    return out, dsrc, dprev, _fold_maps(dev, dmaps, n, h, w, fh, fw, planes)


def _fold_maps(dev, dmaps, n, h, w, fh, fw, planes):
    _written(dmaps, "warp_bwd dmaps")
    if (fh, fw) == (h, w):
        return dmaps[:, :planes]
    low = _nan((n, 3, fh, fw), dev)
    _call("lfdm_resize_adjoint_f32", ops._p(dmaps), ops._p(low), n * 3, h, w, fh, fw)
    _written(low, "resize_adjoint")
    return low[:, :planes]


def _optical_reference(src, prev, flow, occ, dy, subset):
    s64, f64 = src.double().requires_grad_(subset != "src_const"), flow.double().requires_grad_(True)
    p64 = None if subset in ("no_prev", "no_occ") else prev.double().requires_grad_(subset != "prev_const")
    o64 = None if subset == "no_occ" else occ.double().requires_grad_(True)
    ref = _apply_optical_ref(s64, p64, f64, o64)
    ref.backward(dy.double())
    return ref.detach(), s64, p64, f64, o64


@pytest.mark.parametrize("c,h,w,fh,fw", OPTICAL_CASES)
@pytest.mark.parametrize("subset", OPTICAL_SUBSETS)
def test_apply_optical_cl_edges(backend, c, h, w, fh, fw, subset):
    dev = backend
    n = 2
    src, prev, dy = rnd(n, c, h, w, seed=1), rnd(n, c, h, w, seed=2), rnd(n, c, h, w, seed=5)
    flow, occ = _flow(n, fh, fw, 3, amp=0.6), torch.sigmoid(rnd(n, 1, fh, fw, seed=4))
    ref, s64, p64, f64, o64 = _optical_reference(src, prev, flow, occ, dy, subset)
    _sample_positions_clear(f64, h, w, "apply_optical")
    maps = L._maps_planar(flow, None if o64 is None else occ).to(dev)
    sr, dr = _rows(src).to(dev), _rows(dy).to(dev)
    pr = None if p64 is None else _rows(prev).to(dev)

    def run():
        res = _optical_cl(dev, sr, pr, dr, maps, n, h, w, c, s64.requires_grad, p64 is not None and p64.requires_grad)
        _state_clean(dev, "apply_optical")
        return res

    out, dsrc, dprev, dm = run()
    _written(out, "warp_cl out")
    assert_close(_unrows(out.cpu(), n, h, w), ref, TOL, "lfdm_warp_cl_f32 (training) out")
    assert (dsrc is not None) == s64.requires_grad and (dprev is not None) == (p64 is not None and p64.requires_grad)
    if dsrc is not None:
        _written(dsrc, "fix_finalize dsrc")
        _scaled(_unrows(dsrc, n, h, w), s64.grad, "lfdm_warp_bwd_f32 dsrc")
    if dprev is not None:
        _written(dprev, "warp_bwd dprev")
        _scaled(_unrows(dprev, n, h, w), p64.grad, "lfdm_warp_bwd_f32 dprev")
    _scaled(dm[:, :2], f64.grad.permute(0, 3, 1, 2), "lfdm_warp_bwd_f32 dflow")
    if o64 is not None:
        _scaled(dm[:, 2:], o64.grad, "lfdm_warp_bwd_f32 docc")
    if (c, h, w, fh, fw) in OPTICAL_TWICE:
        _same_bits((out, dsrc, dprev, dm), run(), "apply_optical forward + backward")


@pytest.mark.parametrize("h,w,fh,fw", list(dict.fromkeys(s[1:] for s in OPTICAL_CASES)))
@pytest.mark.parametrize("c", [1, 3])
def test_apply_optical_image_edges(backend, h, w, fh, fw, c):
    """The same geometries through the strided form (warp_planar_pixel_kernel, warp_bwd_px_kernel): an image of one or three channels; with
    three, prev and its gradient are channel rows of a 4-wide channels-last tensor (a convolution's output)."""
    dev = backend
    n = 2
    src, prev, dy = rnd(n, c, h, w, seed=1).abs(), torch.sigmoid(rnd(n, c, h, w, seed=2)), rnd(n, c, h, w, seed=5)
    flow, occ = _flow(n, fh, fw, 3, amp=0.5), torch.sigmoid(rnd(n, 1, fh, fw, seed=4))
    ref, _, p64, f64, o64 = _optical_reference(src, prev, flow, occ, dy, "src_const")
    _sample_positions_clear(f64, h, w, "apply_optical_image")
    maps = L._maps_planar(flow, occ).to(dev)
    sd, dyd = src.to(dev), dy.to(dev)
    if c == 3:
        pr, _ = _wide(_rows(prev), 4, dev, fill=0.0)
        pv = pr.view(n, h, w, 3).permute(0, 3, 1, 2)
        dq, dq_whole = _wide(torch.full((n * h * w, 3), NAN), 4, dev)
        dprev = dq.view(n, h, w, 3).permute(0, 3, 1, 2)
        kw = dict(prev=pr, prev_is_cl=True)
    else:
        pv, dprev = prev.to(dev), _nan((n, c, h, w), dev)
        kw = dict(prev=pv)
    out = ops.warp_planar(sd, 1, maps[:, 0], maps[:, 1], maps[:, 2], fh, fw, 3 * fh * fw, 0, out=_nan((n, c, 1, h, w), dev), **kw)
    _written(out, "warp_planar out")
    assert_close(out.view(n, c, h, w).cpu(), ref, TOL, "lfdm_warp_planar_f32 (training) out")
    p = WarpBwdParams()
    L._warp_bwd_common(p, maps, n, h, w, c)
    p.layout_cl, p.n_div = 0, 1
    p.src, p.dout, p.prev, p.dprev = sd.data_ptr(), dyd.data_ptr(), pv.data_ptr(), dprev.data_ptr()
    p.ss_n, p.ss_c, p.ss_h, p.ss_w = sd.stride()
    p.ds_n, p.ds_c, p.ds_h, p.ds_w = dyd.stride()
    p.ps_n, p.ps_c, p.ps_h, p.ps_w = pv.stride()
    p.dps_n, p.dps_c, p.dps_h, p.dps_w = dprev.stride()
    dmaps = _nan((n, 3, h, w), dev)
    p.dmaps = dmaps.data_ptr()
    _call("lfdm_warp_bwd_f32", C.byref(p))
    dm = _fold_maps(dev, dmaps, n, h, w, fh, fw, 3)
    _written(dprev, "warp_bwd (strided) dprev")
    if c == 3:
        _untouched(dq_whole[:, 3], "warp_bwd (strided): the fourth channel of the dprev rows")
    _scaled(dprev, p64.grad, "lfdm_warp_bwd_f32 (strided) dprev")
    _scaled(dm[:, :2], f64.grad.permute(0, 3, 1, 2), "lfdm_warp_bwd_f32 (strided) dflow")
    _scaled(dm[:, 2:], o64.grad, "lfdm_warp_bwd_f32 (strided) docc")
    _state_clean(dev, "apply_optical_image")


# ------------------------------------------------------------------------------------------------------------------------------------
# 4.  lfdm_resize_adjoint_f32 alone, against the float64 autograd adjoint of F.interpolate(bilinear, align_corners=False)

# (h, w, fh, fw): up-scaling | ragged | fh * fw = 600 over blocks of 256, shrinking in x | shrinking both ways | one map pixel | one image pixel
# | equal sizes (the identity, which lfae_ops never asks for)
@pytest.mark.parametrize("h,w,fh,fw", [(8, 8, 3, 3), (9, 7, 5, 3), (5, 40, 2, 300), (4, 4, 9, 11), (7, 7, 1, 1), (1, 1, 4, 4), (8, 8, 8, 8)])
@pytest.mark.parametrize("planes", [1, 6])
def test_resize_adjoint_edges(backend, h, w, fh, fw, planes):
    dev = backend
    low = torch.zeros(1, planes, fh, fw, dtype=torch.float64, requires_grad=True)
    dhigh = rnd(planes, h, w, seed=1)
    F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False).backward(dhigh.double()[None])
    dhd, got = dhigh.to(dev), _nan((planes, fh, fw), dev)
    _call("lfdm_resize_adjoint_f32", ops._p(dhd), ops._p(got), planes, h, w, fh, fw)
    _written(got, "resize_adjoint")
    _scaled(got, low.grad[0], "lfdm_resize_adjoint_f32")


# ------------------------------------------------------------------------------------------------------------------------------------
# 5.  lfdm_absmax_f32 / lfdm_fix_finalize_f32: exact results

# (rows, c, ld): one float4 | the scalar path (c % 4 != 0) | rows of 12 floats | one item beyond the block caps of both kernels (absmax: 2048
# blocks of 4096 floats; finalize: 4096 blocks of 2048)
FIX_CASES = [(1, 4, 4), (5, 3, 5), (7, 8, 12), (2 ** 21 + 1, 4, 4)]


@pytest.mark.parametrize("rows,c,ld", FIX_CASES)
@pytest.mark.parametrize("where", ["last", "first"])
def test_absmax_exact(backend, rows, c, ld, where):
    dev = backend
    x = rnd(rows, c, seed=1)
    x[-1 if where == "last" else 0, -1 if where == "last" else 0] = -7.25          # beyond any |randn| of these sizes
    assert float(x.abs().max()) == 7.25
    xd, _ = _wide(x, ld, dev, fill=1e30)                                          # what lies behind a row is not read
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("lfdm_absmax_f32", ops._p(xd), rows, c, ld, ops._p(word))
    assert int(word) == int(torch.tensor(7.25).view(torch.int32)), "absmax: not the bit pattern of max |x|"


def _fix_exponent(amax, count):
    if not amax > 0:
        return 0
    e = math.frexp(amax)[1]
    lc = 0
    while (1 << lc) < count:
        lc += 1
    return max(-120, min(120, 62 - lc - e))


# (the block cap is a property of the size: one scale is enough there)
@pytest.mark.parametrize("rows,c,ld,amax", [s + (a,) for s in FIX_CASES[:3] for a in (0.0, 1e-30, 1.0, 3e4, 1e30)] + [FIX_CASES[3] + (1.0,)])
def test_fix_finalize_exact(backend, rows, c, ld, amax):
    dev = backend
    count = 4 * 15 * 17
    amax32 = float(torch.tensor(amax, dtype=torch.float32))
    k = _fix_exponent(amax32, count)
    v = rnd(rows, c, seed=2).double().clamp(-1, 1) * (amax32 if amax32 > 0 else 1000.0) * count
    q = torch.round(v * 2.0 ** k).to(torch.int64)                                 # |q| <= count * amax * 2^k < 2^62
    want = (q.double() * 2.0 ** -k).float()
    acc = q.reshape(-1).clone().to(dev)
    words = torch.zeros(2, dtype=torch.int32, device=dev)
    words[0] = int(torch.tensor(amax32).view(torch.int32))
    out, whole = _wide(torch.full((rows, c), NAN), ld, dev)
    _call("lfdm_fix_finalize_f32", ops._p(acc), ops._p(out), rows, c, ld, ops._p(words), count, C.c_void_p(words.data_ptr() + 4))
    _written(out, "fix_finalize")
    if ld > c:
        _untouched(whole[:, c:], "fix_finalize: the columns behind the row")
    assert torch.equal(out.cpu(), want), "fix_finalize: not ldexp(q, -k)"
    assert int(acc.abs().max()) == 0 and int(words.abs().max()) == 0, "fix_finalize: accumulator / max word / ticket not left zero"


# ------------------------------------------------------------------------------------------------------------------------------------
# 6.  lfdm_batchnorm_train_{fwd,bwd}_cl_f32: bn_reduce_kernel / bn_apply_kernel over chunks of >= 128 rows, ticket groups of 32 chunks

EPS, MOM = 1e-5, 0.1


def _bn_reference(x, g, b, rm, rv, dy, relu, segments, add, dtype):
    """S module calls of nn.BatchNorm2d in training mode (+ ReLU) on the S sub-batches, in `dtype`: (y, stat, rm, rv, dx, dgamma, dbeta, pre).
    One row per channel has no unbiased variance (the module refuses it): the running variance then takes the biased one, 0."""
    x = x.to(dtype).requires_grad_(True)
    g, b = g.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    ys, stats = [], []
    for xs in x.chunk(segments):
        mean, var = xs.mean(0), xs.var(0, unbiased=False)
        if xs.shape[0] > 1:
            ys.append(F.batch_norm(xs, rm, rv, g, b, True, MOM, EPS))
        else:
            ys.append((xs - mean) / (var + EPS).sqrt() * g + b)
            rm.mul_(1 - MOM).add_(MOM * mean.detach())
            rv.mul_(1 - MOM).add_(MOM * var.detach())
        stats.append(torch.stack((mean.detach(), 1 / (var.detach() + EPS).sqrt())))
    pre = torch.cat(ys)
    y = F.relu(pre) if relu else pre
    y.backward(dy.to(dtype))
    dx = x.grad if add is None else x.grad + add.to(dtype)
    return y.detach(), torch.stack(stats), rm, rv, dx, g.grad, b.grad, pre.detach()


def _bn_kernel(dev, xd, dyd, gd, bd, rm, rv, relu, segments, addd, ld_out):
    rows, c = xd.shape
    seg_rows = rows // segments
    lib = ops._lib()
    nbytes = lib.lfdm_batchnorm_train_ws_bytes(seg_rows, c, segments)
    tk = ops._p(L._state(torch.device(dev))["tickets"])
    y, y_whole = _wide(torch.full((rows, c), NAN), ld_out, dev)
    dx, dx_whole = _wide(torch.full((rows, c), NAN), ld_out, dev)
    stat, dg, db = _nan((segments, 2, c), dev), _nan((c,), dev), _nan((c,), dev)
    rmd, rvd = rm.to(dev), rv.to(dev)
    ws = _nan(((nbytes + 3) // 4,), dev)                      # partials read before they are written would show as NaN
    _call("lfdm_batchnorm_train_fwd_cl_f32", ops._p(xd), ops._p(y), seg_rows, c, segments, xd.stride(0), ld_out, ops._p(gd), ops._p(bd),
          ops._p(rmd), ops._p(rvd), MOM, EPS, int(relu), ops._p(stat), ops._p(ws), nbytes, tk)
    ws = _nan(((nbytes + 3) // 4,), dev)
    _call("lfdm_batchnorm_train_bwd_cl_f32", ops._p(xd), ops._p(dyd), ops._p(dx), seg_rows, c, segments, xd.stride(0), dyd.stride(0), ld_out,
          ops._p(addd), 0 if addd is None else addd.stride(0), ops._p(gd), ops._p(bd), ops._p(stat), int(relu), ops._p(dg), ops._p(db),
          ops._p(ws), nbytes, tk)
    for t, what in ((y, "bn y"), (stat, "bn stat"), (rmd, "bn running_mean"), (rvd, "bn running_var"), (dx, "bn dx"), (dg, "bn dgamma"),
                    (db, "bn dbeta")):
        _written(t, what)
    if ld_out > c:
        _untouched(y_whole[:, c:], "bn y: the columns behind the row")
        _untouched(dx_whole[:, c:], "bn dx: the columns behind the row")
    _state_clean(dev, "batchnorm")
    return y, stat, rmd, rvd, dx, dg, db


def _err(got, ref, scaled):
    """the figure assert_close / _scaled compare with their bar"""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    sc = float(ref.abs().max())
    return float((got - ref).abs().max()) / ((sc or 1.0) if scaled else max(1.0, sc))


BN_NAMES = ("y", "stat", "running_mean", "running_var", "dx", "dgamma", "dbeta")
BN_SCALED = (False, False, False, False, True, True, True)


def _bn_case(dev, rows, c, relu, mean, std, segments=1, sliced=False, fork=False, twice=False, derived=False):
    """rows: per segment.  derived: the case is ill-conditioned in fp32 whoever computes it, and its bar is max(TOL, 2 x the error of the fp32 ATen
    op - what the reference model runs - against float64 on the same inputs); otherwise the bar is TOL."""
    total = rows * segments
    x = rnd(total, c, seed=1) * std + mean
    x = x + torch.arange(segments).repeat_interleave(rows).view(-1, 1).float() * std             # different means per segment
    g, b = rnd(c, seed=2) * 0.3 + 1.0, rnd(c, seed=3) * 0.2
    rm, rv = rnd(c, seed=4) * 0.1, rnd(c, seed=5).abs() + 0.5
    dy = rnd(total, c, seed=6)
    add = rnd(total, c, seed=7) if fork else None
    if relu:
        # premise of the mask comparison: no float64 pre-activation within 1e-4 of zero.  Moving an element moves its segment's statistics a
        # little, hence the passes; the assertion is what counts.
        for _ in range(8):
            pre = _bn_reference(x, g, b, rm, rv, dy, False, segments, None, torch.float64)[7]
            near = pre.abs() < 2e-4
            if not bool(near.any()):
                break
            x = torch.where(near, x + 0.01 * std * torch.where(pre >= 0, 1.0, -1.0).float(), x)
    ref = _bn_reference(x, g, b, rm, rv, dy, relu, segments, add, torch.float64)
    aten = _bn_reference(x, g, b, rm, rv, dy, relu, segments, add, torch.float32)
    if relu:
        assert float(ref[7].abs().min()) >= 1e-4, "a pre-activation lies next to zero: the case does not hold its premise"
    if sliced:
        xd, _ = _wide(x, c + 8, dev)
        dyd, _ = _wide(dy, c + 12, dev)
        addd = None if add is None else _wide(add, c + 4, dev)[0]
    else:
        xd, dyd, addd = x.to(dev), dy.to(dev), None if add is None else add.to(dev)
    run = lambda: _bn_kernel(dev, xd, dyd, g.to(dev), b.to(dev), rm, rv, relu, segments, addd, c + 16 if sliced else c)
    got = run()
    if relu:
        assert torch.equal(got[0].cpu() > 0, ref[0] > 0), "bn: the ReLU mask differs from the float64 reference's"
    failures = []
    for name, scaled, k, r, a in zip(BN_NAMES, BN_SCALED, got, ref, aten):
        e_kernel, e_aten = _err(k, r, scaled), _err(a, r, scaled)
        bar = max(TOL, 2 * e_aten) if derived else TOL
        record_margin("lfdm_batchnorm_train_cl_f32 %s (mean %g, std %g; fp32 ATen %.3e)" % (name, mean, std, e_aten), e_kernel, 1.0, bar)
        print("bn %s rows %d c %d mean %g std %g relu %d: kernel %.3e, fp32 ATen %.3e, bar %.3e" % (name, rows, c, mean, std, relu, e_kernel, e_aten, bar))
        if not e_kernel <= bar:
            failures.append("bn %s: error %.3e against float64 over the bar %.3e (%s; fp32 ATen: %.3e)"
                            % (name, e_kernel, bar, "max(TOL, 2 x fp32 ATen)" if derived else "TOL", e_aten))
    assert not failures, "; ".join(failures)
    if twice:
        _same_bits(got, run(), "batchnorm forward + backward")


# rows x c.  (1: variance 0, no unbiased variance) (2) (127 | 128: one chunk; 129: two; q = 4 at c <= 16, 8 at c <= 32, 16 above - c = 20 and
# 36 leave the last channel tile ragged) (4096 | 4097: 32 | 33 chunks = one | two ticket groups) (131072 | 131073: the 1024-chunk cap, exact
# and with ragged chunks of 129 rows; 200001: chunks of 196 rows, the only ones long enough for the four-rows-in-flight loop at q = 4, whose 64 row
# lanes need more than 192) (2048 channels: 32 channel tiles)
BN_SHAPES = [(1, 4), (2, 8), (127, 20), (128, 20), (129, 16), (129, 36), (4096, 4), (4097, 4), (131072, 4), (131073, 4), (200001, 4), (3, 2048)]
BN_TWICE = ((131072, 4), (131073, 4))


@pytest.mark.parametrize("rows,c", BN_SHAPES)
@pytest.mark.parametrize("relu", [False, True])
def test_batchnorm_chunk_edges(backend, rows, c, relu):
    # two rows: xhat = +-(1 - eps / 2 var), and dx = gamma rstd (dy_0 - dy_1) / 2 * eps / (var + eps) is what is left of 1 - xhat^2 - six digits cancel
    # in fp32 whoever computes it (fp32 ATen: 4.5e-4 / 7.6e-4 of max |dx|), so this one case takes the derived bar like the ones below
    _bn_case(backend, rows, c, relu, 0.3, 1.7, twice=(rows, c) in BN_TWICE, derived=rows == 2)


# mean >> std: E[x^2] - E[x]^2 cancels unless the sums are taken about a pivot (bn_reduce_kernel: row 0).  The bar is derived from what the
# reference model's own fp32 ATen op does on the same inputs.
@pytest.mark.parametrize("rows,c", [s for s in BN_SHAPES if s[0] >= 127])
@pytest.mark.parametrize("mean,std", [(100.0, 1.0), (100.0, 0.01), (1.0, 0.01)])
def test_batchnorm_conditioning(backend, rows, c, mean, std):
    _bn_case(backend, rows, c, False, mean, std, derived=True)


@pytest.mark.parametrize("rows,c", [(1, 12), (130, 36)])
def test_batchnorm_segments(backend, rows, c):
    _bn_case(backend, rows, c, True, 0.3, 1.7, segments=3)


@pytest.mark.parametrize("sliced,fork", [(True, False), (False, True), (True, True)])
def test_batchnorm_fork_and_slices(backend, sliced, fork):
    """dx_add (the skip path's gradient, summed inside the backward kernel) and operands that are channel slices of wider rows (ld > c)"""
    _bn_case(backend, 129, 36, True, 0.3, 1.7, sliced=sliced, fork=fork)


@pytest.mark.parametrize("rows,c,segments,msg", [(2, 2048, 64, "exceeds LFDM_BN_TICKETS"), (5, 6, 1, "channels % 4 == 0"), (5, 2052, 1, "<= 2048")])
def test_batchnorm_refusals(backend, rows, c, segments, msg):
    dev = backend
    x, dy = rnd(rows * segments, c, seed=1).to(dev), rnd(rows * segments, c, seed=2).to(dev)
    g, b, rm, rv = torch.ones(c, device=dev), torch.zeros(c, device=dev), torch.zeros(c, device=dev), torch.ones(c, device=dev)
    y, dx, stat, dg, db = _nan(x.shape, dev), _nan(x.shape, dev), _nan((segments, 2, c), dev), _nan((c,), dev), _nan((c,), dev)
    ws = _nan((1 << 20,), dev)
    tk = ops._p(L._state(torch.device(dev))["tickets"])
    with pytest.raises(RuntimeError, match=msg):
        _call("lfdm_batchnorm_train_fwd_cl_f32", ops._p(x), ops._p(y), rows, c, segments, c, c, ops._p(g), ops._p(b), ops._p(rm), ops._p(rv), MOM,
              EPS, 1, ops._p(stat), ops._p(ws), 4 << 20, tk)
    stat0 = torch.zeros(segments, 2, c, device=dev)
    with pytest.raises(RuntimeError, match=msg):
        _call("lfdm_batchnorm_train_bwd_cl_f32", ops._p(x), ops._p(dy), ops._p(dx), rows, c, segments, c, c, c, None, 0, ops._p(g), ops._p(b),
              ops._p(stat0), 1, ops._p(dg), ops._p(db), ops._p(ws), 4 << 20, tk)
    for t in (y, dx, stat, dg, db):
        _untouched(t, "batchnorm (refused)")
    assert float(rm.abs().max()) == 0.0 and float((rv - 1).abs().max()) == 0.0
    _state_clean(dev, "batchnorm (refused)")


# ------------------------------------------------------------------------------------------------------------------------------------
# 7.  lfdm_blur_down_{fwd,bwd}_f32

# (scale, h, w): image smaller than the 13- / 5-tap filter | one pixel | the 29-tap filter on a 5-row image | ragged workgroups (17 x 300
# input pixels in the backward)
@pytest.mark.parametrize("scale,h,w", [(0.25, 3, 3), (0.5, 2, 3), (0.5, 1, 1), (0.125, 5, 40), (0.25, 17, 300)])
@pytest.mark.parametrize("rows4,affine", [(False, False), (True, True), (True, False), (False, True)])
def test_blur_down_edges(backend, scale, h, w, rows4, affine):
    dev = backend
    n, c, stride = 2, 3, int(1 / scale)
    x = rnd(n, c, h, w, seed=1).double().requires_grad_(True)
    weight = P.antialias_kernel(c, scale)
    sc = (rnd(c, seed=2).abs() + 0.5) if affine else None
    bi = rnd(c, seed=3) if affine else None
    ref = _antialias_ref(x, weight.double(), scale)
    if affine:
        ref = ref * sc.double().view(1, c, 1, 1) + bi.double().view(1, c, 1, 1)
    dy = rnd(*ref.shape, seed=4)
    ref.backward(dy.double())
    # a strided input: the 3 real channels of 4-channel rows
    x4 = torch.zeros(n, h, w, 4)
    x4[..., :c] = x.detach().float().permute(0, 2, 3, 1)
    xd = x4.to(dev).permute(0, 3, 1, 2)[:, :c]
    wgt = weight.reshape(c, weight.shape[-2], weight.shape[-1]).contiguous().to(dev)
    pad_lo, pad_hi, ho, wo = L.blur_geometry(h, w, wgt.shape[-1], stride)
    assert (ho, wo) == tuple(ref.shape[2:])
    out = _nan((n, ho, wo, 4), dev).permute(0, 3, 1, 2) if rows4 else _nan((n, c, ho, wo), dev)
    scd, bid = (None, None) if not affine else (sc.to(dev), bi.to(dev))
    p = L._blur_params(xd, xd.shape, wgt, stride, pad_lo, pad_hi, out, out.shape[1], scd, bid)
    p.x, p.out = xd.data_ptr(), out.data_ptr()
    _call("lfdm_blur_down_fwd_f32", C.byref(p))
    _written(out, "blur_down out")
    if rows4:
        assert float(out[:, c:].abs().max()) == 0.0, "blur_down: the fourth channel of the rows is written as zero"
    assert_close(out[:, :c].cpu(), ref.detach(), 1e-5, "lfdm_blur_down_fwd_f32 out")
    dyd = torch.zeros_like(out)
    dyd[:, :c] = dy.to(dev)
    dx = _nan((n, c, h, w), dev)
    p = L._blur_params(dx, (n, c, h, w), wgt, stride, pad_lo, pad_hi, dyd, dyd.shape[1], scd, None)
    p.dy, p.dx = dyd.data_ptr(), dx.data_ptr()
    _call("lfdm_blur_down_bwd_f32", C.byref(p))
    _written(dx, "blur_down dx")
    _scaled(dx, x.grad, "lfdm_blur_down_bwd_f32 dx", tol=1e-5)


def test_blur_down_refuses_filter_larger_than_padded_input(backend):
    dev = backend
    n, c, h, w = 1, 3, 3, 3
    wgt = P.antialias_kernel(c, 0.25)
    assert wgt.shape[-1] == 13
    x, wgt = rnd(n, c, h, w, seed=1).to(dev), wgt.reshape(c, 13, 13).contiguous().to(dev)
    out, dx = _nan((n, c, 1, 1), dev), _nan((n, c, h, w), dev)
    p = L._blur_params(x, x.shape, wgt, 4, 4, 4, out, c, None, None)               # 3 + 4 + 4 < 13
    p.x, p.out = x.data_ptr(), out.data_ptr()
    with pytest.raises(RuntimeError, match="kernel larger than the padded input"):
        _call("lfdm_blur_down_fwd_f32", C.byref(p))
    p = L._blur_params(dx, x.shape, wgt, 4, 4, 4, out, c, None, None)
    p.dy, p.dx = x.data_ptr(), dx.data_ptr()
    with pytest.raises(RuntimeError, match="kernel larger than the padded input"):
        _call("lfdm_blur_down_bwd_f32", C.byref(p))
    _untouched(out, "blur_down (refused)")
    _untouched(dx, "blur_down_bwd (refused)")


# ------------------------------------------------------------------------------------------------------------------------------------
# 8.  lfdm_grid_sample_{fwd,bwd}_f32

# (reflection, amp, h, w, ho, wo): reflected once or twice | dozens of times | a 1 x 1 image, reflected and zero-padded | 700 output pixels of a
# 2 x 300 image (ragged workgroups) | the identity
@pytest.mark.parametrize("reflection,amp,h,w,ho,wo", [(True, 3.0, 9, 11, 17, 19), (True, 40.0, 5, 4, 17, 19), (True, 3.0, 1, 1, 3, 3),
                                                      (False, 1.5, 1, 1, 3, 3), (False, 0.5, 2, 300, 1, 700), (True, 0.0, 4, 4, 4, 4)])
@pytest.mark.parametrize("n_div", [1, 2, 3])
def test_grid_sample_edges(backend, reflection, amp, h, w, ho, wo, n_div):
    dev = backend
    nb, c = 2, 3
    n = nb * n_div
    x = rnd(nb, c, h, w, seed=1)
    grid = _flow(n, ho, wo, 2, amp=amp).double().requires_grad_(not reflection)
    ref = F.grid_sample(x.double().repeat_interleave(n_div, 0), grid, padding_mode="reflection" if reflection else "zeros", align_corners=False)
    xd, gd = x.to(dev), grid.detach().float().to(dev)
    out = _nan((n, c, ho, wo), dev)
    p = L._gs_params(xd, gd, out, n_div, 1 if reflection else 0)
    p.out = out.data_ptr()
    _call("lfdm_grid_sample_fwd_f32", C.byref(p))
    _written(out, "grid_sample out")
    assert_close(out.cpu(), ref.detach(), TOL, "lfdm_grid_sample_fwd_f32 out")
    if reflection:
        return
    _sample_positions_clear(grid, h, w, "grid_sample", resize=False)
    dy = rnd(*ref.shape, seed=3)
    ref.backward(dy.double())
    dyd, dgrid = dy.to(dev), _nan((n, ho, wo, 2), dev)
    p = L._gs_params(xd, gd, dyd, n_div, 0)
    p.dout, p.dgrid = dyd.data_ptr(), dgrid.data_ptr()
    _call("lfdm_grid_sample_bwd_f32", C.byref(p))
    _written(dgrid, "grid_sample dgrid")
    _scaled(dgrid, grid.grad, "lfdm_grid_sample_bwd_f32 dgrid")


# ------------------------------------------------------------------------------------------------------------------------------------
# 9.  lfdm_svd2x2_sym_f32 / lfdm_svd2x2_sym_bwd_f32: one matrix, one matrix beyond a workgroup

@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("grads", ["gu", "gs", "both"])
def test_svd2x2_sym_bwd_edges(backend, n, grads):
    dev = backend
    g = torch.Generator().manual_seed(1)
    th, e0, e1 = torch.rand(n, generator=g) * 6.28, torch.rand(n, generator=g), torch.rand(n, generator=g)
    rot = torch.stack((th.cos(), -th.sin(), th.sin(), th.cos()), -1).view(n, 2, 2)
    a32 = rot @ torch.diag_embed(torch.stack((1 + e0, 0.2 + 0.1 * e1), -1)) @ rot.transpose(1, 2)
    a32 = 0.5 * (a32 + a32.transpose(1, 2))
    a = a32.double().requires_grad_(True)
    u, s, _ = torch.svd(a)
    gap = (s.detach()[:, 0] - s.detach()[:, 1]) / s.detach()[:, 0]
    assert float(gap.min()) > 0.3, "the case does not hold its premise (a healthy singular-value gap in every matrix)"
    gu, gs = (rnd(n, 2, 2, seed=2) if grads != "gs" else None), (rnd(n, 2, seed=3) if grads != "gu" else None)
    loss = 0
    if gu is not None:
        loss = loss + (u * gu.double()).sum()
    if gs is not None:
        loss = loss + (s * gs.double()).sum()
    loss.backward()
    abc = torch.stack((a32[:, 0, 0], a32[:, 0, 1], a32[:, 1, 1]), -1).contiguous().to(dev)
    ud, sd, ga = _nan((n, 2, 2), dev), _nan((n, 2), dev), _nan((n, 2, 2), dev)
    _call("lfdm_svd2x2_sym_f32", ops._p(abc), n, ops._p(ud), ops._p(sd))
    _written(ud, "svd u")
    _written(sd, "svd s")
    assert_close(ud.cpu(), u.detach(), 1e-4, "lfdm_svd2x2_sym_f32 u")
    assert_close(sd.cpu(), s.detach(), 1e-4, "lfdm_svd2x2_sym_f32 s")
    gud, gsd = None if gu is None else gu.to(dev), None if gs is None else gs.to(dev)
    _call("lfdm_svd2x2_sym_bwd_f32", ops._p(ud), ops._p(sd), ops._p(gud), ops._p(gsd), ops._p(ga), n)
    _written(ga, "svd backward")
    _scaled(ga, a.grad, "lfdm_svd2x2_sym_bwd_f32 ga", tol=5e-4)


# ------------------------------------------------------------------------------------------------------------------------------------
# 10.  lfdm_pool2_cl_f32, lfdm_relu_bwd_f32, lfdm_l1_mean_{fwd,bwd}_f32, lfdm_im2col_cl_f32

POOL_AVG, POOL_SUM, POOL_UP, POOL_UP_QUARTER, POOL_MAX, POOL_MAX_BWD = range(6)


def _pool(dev, x, aux, n, h, w, mode):
    """(h, w): the fine resolution"""
    c = x.shape[1]
    rows = n * h * w if mode in (POOL_UP, POOL_UP_QUARTER, POOL_MAX_BWD) else n * (h // 2) * (w // 2)
    out = _nan((rows, c), dev)
    _call("lfdm_pool2_cl_f32", ops._p(x), ops._p(aux), ops._p(out), n, h, w, c, mode)
    _written(out, "pool2 mode %d" % mode)
    return out


# (n, c, h, w) at the fine resolution: one window per channel quad | one row of windows | one column | three images of 3 x 5 windows
@pytest.mark.parametrize("n,c,h,w", [(1, 4, 2, 2), (1, 8, 2, 6), (1, 8, 6, 2), (3, 12, 6, 10)])
@pytest.mark.parametrize("kind", ["avg", "max", "up"])
def test_pool2_edges(backend, kind, n, c, h, w):
    dev = backend
    if kind == "up":
        x = rnd(n, c, h // 2, w // 2, seed=1)
    elif kind == "avg":
        x = rnd(n, c, h, w, seed=1)
    else:
        # window i holds the 0 / 1 pattern i % 16 in row-major order: ties in every position, windows of four equal values; the FIRST
        # maximum takes the gradient
        wi = torch.arange(n * c * (h // 2) * (w // 2)).view(n, c, h // 2, w // 2)
        x = torch.zeros(n, c, h, w)
        for t in range(4):
            x[:, :, t // 2::2, t % 2::2] = ((wi >> t) & 1).float()
        x = x + rnd(n, c, 1, 1, seed=1)
    x = x.double().requires_grad_(True)
    ref = {"avg": lambda: F.avg_pool2d(x, 2), "max": lambda: F.max_pool2d(x, 2), "up": lambda: F.interpolate(x, scale_factor=2)}[kind]()
    dy = rnd(*ref.shape, seed=2)
    ref.backward(dy.double())
    xr, dr = _rows(x.detach().float()).to(dev), _rows(dy).to(dev)
    if kind == "up":
        out, dx = _pool(dev, xr, None, n, h, w, POOL_UP), _pool(dev, dr, None, n, h, w, POOL_SUM)
        ho, wo, hi, wi_ = h, w, h // 2, w // 2
    else:
        out = _pool(dev, xr, None, n, h, w, POOL_AVG if kind == "avg" else POOL_MAX)
        dx = _pool(dev, dr, None, n, h, w, POOL_UP_QUARTER) if kind == "avg" else _pool(dev, xr, dr, n, h, w, POOL_MAX_BWD)
        ho, wo, hi, wi_ = h // 2, w // 2, h, w
    assert_close(_unrows(out.cpu(), n, ho, wo), ref.detach(), 1e-6, "lfdm_pool2_cl_f32 %s" % kind)
    assert_close(_unrows(dx.cpu(), n, hi, wi_), x.grad, 1e-6, "lfdm_pool2_cl_f32 %s backward" % kind)


@pytest.mark.parametrize("n", [4, 4 * 257])
def test_relu_bwd_exact(backend, n):
    dev = backend
    y, dy = rnd(n, seed=1), rnd(n, seed=2)
    y[0::5] = 0.0
    y[1::5] = -0.0
    yd, dyd, out = y.to(dev), dy.to(dev), _nan((n,), dev)
    _call("lfdm_relu_bwd_f32", ops._p(yd), ops._p(dyd), ops._p(out), n)
    _written(out, "relu_bwd")
    assert torch.equal(out.cpu(), torch.where(y > 0, dy, torch.zeros(()))), "relu_bwd: not dy where y > 0 and +0 elsewhere"


# one float4 | two workgroups of 2048 float4, the second with one | one float4 beyond the cap of 1024 workgroups
@pytest.mark.parametrize("n", [4, 4 * 2049, 4 * (1024 * 2048 + 1)])
def test_l1_mean_edges(backend, n):
    dev = backend
    x, y = rnd(n, seed=1), rnd(n, seed=2)
    x[1::3] = y[1::3]                                                               # equal elements: gradient exactly 0
    weight, gout = 10.0, torch.tensor([0.7])
    ref = weight * (x.double() - y.double()).abs().mean()
    want_dx = torch.sign(x.double() - y.double()) * (weight * 0.7 / n)
    xd, yd, gd = x.to(dev), y.to(dev), gout.to(dev)
    st = L._state(torch.device(dev))

    def run():
        out, dx, ws = _nan((1,), dev), _nan((n,), dev), _nan((2048,), dev)
        _call("lfdm_l1_mean_fwd_f32", ops._p(xd), ops._p(yd), n, weight, ops._p(out), ops._p(ws), 8192, C.c_void_p(st["amax"].data_ptr() + 8))
        _call("lfdm_l1_mean_bwd_f32", ops._p(xd), ops._p(yd), n, weight, ops._p(gd), ops._p(dx))
        _state_clean(dev, "l1_mean")
        return out, dx

    out, dx = run()
    _written(out, "l1_mean")
    _written(dx, "l1_mean dx")
    assert abs(float(out) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), "l1_mean: %.9g against %.9g" % (float(out), float(ref))
    assert float(dx.cpu()[1::3].abs().max()) == 0.0, "l1_mean: x == y has the gradient 0"
    _scaled(dx, want_dx, "lfdm_l1_mean_bwd_f32 dx")
    _same_bits((out, dx), run(), "l1_mean")


# (c, h, w, k, pad, ldx): one pixel under a 7 x 7 window | no padding, rows of 20 floats | 1 x 1 | 5 x 5, three float4 per tap
@pytest.mark.parametrize("c,h,w,k,pad,ldx", [(4, 1, 1, 7, 3, 4), (16, 3, 3, 3, 0, 20), (8, 5, 2, 1, 0, 8), (12, 4, 6, 5, 2, 12)])
def test_im2col_exact(backend, c, h, w, k, pad, ldx):
    dev = backend
    n = 2
    x = rnd(n, c, h, w, seed=1)
    hq, wq = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    want = F.unfold(x, k, padding=pad).view(n, c, k * k, hq * wq).permute(0, 3, 2, 1).reshape(n * hq * wq, k * k * c)
    xd, _ = _wide(_rows(x), ldx, dev, fill=1e30)
    out = _nan((n * hq * wq, k * k * c), dev)
    _call("lfdm_im2col_cl_f32", ops._p(xd), ops._p(out), n, h, w, c, ldx, k, pad)
    _written(out, "im2col")
    assert torch.equal(out.cpu(), want), "im2col: not F.unfold in (pixel, tap, channel) order"


def test_im2col_refuses_20_channels(backend):
    dev = backend
    x, out = rnd(2 * 3 * 3, 20, seed=1).to(dev), _nan((2 * 3 * 3, 9 * 20), dev)
    with pytest.raises(RuntimeError, match="im2col_cl: channels % 4 == 0 and <= 16"):
        _call("lfdm_im2col_cl_f32", ops._p(x), ops._p(out), 2, 3, 3, 20, 20, 3, 1)
    _untouched(out, "im2col (refused)")


# ------------------------------------------------------------------------------------------------------------------------------------
# 11.  lfdm_lfae_region_stats_f32 against the closed formula (region_predictor.py:16-26, 60-96)

def _coordinate_grid(h, w):
    ys, xs = torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64)
    gy, gx = torch.meshgrid(2 * (ys / (h - 1)) - 1, 2 * (xs / (w - 1)) - 1, indexing="ij")
    return torch.stack((gx, gy), -1)                      # (h, w, 2)


# (n, k, h, w, ld): four pixels, one region, rows of 4 | 600 pixels: three pixel slots per thread, the third ragged | the shipped 64 x 64 = all 16
# slots | 255 pixels: one slot, one thread idle | 33 regions | 4095 of 4096 pixels, rows of one float
@pytest.mark.parametrize("n,k,h,w,ld", [(1, 1, 2, 2, 4), (2, 3, 2, 300, 5), (1, 10, 64, 64, 12), (2, 2, 15, 17, 2), (1, 33, 16, 16, 36),
                                        (1, 1, 63, 65, 1)])
@pytest.mark.parametrize("temperature", [0.1, 1.0])
def test_region_stats_edges(backend, n, k, h, w, ld, temperature):
    dev = backend
    logits = rnd(n * h * w, ld, seed=1)
    t32 = float(torch.tensor(temperature, dtype=torch.float32))
    heat = (logits[:, :k].double() / t32).view(n, h * w, k).softmax(dim=1).permute(0, 2, 1)            # (n, k, hw)
    grid = _coordinate_grid(h, w).view(1, 1, h * w, 2)
    shift = (heat.unsqueeze(-1) * grid).sum(2)                                                       # (n, k, 2)
    d = grid - shift.unsqueeze(2)
    covar = (heat.view(n, k, h * w, 1, 1) * (d.unsqueeze(-1) * d.unsqueeze(-2))).sum(2)              # (n, k, 2, 2)
    got = dict(heat=_nan((n, k, h, w), dev), shift=_nan((n, k, 2), dev), covar=_nan((n, k, 2, 2), dev), affine=_nan((n, k, 2, 2), dev),
               u=_nan((n * k, 2, 2), dev), d=_nan((n * k, 2, 2), dev))
    ldev = logits.to(dev)
    _call("lfdm_lfae_region_stats_f32", ops._p(ldev), ld, n, k, h, w, temperature, *[ops._p(got[key]) for key in
                                                                                           ("heat", "shift", "covar", "affine", "u", "d")])
    for key, t in got.items():
        _written(t, "region_stats " + key)
    got = {key: t.cpu() for key, t in got.items()}
    assert_close(got["heat"].view(n, k, h * w), heat, TOL, "lfdm_lfae_region_stats_f32 heatmap")
    assert_close(got["shift"], shift, TOL, "lfdm_lfae_region_stats_f32 shift")
    assert_close(got["covar"], covar, TOL, "lfdm_lfae_region_stats_f32 covar")
    af = got["affine"].double()
    assert_close(af @ af.transpose(-1, -2), covar, TOL, "lfdm_lfae_region_stats_f32 affine @ affine^T")
    u, dd = got["u"].view(n, k, 2, 2), got["d"].view(n, k, 2, 2)
    assert float(dd[..., 0, 1].abs().max()) == 0.0 and float(dd[..., 1, 0].abs().max()) == 0.0
    assert torch.equal(got["affine"], u * torch.stack((dd[..., 0, 0], dd[..., 1, 1]), -1).unsqueeze(-2)), "affine is u * sqrt(s) by columns"
    assert_close(u.double() @ u.double().transpose(-1, -2), torch.eye(2, dtype=torch.float64).expand(n, k, 2, 2), TOL, "region_stats u u^T")
    ev = torch.linalg.eigvalsh(covar).flip(-1)
    assert_close(torch.stack((dd[..., 0, 0], dd[..., 1, 1]), -1).double() ** 2, ev, TOL, "lfdm_lfae_region_stats_f32 d^2")


@pytest.mark.parametrize("h,w", [(64, 65), (1, 8)])
def test_region_stats_refusals(backend, h, w):
    dev = backend
    n, k = 1, 2
    logits = rnd(n * h * w, 4, seed=1).to(dev)
    outs = [_nan((n, k, h, w), dev), _nan((n, k, 2), dev), _nan((n, k, 2, 2), dev), _nan((n, k, 2, 2), dev), _nan((n * k, 2, 2), dev),
            _nan((n * k, 2, 2), dev)]
    with pytest.raises(RuntimeError, match="lfae_region_stats: bad arguments"):
        _call("lfdm_lfae_region_stats_f32", ops._p(logits), 4, n, k, h, w, 0.1, *[ops._p(t) for t in outs])
    for t in outs:
        _untouched(t, "region_stats (refused)")


# ------------------------------------------------------------------------------------------------------------------------------------
# 12.  lfdm_lfae_motion_inputs_f32 + lfdm_lfae_motion_combine_f32 against the closed formula (pixelwise_flow_predictor.py:48-128)

def _elementwise(got, ref, what):
    """coordinates that a homography throws far outside dwarf the others: every element against its own magnitude"""
    got, ref = got.double().cpu(), ref.double()
    err = ((got - ref).abs() / ref.abs().clamp(min=1.0)).max()
    assert float(err) <= TOL, "%s: max error relative to max(1, |ref|) %.3e (tol %.1e)" % (what, float(err), TOL)


def _spd(n, k, seed):
    l = rnd(n, k, 2, 2, seed=seed) * 0.3
    return l @ l.transpose(-1, -2) + 0.02 * torch.eye(2)


# (b, frames, k, h, w, covar, affine, bg): one region on four pixels | every branch on a ragged image | K = 32 | 600 pixels, fixed variance |
# the shipped resolution
MOTION_CASES = [(1, 1, 1, 2, 2, False, False, False), (2, 3, 5, 15, 17, True, True, True), (1, 2, 32, 16, 16, True, False, True),
                (1, 1, 10, 2, 300, False, True, False), (2, 1, 3, 64, 64, True, True, True)]


@pytest.mark.parametrize("b,frames,k,h,w,use_covar,use_affine,use_bg", MOTION_CASES)
def test_motion_inputs_and_combine_edges(backend, b, frames, k, h, w, use_covar, use_affine, use_bg):
    dev = backend
    n, hw, region_var = b * frames, h * w, 0.01
    img = rnd(b, 3, h, w, seed=1).abs()
    dsh, ssh = rnd(n, k, 2, seed=2) * 0.4, rnd(b, k, 2, seed=3) * 0.4
    dcv, scv = (_spd(n, k, 4), _spd(b, k, 5)) if use_covar else (None, None)
    daf, saf = (torch.eye(2) + 0.3 * rnd(n, k, 2, 2, seed=6), torch.eye(2) + 0.3 * rnd(b, k, 2, 2, seed=7)) if use_affine else (None, None)
    bg = None
    if use_bg:
        bg = torch.eye(3).repeat(n, 1, 1) + 0.05 * rnd(n, 3, 3, seed=8)
        bg[-1] = torch.tensor([[1.0, 0.2, 3.0], [0.1, 1.0, 3.0], [0.0, 0.0, 1e-6]])        # coordinates ~1e6: every tap far outside the image
    grid = _coordinate_grid(h, w)                                                          # (h, w, 2)
    rep = lambda t: t.double().repeat_interleave(frames, 0)                                # source (b, ...) -> per frame (n, ...)
    dd = grid.view(1, 1, h, w, 2) - dsh.double().view(n, k, 1, 1, 2)
    de = grid.view(1, 1, h, w, 2) - rep(ssh).view(n, k, 1, 1, 2)
    if use_covar:
        quad = lambda v, cv: (v.unsqueeze(-2) @ torch.inverse(cv.double()).view(n, k, 1, 1, 2, 2) @ v.unsqueeze(-1)).squeeze(-1).squeeze(-1)
        heat = torch.exp(-0.5 * quad(dd, dcv)) - torch.exp(-0.5 * quad(de, rep(scv)))
    else:
        rv32 = float(torch.tensor(region_var, dtype=torch.float32))
        heat = torch.exp(-0.5 * (dd ** 2).sum(-1) / rv32) - torch.exp(-0.5 * (de ** 2).sum(-1) / rv32)
    motion = dd
    if use_affine:
        aff = rep(saf) @ torch.inverse(daf.double())
        assert float(aff[..., 0, 0].abs().min()) > 1e-3, "the case does not hold its premise (the sign of affine[0][0] is beyond rounding)"
        aff = aff * torch.sign(aff[..., 0:1, 0:1])                                         # revert_axis_swap
        motion = (aff.view(n, k, 1, 1, 2, 2) @ dd.unsqueeze(-1)).squeeze(-1)
    motion = motion + rep(ssh).view(n, k, 1, 1, 2)
    back = grid.view(1, h, w, 2).expand(n, h, w, 2)
    if use_bg:
        hom = (bg.double().view(n, 1, 1, 3, 3) @ torch.cat((back, torch.ones(n, h, w, 1, dtype=torch.float64)), -1).unsqueeze(-1)).squeeze(-1)
        back = hom[..., :2] / hom[..., 2:]
    sparse = torch.cat((back.unsqueeze(1), motion), 1)                                     # (n, k + 1, h, w, 2)
    heat = torch.cat((torch.zeros(n, 1, h, w, dtype=torch.float64), heat), 1)
    deformed = F.grid_sample(rep(img).unsqueeze(1).expand(n, k + 1, 3, h, w).reshape(-1, 3, h, w), sparse.view(-1, h, w, 2), align_corners=False)
    want = torch.cat((heat.unsqueeze(2), deformed.view(n, k + 1, 3, h, w)), 2).permute(0, 3, 4, 1, 2).reshape(n * hw, 4 * (k + 1))
    if use_bg:
        assert float(deformed.view(n, k + 1, 3, hw)[-1, 0].abs().max()) == 0.0 and float(sparse[-1, 0].abs().max()) > 1e5

    used, ld = 4 * (k + 1), ops.round_up(4 * (k + 1), 32)
    rows, sp = _nan((n * hw, ld), dev), _nan((n, k + 1, h, w, 2), dev)
    held = [None if t is None else t.contiguous().to(dev) for t in (img, dsh, dcv, daf, ssh, scv, saf, bg)]
    _call("lfdm_lfae_motion_inputs_f32", *[ops._p(t) for t in held], region_var, 1, b, frames, k, h, w, ops._p(rows), ld, ops._p(sp))
    _written(rows, "motion_inputs rows")
    _written(sp, "motion_inputs sparse")
    assert float(rows[:, used:].abs().max()) == 0.0, "motion_inputs: the padding columns of a row are written as zero"
    assert ld > used
    _elementwise(sp, sparse, "lfdm_lfae_motion_inputs_f32 sparse")
    assert_close(rows[:, :used].cpu(), want, TOL, "lfdm_lfae_motion_inputs_f32 rows")

    # the tail, on the reference's sparse motions: logits x 4, one row with a logit of 80, with and without the occlusion column
    sp32 = sparse.float()
    for has_occ in (True, False):
        ldh = k + 1 + (1 if has_occ else 0) + 3
        heads = 4 * rnd(n * hw, ldh, seed=9)
        heads[hw // 2, k // 2] = 80.0
        mask = heads[:, :k + 1].double().softmax(dim=1).view(n, hw, k + 1)
        flow_ref = (mask.unsqueeze(-1) * sp32.double().view(n, k + 1, hw, 2).permute(0, 2, 1, 3)).sum(2)          # (n, hw, 2)
        flow, occ = _nan((n, h, w, 2), dev), _nan((n, 1, h, w), dev) if has_occ else None
        hd, spd = heads.to(dev), sp32.contiguous().to(dev)
        _call("lfdm_lfae_motion_combine_f32", ops._p(hd), ldh, ops._p(spd), n, k, hw, ops._p(flow), ops._p(occ))
        _written(flow, "motion_combine flow")
        _elementwise(flow.view(n, hw, 2), flow_ref, "lfdm_lfae_motion_combine_f32 flow")
        if has_occ:
            _written(occ, "motion_combine occlusion")
            assert_close(occ.view(n * hw).cpu(), torch.sigmoid(heads[:, k + 1].double()), TOL, "lfdm_lfae_motion_combine_f32 occlusion")


def test_motion_inputs_refuses_33_regions(backend):
    dev = backend
    b, frames, k, h, w = 1, 1, 33, 4, 4
    ld = 4 * (k + 1)
    img, dsh, ssh = rnd(b, 3, h, w, seed=1).to(dev), rnd(b, k, 2, seed=2).to(dev), rnd(b, k, 2, seed=3).to(dev)
    rows, sp = _nan((h * w, ld), dev), _nan((1, k + 1, h, w, 2), dev)
    with pytest.raises(RuntimeError, match="lfae_motion_inputs: bad arguments"):
        _call("lfdm_lfae_motion_inputs_f32", ops._p(img), ops._p(dsh), None, None, ops._p(ssh), None, None, None, 0.01, 0, b, frames, k, h, w,
              ops._p(rows), ld, ops._p(sp))
    _untouched(rows, "motion_inputs (refused)")
    _untouched(sp, "motion_inputs (refused)")
