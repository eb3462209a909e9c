"""Paired video metrics on the device: csrc/metrics.hip through ops.video_metrics / ops.flow_metrics / ops.psnr,
cvpr23_lfdm_amd.evaluate and tools/eval.py.  Kernel tests take the `backend` fixture: the x86 emulator build everywhere, the gfx950
build on the GPU.

Two references, both float64 and both written here: the window moments as a separable valid torch conv2d, and scikit-image's formula
with scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5) cropped by 5 pixels.  They agree to <= 1.4e-14 on every shape below, and
the same formula with fp32 moments is off by up to 4.3e-6, so the bars are: SSIM absolute 1e-10 (10^4 above the spread of correct fp64
evaluations, 10^4 below an fp32 kernel's error - an fp32 kernel does not pass), L1 and MSE relative 1e-10 (worst-case fp64 summation
error for N = C H W <= 3 * 2^16 terms: N 2^-53 = 2e-11), flow metrics relative 1e-10."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
from cvpr23_lfdm_amd import io_compat as IO

MEAN = (10.0, -7.5, 3.25)
SSIM_ABS = 1e-10
REL = 1e-10
C1, C2 = 0.01 ** 2, 0.03 ** 2
# (B, C, T, H, W): one valid pixel | odd sizes, rows not 16-byte aligned | one tile | several 16 x 32 tiles each way | headline | C = 1
SHAPES = [(2, 3, 3, 11, 11), (2, 3, 3, 13, 29), (2, 3, 3, 32, 32), (2, 3, 3, 48, 80), (2, 3, 2, 128, 128), (2, 1, 3, 16, 20)]
KINDS = ("noise", "smooth", "near", "edges")
DOMAINS = ("raw", "unit", "uint8")


def _mean(c):
    return MEAN[:c]


def _edge_values():
    """Every k / 255 in fp32 and its two neighbours, 0, 1, and values outside [0, 1] (tests/test_render.py's set)."""
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    return np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)),
                           np.array([0.0, 1.0, -0.0, -0.25, -1e-8, 1.0 + 1e-6, 1.5, -3.0, 7.0], np.float32)]).astype(np.float32)


def _pair(shape, kind, seed=0):
    """(a, b) fp32 videos.  noise: independent uniform pairs (SSIM about 0, may be negative); smooth: a bilinearly up-sampled 4 x 4 field
    + 1e-2 noise each (SSIM 0.9 - 0.99); near: b = a + 1e-3 noise; edges: values below 0 and above 1 with the edge values sown in."""
    g = torch.Generator().manual_seed(1000 * seed + sum(shape) + len(kind))
    b_, c, t, h, w = shape
    if kind == "noise":
        return torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if kind == "smooth":
        base = F.interpolate(torch.rand(b_ * c * t, 1, 4, 4, generator=g), size=(h, w), mode="bilinear", align_corners=False)
        base = base.reshape(b_, c, t, h, w)
        return base + 1e-2 * torch.randn(shape, generator=g), base + 1e-2 * torch.randn(shape, generator=g)
    if kind == "near":
        a = torch.rand(shape, generator=g)
        return a, a + 1e-3 * torch.randn(shape, generator=g)
    a = torch.randn(shape, generator=g) * 0.45 + 0.5
    b = a + 0.05 * torch.randn(shape, generator=g)
    e = torch.from_numpy(_edge_values())
    for v in (a, b):
        flat = v.reshape(-1)
        pos = torch.randperm(flat.numel(), generator=g)[:min(flat.numel() // 2, 2 * e.numel())]
        flat[pos] = e.repeat(math.ceil(pos.numel() / e.numel()))[:pos.numel()]
    return a.contiguous(), b.contiguous()


def _values(x, mean, domain):
    """The float64 values of a domain, restated on the host.  uint8 goes through io_compat.sample_img: the bytes the demo writes."""
    if domain == "raw":
        return x.double()
    if domain == "unit":
        add = torch.from_numpy(np.array(mean) / 255.0).view(1, -1, 1, 1, 1)
        return (x.double() + add).float().clamp(0, 1).double()
    out = torch.empty(x.shape, dtype=torch.float64)
    for b in range(x.shape[0]):
        for t in range(x.shape[2]):
            img = IO.sample_img(x[:, :, t], b, mean)          # (H, W, C) uint8
            out[b, :, t] = torch.from_numpy(img.astype(np.float64) / 255.0).permute(2, 0, 1)
    return out


def _window():
    x = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(x * x) / (2 * 1.5 ** 2))
    return g / g.sum()


def _ssim_from_moments(ma, mb, eaa, ebb, eab):
    va, vb, vab = eaa - ma * ma, ebb - mb * mb, eab - ma * mb
    return ((2 * ma * mb + C1) * (2 * vab + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2))


def _ref_conv(va, vb):
    """(B, T, 3) float64 [l1, mse, ssim]: window moments by a separable valid conv2d."""
    b, c, t, h, w = va.shape
    g = _window()
    blur = lambda v: F.conv2d(F.conv2d(v, g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1))
    xa = va.permute(0, 2, 1, 3, 4).reshape(-1, 1, h, w)
    xb = vb.permute(0, 2, 1, 3, 4).reshape(-1, 1, h, w)
    s = _ssim_from_moments(blur(xa), blur(xb), blur(xa * xa), blur(xb * xb), blur(xa * xb))
    d = va - vb
    return torch.stack((d.abs().mean(dim=(1, 3, 4)), (d * d).mean(dim=(1, 3, 4)), s.mean(dim=(1, 2, 3)).reshape(b, t, c).mean(dim=-1)), dim=-1)


def _ref_scipy(va, vb):
    """The same through scipy.ndimage.gaussian_filter cropped by 5 pixels: scikit-image's structural_similarity(gaussian_weights=True,
    use_sample_covariance=False, data_range=1)."""
    from scipy.ndimage import gaussian_filter
    a, b = va.numpy(), vb.numpy()
    blur = lambda v: gaussian_filter(v, sigma=(0, 0, 0, 1.5, 1.5), truncate=3.5)[..., 5:-5, 5:-5]
    s = _ssim_from_moments(blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b))
    d = a - b
    return torch.from_numpy(np.stack((np.abs(d).mean(axis=(1, 3, 4)), (d * d).mean(axis=(1, 3, 4)), s.mean(axis=(1, 3, 4))), axis=-1))


def _assert_table(got, want, what):
    got = got.cpu()
    assert got.dtype == torch.float64 and got.shape == want.shape, what
    for j, name in enumerate(("l1", "mse")):
        err = ((got[..., j] - want[..., j]).abs() / want[..., j].abs().clamp_min(1e-300)).max().item() if want[..., j].abs().max() > 0 \
            else got[..., j].abs().max().item()
        print("%s %s: worst relative error %.3e" % (what, name, err))
        assert err <= REL, (what, name, err)
    err = (got[..., 2] - want[..., 2]).abs().max().item()
    print("%s ssim: worst absolute error %.3e (range %.4f .. %.4f)" % (what, err, want[..., 2].min(), want[..., 2].max()))
    assert err <= SSIM_ABS, (what, err)


_ref_cache = {}


def _case(shape, kind):
    """The inputs of one (shape, kind) and, per domain, both references - computed once and shared."""
    key = (shape, kind)
    if key not in _ref_cache:
        a, b = _pair(shape, kind)
        mean = _mean(shape[1])
        refs = {}
        for domain in DOMAINS:
            va, vb = _values(a, mean, domain), _values(b, mean, domain)
            refs[domain] = (_ref_conv(va, vb), _ref_scipy(va, vb))
        _ref_cache[key] = (a, b, refs)
    return _ref_cache[key]


# ------------------------------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_video_metrics_match_both_references(backend, shape, kind):
    from cvpr23_lfdm_amd import ops
    a, b, refs = _case(shape, kind)
    for domain in DOMAINS:
        conv, sci = refs[domain]
        assert (conv - sci).abs().max().item() <= 1e-13          # the two references agree far inside the bars
        got = ops.video_metrics(a.to(backend), b.to(backend), mean=_mean(shape[1]), domain=domain)
        assert got.is_contiguous() and got.device.type == backend
        _assert_table(got, conv, "%s %s %s vs conv2d" % (shape, kind, domain))
        _assert_table(got, sci, "%s %s %s vs scipy" % (shape, kind, domain))


def test_reference_inputs_are_what_they_claim():
    shape = (2, 3, 3, 48, 80)
    ssim = {k: _case(shape, k)[2]["raw"][0][..., 2] for k in KINDS}
    assert ssim["noise"].abs().max() < 0.1 and 0.9 < ssim["smooth"].min() and ssim["smooth"].max() < 0.995 and ssim["near"].min() > 0.995
    a, b, _ = _case(shape, "edges")
    assert a.min() < 0 and a.max() > 1 and np.isin(_edge_values(), a.numpy()).all()


def test_uint8_domain_is_the_bytes_of_sample_img(backend):
    """Metrics of the uint8 domain = raw-domain metrics of the demo's bytes over 255 (bytes / 255 is not exact in fp32, so the raw call
    sees the fp32 neighbours: the comparison is to the fp64 reference of the bytes, inside the bars)."""
    from cvpr23_lfdm_amd import ops
    shape = (2, 3, 3, 13, 29)
    a, b, _ = _case(shape, "edges")
    va, vb = _values(a, MEAN, "uint8"), _values(b, MEAN, "uint8")
    assert set(np.unique((va * 255).round().numpy())) <= set(range(256)) and va.min() == 0 and va.max() == 1
    _assert_table(ops.video_metrics(a.to(backend), b.to(backend), mean=MEAN, domain="uint8"), _ref_conv(va, vb), "uint8 bytes")


# ------------------------------------------------------------------------------------------ 2. exact cases
@pytest.mark.parametrize("domain", DOMAINS)
def test_identical_operands_are_exact(backend, domain):
    from cvpr23_lfdm_amd import ops
    for shape in ((2, 3, 3, 13, 29), (1, 3, 2, 48, 80)):
        a = _pair(shape, "edges", seed=3)[0].to(backend)
        got = ops.video_metrics(a, a, mean=MEAN, domain=domain)
        assert torch.equal(got[..., 0], torch.zeros_like(got[..., 0])) and torch.equal(got[..., 1], torch.zeros_like(got[..., 1]))
        assert torch.equal(got[..., 2], torch.ones_like(got[..., 2]))
        p = ops.psnr(got[..., 1])
        assert p.shape == got.shape[:2] and torch.isinf(p).all() and (p > 0).all()


def test_constant_frames(backend):
    from cvpr23_lfdm_amd import ops
    p, q = 0.3, 0.55
    shape = (1, 3, 2, 20, 37)
    a, b = torch.full(shape, p), torch.full(shape, q)
    pd, qd = float(np.float32(p)), float(np.float32(q))
    got = ops.video_metrics(a.to(backend), b.to(backend), mean=(0, 0, 0), domain="raw").cpu()
    want = torch.tensor([abs(pd - qd), (pd - qd) ** 2, (2 * pd * qd + C1) / (pd * pd + qd * qd + C1)], dtype=torch.float64).expand(1, 2, 3)
    _assert_table(got, want, "constant frames")


def test_psnr(backend):
    from cvpr23_lfdm_amd import ops
    mse = torch.tensor([[1.0, 0.25, 0.0], [1e-6, 3.7e-3, 4.0]], dtype=torch.float64)
    got = ops.psnr(mse.to(backend)).cpu()
    assert got.dtype == torch.float64 and got.shape == mse.shape and got[0, 2] == math.inf and got[0, 0] == 0.0
    want = 10 * torch.log10(1 / mse)
    fin = torch.isfinite(want)
    assert ((got[fin] - want[fin]).abs() <= 1e-12 * want[fin].abs().clamp_min(1.0)).all()          # two ~1-ulp fp64 operations
    with pytest.raises(TypeError):
        ops.psnr(mse.float().to(backend))


# ------------------------------------------------------------------------------------------ 3. determinism and independence
@pytest.mark.parametrize("hw", [(13, 29), (48, 80)])
def test_deterministic_and_independent_of_the_batch(backend, hw):
    from cvpr23_lfdm_amd import ops
    shape = (3, 3, 4) + hw
    a, b = (v.to(backend) for v in _pair(shape, "smooth", seed=5))
    for domain in ("raw", "uint8"):
        kw = dict(mean=MEAN, domain=domain)
        got = ops.video_metrics(a, b, **kw)
        assert torch.equal(got, ops.video_metrics(a, b, **kw))
        for i in range(3):
            for f in range(4):
                one = ops.video_metrics(a[i:i + 1, :, f:f + 1], b[i:i + 1, :, f:f + 1], **kw)          # strided views: copied by the op
                assert torch.equal(one[0, 0], got[i, f]), (domain, i, f)
        back = ops.video_metrics(b, a, **kw)
        assert torch.equal(back[..., :2], got[..., :2])
        assert (back[..., 2] - got[..., 2]).abs().max().item() <= SSIM_ABS


# ------------------------------------------------------------------------------------------ 4. flow metrics
def _flow_pair(b, t, s, seed):
    g = torch.Generator().manual_seed(seed)
    lat_a = torch.randn(b, 3, t, s, s, generator=g).clamp(-1.3, 1.3)
    lat_b = lat_a + 0.1 * torch.randn(b, 3, t, s, s, generator=g)
    return lat_a, lat_b, torch.rand(b, 1, t, s, s, generator=g), torch.rand(b, 1, t, s, s, generator=g)


@pytest.mark.parametrize("s", [4, 8, 32])
def test_flow_metrics(backend, s):
    from cvpr23_lfdm_amd import ops
    b, t = 2, 3
    lat_a, lat_b, ca, cb = (v.to(backend) for v in _flow_pair(b, t, s, 40 + s))
    d = lat_a[:, :2].double().cpu() - lat_b[:, :2].double().cpu()
    epe = torch.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2).mean(dim=(2, 3))
    occ = (ca.double().cpu() - cb.double().cpu()).abs().mean(dim=(1, 3, 4))
    view = ops.flow_metrics(lat_a[:, :2], lat_b[:, :2], ca, cb)                    # channel views of the latents: batch stride 3 T s s
    assert view.dtype == torch.float64 and tuple(view.shape) == (b, t, 2) and view.is_contiguous()
    copy = ops.flow_metrics(lat_a[:, :2].contiguous(), lat_b[:, :2].contiguous(), ca, cb)
    mixed = ops.flow_metrics(lat_a[:, :2], lat_b[:, :2].contiguous(), ca, cb)
    assert torch.equal(view, copy) and torch.equal(view, mixed) and torch.equal(view, ops.flow_metrics(lat_a[:, :2], lat_b[:, :2], ca, cb))
    for name, got, want in (("epe", view[..., 0].cpu(), epe), ("occ", view[..., 1].cpu(), occ)):
        err = ((got - want).abs() / want).max().item()
        print("flow s=%d %s: worst relative error %.3e" % (s, name, err))
        assert err <= REL, (name, err)
    bare = ops.flow_metrics(lat_a[:, :2], lat_b[:, :2])
    assert torch.equal(bare[..., 0], view[..., 0]) and torch.equal(bare[..., 1], torch.zeros_like(bare[..., 1]))
    one = ops.flow_metrics(lat_a[1:2, :2, 2:3], lat_b[1:2, :2, 2:3], ca[1:2, :, 2:3], cb[1:2, :, 2:3])
    assert torch.equal(one[0, 0], view[1, 2])
    same = ops.flow_metrics(lat_a[:, :2], lat_a[:, :2], ca, ca)
    assert torch.equal(same, torch.zeros_like(same))
    from cvpr23_lfdm_amd import evaluate as E
    acc = E.FlowAccumulator().update(view[:1]).update(view[1:])
    r, both = acc.result(), E.compare_flows(lat_a[:, :2], lat_b[:, :2], ca, cb)
    assert set(both) == {"table"} and torch.equal(both["table"], view)
    assert r == both["summary"] or all(abs(r[k] - both["summary"][k]) <= 1e-12 * abs(r[k]) for k in r)
    assert r["frames"] == b * t and r["videos"] == b and abs(r["epe"] - epe.mean().item()) <= REL * r["epe"]
    assert abs(r["occlusion_error"] - occ.mean().item()) <= REL * r["occlusion_error"]
    with pytest.raises(RuntimeError, match="nothing has been accumulated"):
        E.FlowAccumulator().result()
    with pytest.raises(ValueError, match="float64"):
        E.FlowAccumulator().update(view.float())


# ------------------------------------------------------------------------------------------ 5. validation
def test_ops_refuse_bad_arguments(backend, monkeypatch):
    from cvpr23_lfdm_amd import _native, ops
    lib = _native.library()

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched before the arguments were checked")
    for name in ("lfdm_video_metrics", "lfdm_flow_metrics"):
        monkeypatch.setattr(lib, name, no_launch)
    v = torch.zeros(1, 3, 2, 16, 16).to(backend)
    with pytest.raises(ValueError, match=r"at least 11.*\(1, 3, 2, 10, 16\)"):
        ops.video_metrics(v[:, :, :, :10], v[:, :, :, :10])
    with pytest.raises(ValueError, match=r"at least 11"):
        ops.video_metrics(v[..., :10], v[..., :10])
    with pytest.raises(ValueError, match=r"one shape.*\(1, 3, 2, 16, 16\).*\(1, 3, 1, 16, 16\)"):
        ops.video_metrics(v, v[:, :, :1])
    with pytest.raises(ValueError, match="one shape"):
        ops.video_metrics(v[0], v[0])
    with pytest.raises(TypeError, match="float32"):
        ops.video_metrics(v.double(), v)
    with pytest.raises(TypeError, match="float32"):
        ops.video_metrics(v, v.half())
    with pytest.raises(ValueError, match="unknown domain 'srgb'"):
        ops.video_metrics(v, v, domain="srgb")
    with pytest.raises(ValueError, match="mean has 2 values for 3 channels"):
        ops.video_metrics(v, v, mean=(0, 0))
    with pytest.raises(ValueError, match="1 <= C <= 4"):
        ops.video_metrics(torch.zeros(1, 5, 1, 16, 16).to(backend), torch.zeros(1, 5, 1, 16, 16).to(backend), mean=(0,) * 5)
    with pytest.raises(ValueError, match="out must be"):
        ops.video_metrics(v, v, out=torch.zeros(1, 2, 3).to(backend))
    g = torch.zeros(2, 2, 3, 8, 8).to(backend)
    c = torch.zeros(2, 1, 3, 8, 8).to(backend)
    with pytest.raises(ValueError, match="both confidences or neither"):
        ops.flow_metrics(g, g, c)
    with pytest.raises(ValueError, match="one shape"):
        ops.flow_metrics(g, g[:1])
    with pytest.raises(ValueError, match=r"\(B, 2, T, s, s\)"):
        ops.flow_metrics(torch.zeros(2, 3, 3, 8, 8).to(backend), torch.zeros(2, 3, 3, 8, 8).to(backend))
    with pytest.raises(ValueError, match="conf_b must be"):
        ops.flow_metrics(g, g, c, c[:, :, :2])
    with pytest.raises(TypeError, match="float32"):
        ops.flow_metrics(g, g.double())


def test_c_entry_points_check_for_themselves(backend):
    from cvpr23_lfdm_amd import _native, ops
    import ctypes
    lib, p = _native.library(), ops._p
    st = ops._stream(lib)
    b, c, t, h, w = 1, 3, 2, 16, 20
    a = torch.rand(b, c, t, h, w).to(backend)
    out = torch.empty(b, t, 3, dtype=torch.float64, device=a.device)
    nbytes = lib.lfdm_video_metrics_ws_bytes(b, c, t, h, w)
    assert nbytes == b * t * c * 1 * 1 * 3 * 8 and lib.lfdm_video_metrics_ws_bytes(b, c, t, 10, w) == 0
    assert lib.lfdm_video_metrics_ws_bytes(1, 3, 1, 128, 128) == 3 * 8 * 4 * 3 * 8          # 118 x 118 map: 8 x 4 tiles of 16 x 32
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device)
    mean = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    good = [p(a), p(a), mean, 1, p(out), b, c, t, h, w, p(ws), nbytes, st]
    names = ["a", "b", "mean", "domain", "out", "batch", "channels", "frames", "h", "w", "ws", "ws_bytes", "stream"]
    assert lib.lfdm_video_metrics(*good) == 0

    def bad(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.lfdm_video_metrics(*args)
    for name in ("a", "b", "mean", "out", "ws"):
        assert bad(**{name: None}) != 0, name
    assert b"video_metrics" in lib.lfdm_last_error()
    assert bad(mean=None, domain=0) == 0          # the raw domain reads no mean
    assert bad(domain=3) != 0 and bad(h=10) != 0 and bad(w=10) != 0 and bad(channels=0) != 0 and bad(channels=5) != 0
    assert bad(batch=0) != 0 and bad(frames=0) != 0 and bad(ws_bytes=nbytes - 8) != 0
    g = torch.rand(b, 2, t, 8, 8).to(backend)
    cf = torch.rand(b, 1, t, 8, 8).to(backend)
    fo = torch.empty(b, t, 2, dtype=torch.float64, device=a.device)
    n = 2 * t * 64
    assert lib.lfdm_flow_metrics(p(g), n, p(g), n, p(cf), p(cf), p(fo), b, t, 8, st) == 0
    assert lib.lfdm_flow_metrics(None, n, p(g), n, None, None, p(fo), b, t, 8, st) != 0 and b"flow_metrics" in lib.lfdm_last_error()
    assert lib.lfdm_flow_metrics(p(g), n, p(g), n, p(cf), None, p(fo), b, t, 8, st) != 0
    assert lib.lfdm_flow_metrics(p(g), n - 1, p(g), n, None, None, p(fo), b, t, 8, st) != 0
    assert lib.lfdm_flow_metrics(p(g), n, p(g), n, None, None, p(fo), b, 0, 8, st) != 0
    assert lib.lfdm_flow_metrics(p(g), n, p(g), n, None, None, None, b, t, 8, st) != 0
    assert lib.lfdm_psnr_f64(None, p(fo), 4, st) != 0 and lib.lfdm_psnr_f64(p(fo), p(fo), 0, st) != 0


def test_metric_ops_refuse_cpu_tensors_on_the_product_library():
    from cvpr23_lfdm_amd import _native, ops
    _native._set_library_for_tests(None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.video_metrics(torch.zeros(1, 3, 1, 16, 16), torch.zeros(1, 3, 1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.flow_metrics(torch.zeros(1, 2, 1, 8, 8), torch.zeros(1, 2, 1, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.psnr(torch.zeros(3, dtype=torch.float64))


# ------------------------------------------------------------------------------------------ 6. accumulator
def test_accumulator(backend):
    from cvpr23_lfdm_amd import evaluate as E, ops
    shape = (6, 3, 3, 13, 29)
    a, b = _pair(shape, "smooth", seed=7)
    b[1, :, 2] = a[1, :, 2]          # two identical frames: mse == 0, left out of the PSNR mean and counted
    b[4, :, 0] = a[4, :, 0]
    a, b = a.to(backend), b.to(backend)
    table = ops.video_metrics(a, b, mean=MEAN, domain="unit")
    acc = E.MetricAccumulator()
    for lo, hi in ((0, 1), (1, 4), (4, 6)):
        assert acc.update(ops.video_metrics(a[lo:hi], b[lo:hi], mean=MEAN, domain="unit")) is acc
    r = acc.result()
    rows = table.reshape(-1, 3).cpu()
    assert r["frames"] == 18 and r["videos"] == 6 and r["identical_frames"] == 2
    for j, k in enumerate(("l1", "mse", "ssim")):
        assert abs(r[k] - rows[:, j].mean().item()) <= 1e-12 * abs(rows[:, j].mean().item()), k
        assert isinstance(r[k], float)
    pos = rows[:, 1] > 0
    want = (10 * torch.log10(1 / rows[pos, 1])).mean().item()
    assert int(pos.sum()) == 16 and abs(r["psnr"] - want) <= 1e-12 * want and math.isfinite(r["psnr"])
    assert abs(r["l1_frame_sum"] - rows[:, 0].sum().item()) <= 1e-12 * rows[:, 0].sum().item()
    whole = E.compare_videos(a, b, mean=MEAN, domain="unit")
    assert torch.equal(whole["table"], table) and tuple(whole["psnr"].shape) == (6, 3) and torch.isinf(whole["psnr"][1, 2])
    assert whole["summary"]["identical_frames"] == 2 and abs(whole["summary"]["ssim"] - r["ssim"]) <= 1e-12
    same = E.MetricAccumulator().update(ops.video_metrics(a, a, mean=MEAN)).result()
    assert same["identical_frames"] == same["frames"] == 18 and same["psnr"] == math.inf and same["ssim"] == 1.0
    fresh = E.compare_videos(a, b, mean=MEAN, domain="unit")
    assert set(fresh) == {"table", "psnr"}          # the summary (a synchronisation) is made when it is first read
    assert fresh["summary"] == whole["summary"] and "summary" in fresh
    with pytest.raises(KeyError):
        fresh["nothing"]
    with pytest.raises(RuntimeError, match="nothing has been accumulated"):
        E.MetricAccumulator().result()
    with pytest.raises(ValueError, match="float64"):
        E.MetricAccumulator().update(table.float())


# ------------------------------------------------------------------------------------------ 7. model level
S, HW, NF, STEPS = 8, 32, 4, 3          # the smallest size of the existing end-to-end tests: latent 8 x 8, frames 32 x 32
S_LFAE = 32          # the frozen-LFAE pass needs 128 x 128 frames: the region predictor's five halvings of the quarter-scale frame (its tests' size)


def _whole_model(dev):
    """A whole UNet forward under the fiber emulator takes minutes (tests/test_end_to_end.py): the model runs on the GPU, and under the
    emulator only with LFDM_EMU_E2E=1.  Otherwise the emulator tests drive the same evaluation code over a model whose network passes
    are replaced by recorded-style stand-ins, so that everything behind them (the metric kernels, the pairing, the summaries) still runs."""
    return dev == "cuda" or os.environ.get("LFDM_EMU_E2E", "0") == "1"


def _stand_in(m, monkeypatch):
    lat, nf = m.diffusion.image_size, m.diffusion.num_frames
    hw = 4 * lat

    def forward():
        g = torch.Generator().manual_seed(11)
        real = m.real_vid.float()
        b = real.shape[0]
        m._real_decode = None
        m._real_out_vid = real + 0.05 * torch.randn(real.shape, generator=g)
        m._real_warped_vid = real + 0.1 * torch.randn(real.shape, generator=g)
        z = torch.randn(b, 3, nf, lat, lat, generator=g).clamp(-1, 1)
        m.real_vid_grid, m.real_vid_conf = z[:, :2], (z[:, 2:3] + 1) * 0.5

    def sample_one_video(cond_scale, **kw):
        b = m.sample_img.shape[0]
        x = torch.empty(b, 3, nf, lat, lat).normal_()          # the default generator, like GaussianDiffusion._draw
        m.sample_latent = x.clamp(-1, 1)
        m.sample_vid_grid, m.sample_vid_conf = m.sample_latent[:, :2], (m.sample_latent[:, 2:3] + 1) * 0.5
        up = F.interpolate(m.sample_latent.permute(0, 2, 1, 3, 4).reshape(b * nf, 3, lat, lat), size=(hw, hw), mode="bilinear")
        m.sample_out_vid = (0.5 + 0.25 * m.sample_steps * up).reshape(b, nf, 3, hw, hw).permute(0, 2, 1, 3, 4).contiguous()
        m.sample_warped_vid = m.sample_out_vid.clone()
    m.sample_steps = 1.0
    monkeypatch.setattr(m, "forward", forward)
    monkeypatch.setattr(m, "sample_one_video", sample_one_video)
    return m


def _model(dev, monkeypatch, lat=S, **kw):
    if _whole_model(dev):
        m = synth.build_flow_diffusion(dev, img_size=lat, num_frames=NF, sampling_timesteps=STEPS, **kw)[0]
        m.region_predictor.load_state_dict(synth.region_state())
        m.bg_predictor.load_state_dict(synth.bg_state())
        return m.eval()
    from cvpr23_lfdm_amd import FlowDiffusion
    m = FlowDiffusion(img_size=lat, num_frames=NF, sampling_timesteps=STEPS, is_train=False, config_pth=synth.CONFIG, **kw)
    return _stand_in(m, monkeypatch)


def test_lfae_reconstruction_reports_the_reference_numbers(backend, monkeypatch):
    from cvpr23_lfdm_amd import evaluate as E
    m = _model(backend, monkeypatch, lat=S_LFAE)
    hw = 4 * S_LFAE
    ref_img, real_vid = synth.train_inputs(2, NF, hw)[:2]
    res = E.lfae_reconstruction(m, real_vid.to(backend), ref_img.to(backend), mean=MEAN)
    # LFAE/test_flowautoenc_mug.py:170-171, 208-213 for one batch: l1_loss(reduction="sum") over (T, B, C, H, W) / (videos * H * W * 3)
    real = m.real_vid.double().permute(2, 0, 1, 3, 4).cpu()
    for key, vid in (("out_loss", m.real_out_vid), ("warp_loss", m.real_warped_vid)):
        want = (real - vid.double().permute(2, 0, 1, 3, 4).cpu()).abs().sum().item() / (2 * hw * hw * 3)
        print("%s: %.12g against %.12g" % (key, res[key], want))
        assert want > 0 and abs(res[key] - want) <= REL * want, key
    for key in ("out", "warp", "out_raw", "warp_raw"):
        assert tuple(res[key]["table"].shape) == (2, NF, 3) and torch.isfinite(res[key]["table"]).all()
        assert res[key]["summary"]["frames"] == 2 * NF and res[key]["summary"]["videos"] == 2
    assert abs(res["out_raw"]["summary"]["l1"] * NF - res["out_loss"]) <= 1e-12 * res["out_loss"]          # per-frame mean x frames
    assert torch.equal(res["out"]["table"], E.compare_videos(m.real_out_vid, m.real_vid, MEAN, "unit")["table"])


def test_sample_against_real(backend, monkeypatch):
    from cvpr23_lfdm_amd import evaluate as E
    m = _model(backend, monkeypatch, lat=S_LFAE)
    real_vid = synth.train_inputs(1, NF, 4 * S_LFAE)[1].to(backend)
    img, cond = synth.inputs(1, 4 * S_LFAE)
    with pytest.raises(RuntimeError, match="nothing has been sampled"):
        E.sample_against_real(m, real_vid)
    torch.manual_seed(3)
    m.set_sample_input(sample_img=img.to(backend), sample_text=cond.to(backend))
    m.sample_one_video(cond_scale=1.0)
    res = E.sample_against_real(m, real_vid, mean=MEAN)
    for key in ("vs_real", "vs_lfae", "lfae"):
        t = res[key]["table"]
        assert t.dtype == torch.float64 and tuple(t.shape) == (1, NF, 3) and torch.isfinite(t).all() and tuple(res[key]["psnr"].shape) == (1, NF)
        assert all(math.isfinite(res[key]["summary"][k]) for k in ("l1", "mse", "ssim", "psnr"))
    f = res["flow"]["table"]
    assert f.dtype == torch.float64 and tuple(f.shape) == (1, NF, 2) and torch.isfinite(f).all() and (f >= 0).all()
    assert res["flow"]["summary"]["frames"] == NF and res["flow"]["summary"]["epe"] > 0
    with pytest.raises(ValueError, match="does not match"):
        E.sample_against_real(m, real_vid[:, :, :2])


def test_ab_compare_pairs_by_seed(backend, monkeypatch):
    """both runs follow torch.manual_seed(seed), so a configuration against itself reproduces every frame - the default
    DDIM (eta = 1) included, whose per-step draws then coincide too - and another seed does not."""
    from cvpr23_lfdm_amd import evaluate as E
    m = _model(backend, monkeypatch)
    img, cond = synth.inputs(1, HW)
    res = E.ab_compare(m, m, img.to(backend), cond.to(backend), seed=5, mean=MEAN)
    v = res["video"]["summary"]
    assert v["frames"] == NF and v["identical_frames"] == NF and v["ssim"] == 1.0 and v["psnr"] == math.inf
    assert torch.equal(res["flow"]["table"], torch.zeros_like(res["flow"]["table"])) and tuple(res["flow"]["table"].shape) == (1, NF, 2)
    a = m.sample_out_vid.clone()
    torch.manual_seed(6)
    m.sample_one_video(cond_scale=1.0)
    assert not torch.equal(a, m.sample_out_vid)
    if _whole_model(backend):
        other = synth.build_flow_diffusion(backend, img_size=S, num_frames=NF, sampling_timesteps=STEPS, sampler="dpmpp_2m")[0]
    else:
        other = _model(backend, monkeypatch)
        other.sample_steps = 0.9
    res = E.ab_compare(m, other, img.to(backend), cond.to(backend), seed=5, mean=MEAN)
    assert res["video"]["summary"]["identical_frames"] < NF and torch.isfinite(res["video"]["table"]).all()
    assert res["flow"]["summary"]["epe"] > 0 or not _whole_model(backend)


def _eval_tool():
    path = os.path.join(synth.REPO_ROOT, "tools", "eval.py")
    spec = importlib.util.spec_from_file_location("lfdm_eval_tool", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _tool_for(backend, monkeypatch):
    """tools/eval.py; under the emulator (no whole model) its build_model hands out stand-in models of the asked size."""
    tool = _eval_tool()
    if not _whole_model(backend):
        from cvpr23_lfdm_amd import FlowDiffusion

        def stand_in(args, overrides=None):
            cfg = dict(sampler=args.sampler, steps=args.steps, conv_precision=args.conv_precision, use_ema=args.use_ema)
            cfg.update(overrides or {})
            m = _stand_in(FlowDiffusion(is_train=False, img_size=args.size // 4, num_frames=args.frames, sampling_timesteps=cfg["steps"],
                                        config_pth=args.config, sampler=cfg["sampler"], conv_precision=cfg["conv_precision"]), monkeypatch)
            m.sample_steps = 1.0 + 0.01 * cfg["steps"]
            return m, cfg
        monkeypatch.setattr(tool, "build_model", stand_in)
    return tool


def test_eval_tool_ab_writes_its_json(backend, monkeypatch, tmp_path, capsys):
    tool = _tool_for(backend, monkeypatch)
    path = str(tmp_path / "sub" / "ab.json")
    out = tool.main(["ab", "--synthetic", "--size", str(HW), "--frames", str(NF), "--steps", str(STEPS), "--a", "sampler=reference",
                     "--b", "sampler=dpmpp_2m,steps=2", "--seed", "9", "--out", path])
    with open(path) as f:
        disk = json.load(f)
    assert disk == json.loads(json.dumps(out))
    assert disk["command"] == "ab" and disk["a"]["sampler"] == "reference" and disk["a"]["steps"] == STEPS
    assert disk["b"] == dict(sampler="dpmpp_2m", steps=2, conv_precision="fp32", use_ema=False)
    assert set(disk["video"]) == {"l1", "mse", "ssim", "psnr", "identical_frames", "frames", "videos", "l1_frame_sum"}
    assert set(disk["flow"]) == {"epe", "occlusion_error", "frames", "videos"}
    assert set(disk["per_frame"]) == {"l1", "mse", "psnr", "ssim", "epe", "occlusion_error"}
    assert all(len(v) == NF for v in disk["per_frame"].values()) and disk["video"]["frames"] == NF
    assert disk["held_fixed"] == tool.HELD_FIXED and disk["seed"] == 9 and disk["domain"] == "unit"
    assert "B against A per frame" in capsys.readouterr().out


def test_eval_tool_options():
    tool = _eval_tool()
    assert tool.parse_overrides("sampler=dpmpp_2m, steps=20,conv_precision=bf16,use_ema=1") == dict(
        sampler="dpmpp_2m", steps=20, conv_precision="bf16", use_ema=True)
    assert tool.parse_overrides("") == {}
    with pytest.raises(SystemExit):
        tool.parse_overrides("eta=0")
    with pytest.raises(SystemExit):
        tool.parse_overrides("steps")
    for cmd in ("lfae", "dm", "ab"):
        args = tool.build_parser().parse_args([cmd, "--synthetic", "--sampler", "dpmpp_2m", "--steps", "20", "--conv-precision", "bf16",
                                               "--size", "64", "--frames", "8", "--use-ema", "--config", "c.yaml", "--lfae-ckpt", "l.pth",
                                               "--dm-ckpt", "d.pth", "--bert", "bert"])
        assert args.command == cmd and args.steps == 20 and args.size == 64 and args.use_ema and args.bert == "bert"
    assert tool.build_parser().parse_args(["lfae", "--dataset", "natops", "--data-dir", "/x"]).dataset == "natops"
    assert tool.jsonable({"a": [1.0, math.inf], "b": (math.nan,)}) == {"a": [1.0, "inf"], "b": ["nan"]}


def _mug_tree(root):
    """Two test-subject takes of the MUG layout (subject / expression / take / frames), 6 and 3 random 60 x 80 frames."""
    takes = {}
    for subject, exp, n, seed in (("001", "fear", 6, 3), ("046", "anger", 3, 4)):
        d = os.path.join(root, subject, exp, "take000")
        os.makedirs(d)
        g = np.random.default_rng(seed)
        takes["%s_%s_take000" % (subject, exp)] = [g.integers(0, 256, size=(60, 80, 3), dtype=np.uint8) for _ in range(n)]
        for i, img in enumerate(takes["%s_%s_take000" % (subject, exp)]):
            IO.imsave(os.path.join(d, "img_%04d.png" % i), img)
    return takes


def test_eval_tool_batches_use_the_reference_mean(tmp_path):
    """The reference's test loops build their data sets with mean=MEAN=(0, 0, 0) (LFAE/test_flowautoenc_mug.py:34,116), not the classes'
    default of 128: frames reach the model as x / 255.  --mean changes both the subtraction and the mean the metrics add back."""
    from cvpr23_lfdm_amd import datasets as DS
    tool = _eval_tool()
    root = str(tmp_path / "MUG")
    _mug_tree(root)
    args = tool.build_parser().parse_args(["lfae", "--dataset", "mug", "--data-dir", root, "--size", "32", "--frames", "4", "--batch-size", "2"])
    assert tuple(args.mean) == (0.0, 0.0, 0.0)
    mean, it = tool.batches(args)
    (vid, labels, names), = list(it)
    assert mean == (0.0, 0.0, 0.0) and tuple(vid.shape) == (2, 3, 4, 32, 32) and vid.dtype == torch.float32
    assert labels == ["fear", "anger"] and names == ["001_fear_take000", "046_anger_take000"]
    assert vid.min() >= 0 and vid.max() <= 1 and vid.max() > 0.6 and vid.min() < 0.4          # x / 255, not (x - 128) / 255
    zero = DS.MUG_test(root, num_frames=4, image_size=32, mean=(0, 0, 0))
    assert np.array_equal(vid[0].numpy(), zero[0][0]) and np.array_equal(vid[1].numpy(), zero[1][0])
    args = tool.build_parser().parse_args(["dm", "--dataset", "mug", "--data-dir", root, "--size", "32", "--frames", "4", "--mean", "128", "100", "90",
                                           "--max-videos", "1"])
    mean, it = tool.batches(args)
    (shifted, _, _), = list(it)
    assert mean == (128.0, 100.0, 90.0) and tuple(shifted.shape) == (1, 3, 4, 32, 32)
    back = shifted + torch.tensor(mean).view(1, 3, 1, 1, 1) / 255.0
    assert (back - vid[:1]).abs().max() < 1e-6
    with pytest.raises(SystemExit):
        tool.batches(tool.build_parser().parse_args(["lfae"]))


def test_eval_tool_lfae_over_a_frame_folder(backend, monkeypatch, tmp_path):
    """`lfae` over a tiny on-disk MUG tree: what reaches the model and the metrics (frames as x / 255 and mean 0 by default, the shifted
    frames and that mean with --mean), and the JSON with the reference's keys."""
    from cvpr23_lfdm_amd import datasets as DS, evaluate as E
    tool = _tool_for(backend, monkeypatch)
    root = str(tmp_path / "MUG")
    _mug_tree(root)
    size = 4 * S_LFAE if _whole_model(backend) else HW
    seen = []
    real = E.lfae_reconstruction

    def spy(model, real_vid, ref_img, mean=(0, 0, 0), domain="unit"):
        seen.append((real_vid.clone(), ref_img.clone(), tuple(mean), domain))
        return real(model, real_vid, ref_img, mean=mean, domain=domain)
    monkeypatch.setattr(tool.E, "lfae_reconstruction", spy)
    zero = DS.MUG_test(root, num_frames=NF, image_size=size, mean=(0, 0, 0))
    common = ["lfae", "--dataset", "mug", "--data-dir", root, "--size", str(size), "--frames", str(NF)]
    out = tool.main(common + ["--out", str(tmp_path / "lfae.json")])
    assert len(seen) == 2 and all(m == (0.0, 0.0, 0.0) and d == "unit" for _, _, m, d in seen)
    for i, (vid, ref, _, _) in enumerate(seen):
        assert np.array_equal(vid[0].numpy(), zero[i][0]) and torch.equal(ref, vid[:, :, 0]) and vid.min() >= 0 and vid.max() <= 1
    with open(str(tmp_path / "lfae.json")) as f:
        disk = json.load(f)
    assert disk == json.loads(json.dumps(out)) and disk["command"] == "lfae" and disk["mean"] == [0.0, 0.0, 0.0]
    assert disk["videos"] == 2 and disk["frames"] == 2 * NF and disk["out_loss"] > 0 and disk["warp_loss"] > 0
    for key in ("out", "warp"):
        assert set(disk[key]) == {"l1", "mse", "ssim", "psnr", "identical_frames", "frames", "videos", "l1_frame_sum"}
        assert all(math.isfinite(disk[key][k]) for k in ("l1", "mse", "ssim", "psnr"))
    del seen[:]
    shifted = tool.main(common + ["--mean", "128", "128", "128", "--max-videos", "1", "--out", str(tmp_path / "lfae128.json")])
    (vid, _, mean, _), = seen
    assert mean == (128.0, 128.0, 128.0) and shifted["mean"] == [128.0, 128.0, 128.0] and shifted["videos"] == 1
    assert vid.min() < 0 and (vid + 128.0 / 255.0 - torch.from_numpy(zero[0][0])).abs().max() < 1e-6


def test_eval_tool_lfae_and_dm_synthetic(backend, monkeypatch, tmp_path):
    """--synthetic through the tool's own model construction (on the GPU: tools/demo.py's make_model plus the synthetic region and
    background predictors, the frozen-LFAE pass and the sampler for real)."""
    tool = _tool_for(backend, monkeypatch)
    size = 4 * S_LFAE if _whole_model(backend) else HW
    common = ["--synthetic", "--size", str(size), "--frames", str(NF), "--steps", str(STEPS)]
    lfae = tool.main(["lfae"] + common + ["--out", str(tmp_path / "l.json")])
    assert lfae["videos"] == 2 and lfae["frames"] == 2 * NF and lfae["mean"] == [0.0, 0.0, 0.0]
    assert 0 < lfae["out_loss"] < 10 and 0 < lfae["warp_loss"] < 10 and abs(lfae["out"]["ssim"]) <= 1
    dm = tool.main(["dm"] + common + ["--sampler", "dpmpp_2m", "--out", str(tmp_path / "d.json")])
    assert dm["config"]["sampler"] == "dpmpp_2m" and dm["config"]["steps"] == STEPS
    for key in ("vs_real", "vs_lfae", "lfae"):
        assert dm[key]["frames"] == 2 * NF and all(math.isfinite(dm[key][k]) for k in ("l1", "mse", "ssim"))
    assert set(dm["flow"]) == {"epe", "occlusion_error", "frames", "videos"} and dm["flow"]["frames"] == 2 * NF and dm["flow"]["epe"] > 0
