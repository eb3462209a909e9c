"""Temporal resampling of a sampled latent: csrc/latent_resample.hip through ops.latent_resample / latent_resample_maps,
retime.frame_times, FlowDiffusion.decode_at and the frame_times keyword of the sampling calls, evaluate.interpolation_error and the new
flags of tools/demo.py and tools/eval.py.

Kernel tests take the `backend` fixture: the x86 emulator build everywhere, the gfx950 build on the GPU.  Their float64 references and
time tables are written out here from the formulas of include/lfdm_hip.h, not taken from ops.

Error bounds, in units of u = 2^-24 times the largest |tap| of the element (M):
  linear  x0 + a (x1 - x0): the difference (|d| <= 2 M) rounds by <= 2 u M, which the product by a < 1 keeps; the product rounds by
          <= u |a d| <= 2 u M; the sum (|.| <= M) by <= u M  ->  5 u M, bound 6 u M.
  cubic   the weights (absolute sum <= 1.25) are evaluated in fp64 and rounded once (<= 0.5 u each, relative): 0.625 u M; four products:
          0.625 u M; three sums of partial results <= 1.25 M: 3.75 u M  ->  5 u M, bound 16 u M.

Model level: the tiny synthetic model of tests/test_render.py (num_frames 8, latent 8 x 8, image 32 x 32, 4 sampler steps), which really
samples.  These cases are GPU-only: under the emulator a 32 x 32 decode takes 0.7 s per frame and the emulator keeps about 0.3 GB per
decoded frame until the process ends - the model-level cases together came to 100 s and 15 GB in the CPU suite.  What the emulator does
run of decode_at is its own logic (pieces, attributes, clamping, refusals) around a stand-in for the generator, with the resampling
kernel real (test_decode_at_pieces_and_attributes)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lfdm_oracle as O
import synth
from util import assert_close

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
MODES = ("linear", "cubic")
PLANES = ((4, 4), (4, 8), (8, 8))
FRAMES = (1, 2, 5)


# ------------------------------------------------------------------------------------------ references
def _tables(times, frames):
    """lfdm_hip.h: i = floor(t) and a = t - i in float64, a rounded to fp32; an a that rounds to 1.0f becomes (i + 1, 0)."""
    idx, frac = [], []
    for t in times:
        t = float(t)
        i = math.floor(t)
        a = np.float32(t - i)
        if a == np.float32(1.0):
            i, a = i + 1, np.float32(0.0)
        assert 0 <= i <= frames - 1 and (a == 0 or i < frames - 1)
        idx.append(int(i))
        frac.append(a)
    return idx, frac


def _weights(a):
    return [((2 - a) * a - 1) * a / 2, ((3 * a - 5) * a * a + 2) / 2, ((4 - 3 * a) * a + 1) * a / 2, (a - 1) * a * a / 2]


def _reference(x, times, mode):
    """float64 result and the per-element largest |tap| from the fp32 latent x (B, C, T, H, W)."""
    t_in = x.shape[2]
    xd = x.double()
    idx, frac = _tables(times, t_in)
    outs, taps = [], []
    for i, a in zip(idx, frac):
        a = float(a)
        if a == 0.0:
            outs.append(xd[:, :, i])
            taps.append(xd[:, :, i].abs())
        elif mode == "linear":
            outs.append((1 - a) * xd[:, :, i] + a * xd[:, :, i + 1])
            taps.append(torch.maximum(xd[:, :, i].abs(), xd[:, :, i + 1].abs()))
        else:
            ii = [max(i - 1, 0), i, i + 1, min(i + 2, t_in - 1)]
            w = _weights(a)
            outs.append(sum(w[k] * xd[:, :, ii[k]] for k in range(4)))
            taps.append(torch.stack([xd[:, :, k].abs() for k in ii]).max(dim=0).values)
    return torch.stack(outs, dim=2), torch.stack(taps, dim=2)


def _times(frames):
    """Unsorted, with repeats: 0, T - 1, integers, values within 1e-7 of an integer on both sides (one of them rounds to a = 1.0f)."""
    if frames == 1:
        return [0.0, 0, 0.0]
    if frames == 2:
        return [1.0, 0.5, 0.0, 0.25, 1 - 1e-7, 1e-7, 0.5, 1 - 1e-9, 0.8125, 1]
    last = frames - 1
    return [2.0, last, 3.5, 0.0, 1.25, 2 + 1e-7, 3 - 1e-7, 0.75, last - 1e-7, 1e-7, 2.5, 2.5, last - 1e-9, 1, 2 - 1e-9, 0.3333333333, 3.9]


def _latent(b, c, t, h, w, seed):
    """Values spread over seven decades of scale, both signs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, c, t, h, w, generator=g)
    return (x * torch.pow(10.0, torch.randint(-4, 3, x.shape, generator=g).float())).contiguous()


def _bound(mode):
    return (6.0 if mode == "linear" else 16.0) * U


def _check_against_f64(got, x, times, mode, what):
    want, taps = _reference(x, times, mode)
    assert got.shape == want.shape and got.dtype == torch.float32, what
    err = (got.double().cpu() - want).abs()
    unit = float((err / (taps * U).clamp_min(1e-300)).max())
    print("%s: worst error %.2f u max|taps| (bound %.0f)" % (what, unit, _bound(mode) / U))
    assert bool((err <= _bound(mode) * taps).all()), (what, unit)


class _Maps:
    """FlowDiffusion._maps without a model around it."""

    def __init__(self, residual):
        self.use_residual_flow = residual

    def __call__(self, pred):
        from cvpr23_lfdm_amd import FlowDiffusion
        return FlowDiffusion._maps(self, pred)

    def get_grid(self, *a, **kw):
        from cvpr23_lfdm_amd import FlowDiffusion
        return FlowDiffusion.get_grid(self, *a, **kw)


def _maps_of(pred, residual):
    """_maps(pred); for a plane that is not square (which _maps does not take) its two statements with H and W kept apart."""
    if pred.shape[3] == pred.shape[4]:
        return _Maps(residual)(pred)
    b, _, nf, h, w = pred.shape
    maps = pred
    if residual:
        grid = pred[:, :2] + _Maps(True).get_grid(b, nf, h, w, normalize=True).to(pred.device)
        maps = torch.cat((grid, pred[:, 2:3]), dim=1).contiguous()
    return maps, (pred[:, 2, :, :, :].unsqueeze(dim=1) + 1) * 0.5


# ------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("frames", FRAMES)
def test_resample_against_float64(backend, frames, mode):
    from cvpr23_lfdm_amd import ops
    for h, w in PLANES:
        x = _latent(2, 3, frames, h, w, seed=100 * frames + h + w)
        times = _times(frames)
        got = ops.latent_resample(x.to(backend), times, mode)
        assert tuple(got.shape) == (2, 3, len(times), h, w) and got.is_contiguous()
        _check_against_f64(got, x, times, mode, "%s T=%d %dx%d on %s" % (mode, frames, h, w, backend))
        # a host tensor of times is the same call
        again = ops.latent_resample(x.to(backend), torch.tensor(times, dtype=torch.float64), mode)
        assert torch.equal(got, again)


def test_time_tables_are_the_documented_ones():
    from cvpr23_lfdm_amd import ops
    for frames in FRAMES:
        idx, frac = ops.resample_tables(_times(frames), frames)
        want_i, want_a = _tables(_times(frames), frames)
        assert idx.dtype == np.int32 and frac.dtype == np.float32
        assert idx.tolist() == want_i and frac.tolist() == [float(a) for a in want_a]
        assert (frac >= 0).all() and (frac < 1).all()
    idx, frac = ops.resample_tables([2 - 1e-9, 3 - 1e-7], 5)
    assert idx.tolist() == [2, 2] and frac[0] == 0.0 and 0.9999 < frac[1] < 1.0          # the first rounds to a = 1.0f -> (2, 0)


# ------------------------------------------------------------------------------------------ 2. exact frames
@pytest.mark.parametrize("mode", MODES)
def test_integer_times_select_the_frame(backend, mode):
    """Selected, not multiplied: every frame that is not asked for is NaN and none reaches the output; the output buffer starts as NaN
    and is overwritten entirely; the guard behind it keeps its value."""
    from cvpr23_lfdm_amd import ops
    for frames, times in ((1, [0, 0]), (2, [1, 1.0]), (2, [0]), (5, [2, 2, 0]), (5, [4, 3.0])):
        for h, w in PLANES:
            x = _latent(2, 3, frames, h, w, seed=7 + frames + h * w)
            picked = sorted({int(t) for t in times})
            poisoned = torch.full_like(x, float("nan"))
            poisoned[:, :, picked] = x[:, :, picked]
            want = x[:, :, [int(t) for t in times]]
            shape = (2, 3, len(times), h, w)
            n, guard = int(np.prod(shape)), 64
            for maps in (False, True):
                buf = torch.full((n + guard,), float("nan")).to(backend)
                buf[n:] = 12345.0
                out = buf[:n].view(shape)
                if maps:
                    got, conf = ops.latent_resample_maps(poisoned.to(backend), times, mode, residual=False, clamp_from=2, out=out)
                    assert torch.equal(conf.cpu(), (want[:, 2:3] + 1) * 0.5)
                else:
                    got = ops.latent_resample(poisoned.to(backend), times, mode, clamp_from=0, out=out)
                assert got.data_ptr() == buf.data_ptr()
                assert torch.equal(got.cpu(), want), (frames, times, h, w, maps)          # (torch.equal is False on any NaN)
                assert bool((buf[n:] == 12345.0).all())


# ------------------------------------------------------------------------------------------ 3. linear reproduction
def test_a_latent_affine_in_time_is_reproduced(backend):
    from cvpr23_lfdm_amd import ops
    frames, h, w = 5, 4, 8
    g = torch.Generator().manual_seed(3)
    base = torch.randint(-64, 64, (2, 3, 1, h, w), generator=g).float() / 8          # multiples of 1 / 8 below 2^7: every frame is exact
    slope = torch.randint(-32, 32, (2, 3, 1, h, w), generator=g).float() / 8
    x = (base + slope * torch.arange(frames).float().view(1, 1, frames, 1, 1)).contiguous()
    times = [0.0, 0.125, 0.5, 0.9, 1.0, 1.3, 2.0, 2.71, 3.0, 3.25, 3.999, 4.0, 1.5, 2.999999]
    exact = base.double() + slope.double() * torch.tensor(times, dtype=torch.float64).view(1, 1, -1, 1, 1)
    scale = x.abs().amax(dim=2, keepdim=True).double()
    lin = ops.latent_resample(x.to(backend), times, "linear").double().cpu()
    # the fp32 fraction a differs from the time's by <= u / 2: |slope| u / 2 more than the kernel's own bound
    assert bool(((lin - exact).abs() <= _bound("linear") * scale + slope.abs().double() * U).all())
    cub = ops.latent_resample(x.to(backend), times, "cubic").double().cpu()
    for j, t in enumerate(times):
        i = min(int(math.floor(t)), frames - 2)
        if 1 <= t <= frames - 2:          # interior intervals: Catmull-Rom reproduces a straight line
            assert bool(((cub[:, :, j] - exact[:, :, j]).abs() <= (_bound("cubic") * scale + slope.abs().double() * U)[:, :, 0]).all()), t
        lo = torch.minimum(x[:, :, i], x[:, :, i + 1]).double() - _bound("cubic") * scale[:, :, 0]
        hi = torch.maximum(x[:, :, i], x[:, :, i + 1]).double() + _bound("cubic") * scale[:, :, 0]
        assert bool(((cub[:, :, j] >= lo) & (cub[:, :, j] <= hi)).all()), t          # at the clamped ends: between its two frames
        if t == int(t):
            assert torch.equal(cub[:, :, j].float(), x[:, :, int(t)]) and torch.equal(lin[:, :, j].float(), x[:, :, int(t)])


# ------------------------------------------------------------------------------------------ 4. maps form
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_maps_at_integer_times_are_maps_of_the_frames(backend, mode, residual):
    from cvpr23_lfdm_amd import ops
    for frames, times in ((1, [0]), (2, [1, 0, 1]), (5, [3, 0, 4, 4, 1])):
        for h, w in PLANES:
            x = (_latent(2, 3, frames, h, w, seed=41 + h + w) * 0.01).clamp(-3, 3).contiguous().to(backend)
            maps, conf = ops.latent_resample_maps(x, times, mode, residual=residual, clamp_from=2)
            want_maps, want_conf = _maps_of(x[:, :, times].contiguous(), residual)
            assert tuple(maps.shape) == (2, 3, len(times), h, w) and tuple(conf.shape) == (2, 1, len(times), h, w)
            assert torch.equal(maps, want_maps) and torch.equal(conf, want_conf), (frames, h, w)


@pytest.mark.parametrize("mode", MODES)
def test_maps_at_fractional_times_are_the_plain_form_plus_one_rounding(backend, mode):
    from cvpr23_lfdm_amd import ops
    for frames in (2, 5):
        for h, w in PLANES:
            x = torch.tanh(_latent(2, 3, frames, h, w, seed=5 + h)).contiguous().to(backend)
            times = _times(frames)
            plain = ops.latent_resample(x, times, mode, clamp_from=2)
            maps, conf = ops.latent_resample_maps(x, times, mode, residual=False, clamp_from=2)
            assert torch.equal(maps, plain) and torch.equal(conf, (plain[:, 2:3] + 1) * 0.5)
            maps, conf = ops.latent_resample_maps(x, times, mode, residual=True, clamp_from=2)
            ident = _Maps(True).get_grid(2, len(times), h, w, normalize=True).double()
            back = maps[:, :2].double().cpu() - ident
            # one rounding of the sum: half an ulp of the sum, <= u |sum|
            assert bool(((back - plain[:, :2].double().cpu()).abs() <= U * maps[:, :2].double().cpu().abs()).all())
            assert torch.equal(maps[:, 2], plain[:, 2])
            back = conf.double().cpu() * 2 - 1          # fl(v + 1) * 0.5 is exact: one rounding, of v + 1
            assert bool(((back - plain[:, 2:3].double().cpu()).abs() <= U * (plain[:, 2:3].double().cpu() + 1).abs()).all())
            _check_against_f64(plain[:, :2], x[:, :2].cpu(), times, mode, "flow channels %s T=%d" % (mode, frames))


def test_cubic_overshoot_is_clamped_from_clamp_from_on(backend):
    """An occlusion channel in [-1, 1] that cubic weights carry outside it.  A channel that strictly alternates +1, -1, +1, ... cannot
    show this: its Catmull-Rom tangents (x[i+1] - x[i-1]) / 2 are all zero, so every interval is a monotone Hermite step between its two
    frames (asserted below).  Alternating in pairs (+1, +1, -1, -1, +1) does: halfway between two equal frames the weights
    (-1, 9, 9, -1) / 16 give 1.125.  The clamp acts on channels >= clamp_from only, and never on a selected frame."""
    from cvpr23_lfdm_amd import ops
    frames, h, w = 5, 4, 4
    x = torch.zeros(1, 3, frames, h, w)
    pairs = torch.tensor([1.0, 1.0, -1.0, -1.0, 1.0]).view(1, frames, 1, 1)
    x[:, 0] = pairs
    x[:, 2] = pairs
    x = x.to(backend)
    times = [0.5, 2.5, 1.5, 3.25, 0.25]
    free = ops.latent_resample(x, times, "cubic")
    assert float(free[:, 2, 0].max()) == 1.125 and float(free[:, 2, 1].min()) == -1.25          # (2.5: both outer frames are +1)
    held = ops.latent_resample(x, times, "cubic", clamp_from=2)
    assert float(held[:, 2].max()) == 1.0 and float(held[:, 2].min()) == -1.0
    assert torch.equal(held[:, :2], free[:, :2]) and float(held[:, 0].max()) == 1.125          # channels below clamp_from are left alone
    assert torch.equal(held[:, 2, 2], free[:, 2, 2])                                           # (values inside [-1, 1] too)
    maps, conf = ops.latent_resample_maps(x, times, "cubic", clamp_from=2)
    assert torch.equal(maps, held) and float(conf.max()) == 1.0 and float(conf.min()) == 0.0
    # linear mode cannot overshoot, clamp or not
    assert torch.equal(ops.latent_resample(x, times, "linear", clamp_from=2), ops.latent_resample(x, times, "linear"))
    # a selected frame is the frame, whatever it holds
    y = x.clone()
    y[:, 2, 3] = 1.5
    assert float(ops.latent_resample(y, [3, 3.0], "cubic", clamp_from=2)[:, 2].min()) == 1.5
    # the strictly alternating channel stays inside its range without any clamp
    z = torch.zeros(1, 3, frames, h, w)
    z[:, 2] = torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0]).view(1, frames, 1, 1)
    fine = [k / 16 for k in range(16 * (frames - 1) + 1)]
    alt = ops.latent_resample(z.to(backend), fine, "cubic")
    assert float(alt[:, 2].abs().max()) <= 1.0 + 16 * U
    assert torch.equal(ops.latent_resample(z.to(backend), fine, "cubic", clamp_from=2)[:, 2], alt[:, 2].clamp(-1, 1))


# ------------------------------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("mode", MODES)
def test_batch_elements_are_independent_and_runs_repeat(backend, mode):
    from cvpr23_lfdm_amd import ops
    x = _latent(3, 3, 5, 4, 8, seed=77).to(backend)
    times = _times(5)
    whole, conf = ops.latent_resample_maps(x, times, mode, residual=True, clamp_from=2)
    again, conf2 = ops.latent_resample_maps(x, times, mode, residual=True, clamp_from=2)
    assert torch.equal(whole, again) and torch.equal(conf, conf2)
    for i in range(3):
        one, c1 = ops.latent_resample_maps(x[i:i + 1].contiguous(), times, mode, residual=True, clamp_from=2)
        assert torch.equal(one[0], whole[i]) and torch.equal(c1[0], conf[i]), i
    # ... and of the frames around them: every output frame alone is the same frame
    for j in (2, 5, 8):
        assert torch.equal(ops.latent_resample(x, [times[j]], mode)[:, :, 0], ops.latent_resample(x, times, mode)[:, :, j])


# ------------------------------------------------------------------------------------------ 6. refusals
def test_resample_refuses_bad_arguments(backend):
    from cvpr23_lfdm_amd import _native, ops
    dev = backend
    x = _latent(2, 3, 5, 4, 4, seed=9).to(dev)
    out = torch.full((2, 3, 2, 4, 4), 777.0).to(dev)
    conf = torch.full((2, 1, 2, 4, 4), 777.0).to(dev)
    for bad, err in (([0, -0.001], IndexError), ([4.0001, 1], IndexError), ([1, float("nan")], ValueError), ([float("inf"), 0], ValueError),
                     ([-float("inf"), 0], ValueError)):
        with pytest.raises(err, match="latent_resample"):
            ops.latent_resample(x, bad, "linear", out=out)
        with pytest.raises(err, match="latent_resample"):
            ops.latent_resample_maps(x, bad, "cubic", out=out, conf=conf)
    with pytest.raises(ValueError, match="empty"):
        ops.latent_resample(x, [], out=out)
    if dev == "cuda":          # times are checked on the host: a device tensor would cost a read-back
        with pytest.raises(ValueError, match="host"):
            ops.latent_resample(x, torch.zeros(2, device=dev), out=out)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.latent_resample(torch.zeros(1, 3, 2, 3, 2).to(dev), [0.5])
    with pytest.raises(ValueError, match="contiguous"):
        ops.latent_resample(x.transpose(3, 4), [0, 1], out=out)
    with pytest.raises(ValueError, match="contiguous"):
        ops.latent_resample(x[:, :, ::2], [0, 1], out=out)
    with pytest.raises(ValueError, match="C == 3"):
        ops.latent_resample_maps(x[:, :2].contiguous(), [0, 1])
    with pytest.raises(ValueError, match="out must be"):
        ops.latent_resample(x, [0, 1, 2], out=out)
    with pytest.raises(ValueError, match="conf must be"):
        ops.latent_resample_maps(x, [0, 1], out=out, conf=conf[:, :, :1])
    with pytest.raises(ValueError, match="out must be"):
        ops.latent_resample(x, [0, 1], out=out.double())
    with pytest.raises(ValueError, match="unknown mode"):
        ops.latent_resample(x, [0, 1], "nearest", out=out)
    with pytest.raises(ValueError, match="float32"):
        ops.latent_resample(x.double(), [0, 1], out=out)
    with pytest.raises(ValueError, match="float32"):
        ops.latent_resample(x[0], [0, 1], out=out)
    assert bool((out == 777.0).all()) and bool((conf == 777.0).all())          # nothing was launched
    # the C entry point checks for itself
    lib = _native.library()
    st, p = ops._stream(lib), ops._p
    idx = torch.tensor([0, 1], dtype=torch.int32).to(dev)
    frac = torch.tensor([0.5, 0.0]).to(dev)
    ix, iy = ops._identity_table(4, x.device), ops._identity_table(4, x.device)
    names = ["latent", "idx", "frac", "ident_x", "ident_y", "out", "conf", "batch", "channels", "frames", "out_frames", "h", "w", "mode",
             "clamp_from", "stream"]
    good = [p(x), p(idx), p(frac), p(ix), p(iy), p(out), p(conf), 2, 3, 5, 2, 4, 4, 1, 2, st]

    def call(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.lfdm_latent_resample_f32(*args)

    for name in ("latent", "idx", "frac", "out"):
        assert call(**{name: None}) != 0 and b"latent_resample" in lib.lfdm_last_error(), name
    assert call(mode=2) != 0 and b"mode" in lib.lfdm_last_error()
    assert call(mode=-1) != 0
    assert call(ident_y=None) != 0 and call(ident_x=None) != 0          # the identity tables come together
    assert call(conf=None) != 0                                          # ... and only with the maps form
    assert call(channels=2) != 0                                         # the maps form has three channels
    assert call(h=3, w=3) != 0 and b"multiple of 4" in lib.lfdm_last_error()
    assert call(batch=0) != 0 and call(frames=0) != 0 and call(out_frames=0) != 0 and call(clamp_from=-1) != 0
    assert call(out=p(x)) != 0 and b"alias" in lib.lfdm_last_error()
    assert call(conf=p(x)) != 0 and call(conf=p(out)) != 0
    assert call(out=ctypes.c_void_p(out.data_ptr() + 4)) != 0
    assert bool((out == 777.0).all()) and bool((conf == 777.0).all())
    assert call() == 0 and call(ident_x=None, ident_y=None) == 0 and call(ident_x=None, ident_y=None, conf=None, channels=3) == 0
    assert not bool((out == 777.0).any())


def test_resample_refuses_cpu_tensors_on_the_product_library():
    from cvpr23_lfdm_amd import _native, ops
    _native._set_library_for_tests(None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.latent_resample(torch.zeros(1, 3, 2, 4, 4), [0.5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.latent_resample_maps(torch.zeros(1, 3, 2, 4, 4), [0.5], "cubic", residual=True)


# ------------------------------------------------------------------------------------------ 7. ABI
def test_resample_entry_point_is_declared_and_the_abi_version_stays():
    from cvpr23_lfdm_amd import _build, _native
    header = open(os.path.join(REPO, "include", "lfdm_hip.h")).read()
    assert "lfdm_latent_resample_f32" in _native.EXPORTED_SYMBOLS and "lfdm_latent_resample_f32(" in header
    decl = re.search(r"/\* Layout:([^*]*)\*/\s*(?:#define[^\n]*\n)*int lfdm_latent_resample_f32\(", header)
    assert decl and "dense" in decl.group(1) and "alias" in decl.group(1)
    lib = _native.NativeLibrary(_build.build_hip(), "hip")
    assert lib.lfdm_abi_version() == 14          # (12 when the entry point was added; 13: lfdm_sampler_step_params; 14: lfdm_train_loss_params)


# ------------------------------------------------------------------------------------------ model level
NF, S, HW = 8, 8, 32
RESULTS = ("sample_vid_grid", "sample_vid_conf", "sample_out_vid", "sample_warped_vid")
_models = {}


@pytest.fixture
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvpr23_lfdm_amd import _native
    _native._set_library_for_tests(None)
    return "cuda"


def _smooth_latent(frames, seed):
    """A latent like a sampled one: small smooth flow (the grid itself, not a residual) and an occlusion channel inside [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(frames, 2, 4, 4, generator=g) * 0.2
    flow = F.interpolate(coarse, size=(S, S), mode="bilinear", align_corners=True) + 0.02 * torch.randn(frames, 2, S, S, generator=g)
    grid = (O.identity_grid(1, frames, S, S)[0].permute(1, 0, 2, 3) + flow).permute(1, 0, 2, 3)
    occ = torch.rand(1, frames, S, S, generator=g) * 2 - 1
    return torch.cat((grid, occ), dim=0).unsqueeze(0).contiguous()


def _sampled(dev):
    """(model holding a sample of NF frames, clones of what sample_one_video left, the source image), built once."""
    if dev not in _models:
        m = synth.build_flow_diffusion(dev, img_size=S, num_frames=NF, sampling_timesteps=4)[0]
        img, cond = synth.inputs(1, HW, seed=5)
        m.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))
        m.diffusion.noise_source = synth.NoiseTape(5)
        m.sample_one_video(cond_scale=1.0)
        base = {k: getattr(m, k).clone() for k in RESULTS + ("sample_latent",)}
        _models[dev] = (m, base, img)
    m, base, img = _models[dev]
    m.sample_latent = base["sample_latent"].clone()
    return m, base, img


def _oracle_decode(latent, img):
    """The oracle's generator decode (CPU) of every frame of a latent (1, 3, T, S, S) -> out, warped (1, 3, T, HW, HW)."""
    gsd = synth.generator_state()
    grid, conf = latent[:, :2], (latent[:, 2:3] + 1) * 0.5
    outs, warps = [], []
    for f in range(latent.shape[2]):
        g = O.generator_forward_with_flow(gsd, img, grid[:, :, f].permute(0, 2, 3, 1), conf[:, :, f])
        outs.append(g["prediction"])
        warps.append(g["deformed"])
    return torch.stack(outs, dim=2), torch.stack(warps, dim=2)


# ------------------------------------------------------------------------------------------ 8. identity
@pytest.mark.gpu
def test_decode_at_the_sampled_instants_is_the_sampled_video(gpu):
    m, base, _ = _sampled(gpu)
    m.decode_at(range(NF))
    for k in RESULTS:
        assert torch.equal(getattr(m, k), base[k]), k
    assert torch.equal(m.sample_latent, base["sample_latent"])
    m.decode_at([float(t) for t in range(NF)], "cubic")
    for k in RESULTS:
        assert torch.equal(getattr(m, k), base[k]), k
    # any order, repeats: frames are decoded independently of their neighbours in the piece
    m.decode_at([3, 3, 0])
    assert torch.equal(m.sample_out_vid, base["sample_out_vid"][:, :, [3, 3, 0]])
    assert torch.equal(m.sample_vid_grid, base["sample_vid_grid"][:, :, [3, 3, 0]])


def test_decode_at_before_sampling_raises():
    from cvpr23_lfdm_amd import FlowDiffusion
    fresh = FlowDiffusion(img_size=S, num_frames=NF, sampling_timesteps=4, is_train=False, config_pth=synth.CONFIG)
    with pytest.raises(RuntimeError, match="nothing has been sampled"):
        fresh.decode_at([0, 1])
    with pytest.raises(RuntimeError, match="nothing has been sampled"):
        fresh.decode_at([0.5], "cubic", latent=torch.zeros(1, 3, 2, S, S))          # no source image either


def test_decode_at_pieces_and_attributes(backend, monkeypatch):
    """decode_at's own logic with the resampling kernel real and the generator replaced by a stand-in (a model of 4 frames per piece,
    11 times: pieces of 4 + 4 + 3): which maps reach the decode, how the pieces are joined, what is refused, what stays."""
    from cvpr23_lfdm_amd import FlowDiffusion, ops
    m = FlowDiffusion(img_size=S, num_frames=4, sampling_timesteps=4, is_train=False, config_pth=synth.CONFIG)
    calls = []

    def decode_video(img, skips, fx, fy, occ, n, h, w, batch_stride, plane, occ_scale, occ_bias):
        assert skips == "skips" and (h, w, plane, batch_stride) == (S, S, S * S, 3 * n * S * S) and (occ_scale, occ_bias) == (0.5, 0.5)
        assert tuple(fx.shape) == tuple(fy.shape) == tuple(occ.shape) == (1, n, S, S) and fx.stride(0) == batch_stride
        calls.append(n)
        return torch.stack((fx, fy, occ), dim=1) * 2, torch.stack((occ, fx, fy), dim=1)
    monkeypatch.setattr(m.generator, "encode", lambda img: "skips")
    monkeypatch.setattr(m.generator, "decode_video", decode_video)
    m.sample_img = synth.inputs(1, HW, seed=5)[0].to(backend)
    latent = _smooth_latent(6, 80).to(backend)
    latent[:, 2] = torch.tensor([1.0, 1.0, -1.0, -1.0, 1.0, 1.0]).view(1, 6, 1, 1).to(backend)          # cubic overshoots between equal frames
    m.sample_latent = latent
    times = [0, 0.5, 1, 2.25, 5, 4.5, 3, 3, 0.125, 4.75, 2]
    for mode, residual in (("linear", False), ("cubic", False), ("cubic", True)):
        m.use_residual_flow = residual
        del calls[:]
        m.decode_at(times, mode)
        assert calls == [4, 4, 3]
        want, conf = ops.latent_resample_maps(latent, times, mode, residual=residual, clamp_from=2 if mode == "cubic" else None)
        assert torch.equal(m.sample_vid_grid, want[:, :2]) and torch.equal(m.sample_vid_conf, conf)
        assert torch.equal(m.sample_out_vid, want * 2) and torch.equal(m.sample_warped_vid, want[:, [2, 0, 1]])
        assert m.sample_latent is latent and float(m.sample_vid_conf.max()) == 1.0 and float(m.sample_vid_conf.min()) == 0.0
        if mode == "cubic":
            assert float(ops.latent_resample(latent, times, mode)[:, 2].max()) > 1.0          # ... which decode_at clamped
    m.use_residual_flow = False
    kept = {k: getattr(m, k) for k in RESULTS}
    del calls[:]
    for bad, err in (([0, 5.5], IndexError), ([-1], IndexError), ([], ValueError), ([float("nan")], ValueError)):
        with pytest.raises(err):
            m.decode_at(bad)
    with pytest.raises(ValueError, match="mode"):
        m.decode_at([0, 1], "nearest")
    assert not calls and all(getattr(m, k) is kept[k] for k in RESULTS)
    m.decode_at(torch.tensor([0.5, 0.0]), latent=latent[:, :, :2].contiguous())          # another latent, times as a host tensor
    assert calls == [2] and m.sample_out_vid.shape[2] == 2 and m.sample_latent is latent


# ------------------------------------------------------------------------------------------ 9. fractional times against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_decode_at_twice_the_frame_rate_matches_the_oracle(gpu, mode):
    from cvpr23_lfdm_amd.retime import frame_times
    m, base, img = _sampled(gpu)
    times = frame_times(NF, 2)
    m.decode_at(times, mode)
    latent = base["sample_latent"].cpu()
    want_latent = _reference(latent, times, mode)[0]
    if mode == "cubic":          # decode_at clamps the interpolated occlusion channel
        want_latent[:, 2, 1::2] = want_latent[:, 2, 1::2].clamp(-1, 1)
    want_out, want_warped = _oracle_decode(want_latent.float(), img)
    assert tuple(m.sample_out_vid.shape) == tuple(m.sample_warped_vid.shape) == (1, 3, 2 * NF - 1, HW, HW)
    assert tuple(m.sample_vid_grid.shape) == (1, 2, 2 * NF - 1, S, S) and tuple(m.sample_vid_conf.shape) == (1, 1, 2 * NF - 1, S, S)
    assert_close(m.sample_out_vid, want_out, 1e-3, "decode_at x2 %s: sample_out_vid" % mode)
    assert_close(m.sample_warped_vid, want_warped, 1e-3, "decode_at x2 %s: sample_warped_vid" % mode)
    assert_close(m.sample_vid_grid, want_latent[:, :2], 1e-5, "decode_at x2 %s: sample_vid_grid" % mode)
    for k in RESULTS:          # the frames at even positions are the sampled ones
        assert torch.equal(getattr(m, k)[:, :, ::2], base[k]), k
    assert torch.equal(m.sample_latent, base["sample_latent"]) and m.sample_latent.shape[2] == NF
    strip = m.render_sample()
    assert tuple(strip.shape) == (1, 2 * NF - 1, HW, 5 * HW, 3)


# ------------------------------------------------------------------------------------------ 10. the frame_times keyword (needs the sampler)
def _resample_now(m, tape):
    m.diffusion.noise_source = synth.NoiseTape(tape)


@pytest.mark.gpu
def test_frame_times_keyword_of_sample_one_video(gpu):
    from cvpr23_lfdm_amd import FlowDiffusionFunctional, io_compat as IO
    from cvpr23_lfdm_amd.retime import frame_times
    m, base, img = _sampled(gpu)
    times = frame_times(NF, 2, pingpong=True)
    _resample_now(m, 5)
    m.sample_one_video(cond_scale=1.0, frame_times=times, interp="cubic")
    got = {k: getattr(m, k).clone() for k in RESULTS}
    assert torch.equal(m.sample_latent, base["sample_latent"])          # sampled as without the keyword
    m.decode_at(times, "cubic", latent=base["sample_latent"])
    for k in RESULTS:
        assert got[k].shape[2] == len(times) == 4 * NF - 4 and torch.equal(got[k], getattr(m, k)), k
    assert len(IO.video_strip_device(m, img.cuda(), indexed=True)) == len(times)
    # bad times are refused before the sampler runs
    m.sample_latent = None
    with pytest.raises(IndexError):
        m.sample_one_video(cond_scale=1.0, frame_times=[0, NF])
    assert m.sample_latent is None
    # the functional flavour returns the same tensors
    _resample_now(m, 5)
    res = FlowDiffusionFunctional.sample_one_video(m, img.cuda(), m.sample_text, 1.0, frame_times=times, interp="cubic")
    for k in RESULTS:
        assert torch.equal(res[k], got[k]), k
    assert torch.equal(res["sample_latent"], base["sample_latent"])


@pytest.mark.gpu
def test_frame_times_keyword_of_sample_long_video(gpu):
    from cvpr23_lfdm_amd.retime import frame_times
    m, _, _ = _sampled(gpu)
    total = 13
    times = frame_times(total, 2)          # 25 frames: four decode pieces of at most 8
    _resample_now(m, 6)
    m.sample_long_video(1.0, total, overlap=3)
    plain = {k: getattr(m, k).clone() for k in RESULTS + ("sample_latent",)}
    m.decode_at(times)
    after = {k: getattr(m, k).clone() for k in RESULTS}
    _resample_now(m, 6)
    m.sample_long_video(1.0, total, overlap=3, frame_times=times)
    assert torch.equal(m.sample_latent, plain["sample_latent"]) and m.sample_latent.shape[2] == total
    for k in RESULTS:
        assert getattr(m, k).shape[2] == 2 * total - 1 and torch.equal(getattr(m, k), after[k]), k
        assert torch.equal(after[k][:, :, ::2], plain[k]), k
    assert tuple(m.render_sample(panels=("out", "flow", "conf")).shape) == (1, 2 * total - 1, HW, 3 * HW, 3)
    with pytest.raises(IndexError):
        m.sample_long_video(1.0, total, overlap=3, frame_times=[total - 0.5])


# ------------------------------------------------------------------------------------------ 11. evaluate.interpolation_error
T_EVAL, NF_EVAL = 9, 5          # nine frames through a model that decodes five at a time: two pieces


def _eval_model(dev, lat):
    """The synthetic model with its region and background predictors, so the frozen-LFAE pass is real (128 x 128 frames: the region
    predictor's five halvings)."""
    m = synth.build_flow_diffusion(dev, img_size=lat, num_frames=NF_EVAL, sampling_timesteps=4)[0]
    m.region_predictor.load_state_dict(synth.region_state())
    m.bg_predictor.load_state_dict(synth.bg_state())
    return m.eval()


@pytest.mark.gpu
def test_interpolation_error(gpu):
    from cvpr23_lfdm_amd import evaluate as E
    lat = 32
    m = _eval_model(gpu, lat)
    ref_img, real_vid = synth.train_inputs(1, T_EVAL, 4 * lat)[:2]
    ref_img, real_vid = ref_img.to(gpu), real_vid.to(gpu)
    m.sample_out_vid = "kept"
    for mode, factor in (("linear", 2), ("cubic", 4)):
        res = E.interpolation_error(m, real_vid, ref_img, factor=factor, mode=mode)
        assert set(res) == {"flow", "video", "interp_vs_real", "lfae_vs_real", "held_out"}
        mask = res["held_out"]
        assert mask.dtype == torch.bool and mask.tolist() == [j % factor != 0 for j in range(T_EVAL)]
        if factor == 2:
            assert torch.nonzero(mask).flatten().tolist() == [1, 3, 5, 7]
        flow = res["flow"]["table"].cpu()
        assert flow.dtype == torch.float64 and tuple(flow.shape) == (1, T_EVAL, 2)
        assert bool((flow[:, ~mask] == 0.0).all())                       # kept frames are copies: exactly 0
        assert bool((flow[:, mask, 0] > 0).all()) and bool(torch.isfinite(flow).all())
        for k in ("video", "interp_vs_real", "lfae_vs_real"):
            t = res[k]["table"].cpu()
            assert t.dtype == torch.float64 and tuple(t.shape) == (1, T_EVAL, 3) and bool(torch.isfinite(t).all()), k
        video = res["video"]["table"].cpu()
        assert bool((video[:, ~mask, :2] == 0.0).all()) and bool((video[:, ~mask, 2] == 1.0).all())
        assert bool((video[:, mask, 0] > 0).all())
        assert res["flow"]["summary"]["frames"] == T_EVAL and res["video"]["summary"]["identical_frames"] == int((~mask).sum())
    assert m.sample_out_vid == "kept"                                    # the sample attributes are put back
    with pytest.raises(ValueError, match="divides"):
        E.interpolation_error(m, real_vid, ref_img, factor=3)
    with pytest.raises(ValueError, match="divides"):
        E.interpolation_error(m, real_vid, ref_img, factor=0)


def _eval_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("lfdm_eval_tool_interp", os.path.join(REPO, "tools", "eval.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_eval_tool_interp_flags_parse():
    tool = _eval_tool()
    args = tool.build_parser().parse_args(["interp", "--synthetic"])
    assert args.command == "interp" and args.factor == 2 and args.interp == "linear" and args.frames == 40
    args = tool.build_parser().parse_args(["interp", "--factor", "4", "--interp", "cubic", "--dataset", "mhad"])
    assert args.factor == 4 and args.interp == "cubic"
    with pytest.raises(SystemExit):
        tool.build_parser().parse_args(["interp", "--interp", "nearest"])


@pytest.mark.gpu
def test_eval_tool_interp_synthetic(gpu, tmp_path):
    import json
    tool = _eval_tool()
    lat = 32
    path = str(tmp_path / "interp.json")
    out = tool.main(["interp", "--synthetic", "--size", str(4 * lat), "--frames", "6", "--factor", "2", "--interp", "cubic", "--out", path])
    with open(path) as f:
        disk = json.load(f)
    assert disk == json.loads(json.dumps(out)) and disk["command"] == "interp"
    assert disk["factor"] == 2 and disk["interp"] == "cubic" and disk["frames_used"] == 5
    assert disk["flow"]["frames"] == 10 and disk["flow"]["videos"] == 2 and disk["flow"]["epe"] > 0
    assert disk["held_out"]["flow"]["frames"] == 4 and disk["held_out"]["flow"]["epe"] > disk["flow"]["epe"]
    for k in ("video", "interp_vs_real", "lfae_vs_real"):
        assert disk[k]["frames"] == 10 and disk["held_out"][k]["frames"] == 4


# ------------------------------------------------------------------------------------------ 12. frame_times, demo flags
def test_frame_times():
    from cvpr23_lfdm_amd.retime import frame_times
    assert frame_times(40) == [float(j) for j in range(40)]
    for t, k in ((40, 4), (8, 2), (2, 3), (1, 5), (13, 2)):
        ft = frame_times(t, k)
        assert len(ft) == (t - 1) * k + 1 and ft[0] == 0.0 and ft[-1] == t - 1 and ft == sorted(ft)
        assert ft[::k] == [float(j) for j in range(t)]                   # the sampled instants are exact integers
        assert all(abs(ft[j] - j / k) < 1e-12 for j in range(len(ft)))
    assert len(frame_times(40, 4)) == 157
    rev = frame_times(8, 2, reverse=True)
    assert rev == frame_times(8, 2)[::-1] and rev[0] == 7.0 and rev[-1] == 0.0
    pp = frame_times(8, 2, pingpong=True)
    assert len(pp) == 2 * 15 - 2 and pp[:15] == frame_times(8, 2) and pp[15:] == frame_times(8, 2)[-2:0:-1] and pp[-1] == 0.5
    assert frame_times(8, 2, reverse=True, pingpong=True)[:15] == rev
    assert frame_times(1, 3, pingpong=True) == [0.0] and frame_times(2, 1, pingpong=True) == [0.0, 1.0]
    slow = frame_times(5, speed=0.5)
    assert slow == [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0]
    fast = frame_times(8, speed=2)
    assert fast == [0.0, 2.0, 4.0, 6.0]                                  # the end point only when a step lands on it
    assert frame_times(8, 2, speed=3) == [0.0, 1.5, 3.0, 4.5, 6.0]
    odd = frame_times(40, 3, speed=0.7)
    assert odd[0] == 0.0 and 39 - 0.7 / 3 < odd[-1] <= 39 and all(b > a for a, b in zip(odd, odd[1:]))
    for ft in (pp, slow, fast, odd, frame_times(40, 4, reverse=True, pingpong=True)):
        assert all(isinstance(v, float) and 0.0 <= v for v in ft)
    assert max(odd) <= 39 and max(pp) <= 7 and max(slow) <= 4
    for bad in (dict(num_frames=0), dict(num_frames=4, factor=0), dict(num_frames=4, factor=1.5), dict(num_frames=4, speed=0),
                dict(num_frames=4, speed=float("nan")), dict(num_frames=4, speed=-1)):
        with pytest.raises(ValueError):
            frame_times(**bad)


def test_demo_retime_flags_parse():
    import importlib.util
    spec = importlib.util.spec_from_file_location("lfdm_demo_tool_retime", os.path.join(REPO, "tools", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    args = demo.build_parser().parse_args([])
    assert args.fps_factor == 1 and args.interp == "linear" and not args.pingpong and not args.reverse
    assert demo.retime(args, 40) is None
    args = demo.build_parser().parse_args(["--fps-factor", "4", "--interp", "cubic", "--render", "device", "--gif", "indexed"])
    demo.check_args(args)
    assert args.fps_factor == 4 and args.interp == "cubic" and len(demo.retime(args, 40)) == 157
    args = demo.build_parser().parse_args(["--pingpong", "--reverse", "--total-frames", "112"])
    assert len(demo.retime(args, 112)) == 222 and demo.retime(args, 112)[0] == 111.0
    with pytest.raises(SystemExit):
        demo.check_args(demo.build_parser().parse_args(["--fps-factor", "0"]))
    with pytest.raises(SystemExit):
        demo.build_parser().parse_args(["--interp", "nearest"])
