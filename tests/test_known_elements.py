"""Per-element known masks and start-from-latent sampling.  Seven groups: one and two steps of each op with an element mask
against the same call without the known operands; a frame-constant element mask against the frame-mask op; the conditioning acting on data
with a closed-form predictor; entering the schedule on a latent; whole videos against a loop over the oracle's own pieces; the plumbing on the
GPU; the wrapper.

Every formula is written out again here (numpy / torch double) from the contract, not imported from the package."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import lfdm_oracle as O
import synth
from util import assert_close, rnd


def big(dev):
    return dev == "cuda"


def diffusion(sampler, steps, total=1000, **kw):
    from cvpr23_lfdm_amd import GaussianDiffusion
    return GaussianDiffusion(torch.nn.Identity(), image_size=8, num_frames=4, timesteps=total, sampling_timesteps=steps,
                             loss_type="l2", sampler=sampler, **kw)


def ms_levels(total, steps):
    """[(alpha, sigma)] in double, steps + 1 rows: the node of x_T on alphas_cumprod[time of the first step], after step i on
    alphas_cumprod[time_next], the end of the last step on a = 1.  Row k is the level the latent sits on in front of step k."""
    acp = O.make_schedule(total)["alphas_cumprod"].double().numpy()
    pairs = O.ddim_time_pairs(total, steps)
    a = [acp[pairs[0][0]]] + [1.0 if i == len(pairs) - 1 else acp[tn] for i, (_, tn) in enumerate(pairs)]
    return np.array([(math.sqrt(v), math.sqrt(1.0 - v)) for v in a])


# ------------------------------------------------------------------------------------------ 1. one and two steps of each op
def _elem_masks(shape):
    """Sample 0: a fixed pseudo-random pattern of about 30 % that includes element 0 and element n - 1; sample 1 all False; sample 2 all True."""
    batch = shape[0]
    n = int(np.prod(shape[1:]))
    m = torch.zeros(batch, n, dtype=torch.bool)
    m[0] = torch.from_numpy(np.random.Generator(np.random.PCG64(99)).random(n) < 0.3)
    m[0, 0] = True
    m[0, n - 1] = True
    if batch > 2:
        m[2] = True
    return m.reshape(shape).contiguous()


def _known_pair(shape, mask, seed):
    """(known, known_noise): finite at the masked elements, NaN at every other element."""
    k, z = rnd(*shape, seed=seed), rnd(*shape, seed=seed + 1)
    nan = torch.full(shape, float("nan"))
    return torch.where(mask, k, nan), torch.where(mask, z, nan)


def _check_select(x, ref_plain, k, z, a, s, mask, what):
    assert torch.isfinite(x).all(), what
    assert torch.equal(x[~mask], ref_plain[~mask]), "%s: an unmasked element differs from the plain call" % what
    if mask.any():
        want = a * k[mask].double() + s * z[mask].double()
        err = (x[mask].double() - want).abs()
        print("%s: masked elements max |x - (a k + s n)| %.3e" % (what, float(err.max())))
        assert bool((err <= 1e-6 * want.abs().clamp_min(1.0)).all()), (what, float(err.max()))
        if (a, s) == (1.0, 0.0):
            assert torch.equal(x[mask], k[mask]), "%s: (1, 0) row does not return the known elements bit for bit" % what


SHAPES = [(3, 5, 71), (3, 7, 57143)]


def _tables(op):
    if op == "step_ms":
        table = torch.tensor([[9.] * 6, [2.0, 0.5, 0.8125, 0.37, 0.0, 0.0], [0.5, 0.25, 0.9, 0.61, -0.23, 0.0]])
    else:
        table = torch.tensor([[9.] * 6, [2.0, 0.5, 0.9, 0.3, 0.0, 0.4], [0.5, 0.25, 0.7, 0.0, 0.2, 0.0]])
    return table, torch.tensor([[9., 9.], [9., 9.], [0.8125, 0.59], [1.0, 0.0]])


def _two_steps(dev, op, q, shape, kf_of, x, e1, e2, z1):
    """Steps 1 and 2 of `op` on one workspace, once with the known operands kf_of(True) and once with kf_of(False) (the second step of both
    starts from the state the first conditioned step left).  -> {(known, step): (x, x0_out, second, step counter)}."""
    from cvpr23_lfdm_amd import ops
    batch, n = shape[0], int(np.prod(shape[1:]))
    ms, counter = op == "step_ms", op == "step_counter"
    table, _ = _tables(op)
    seeds = ops.seeds_tensor([(1 << 63) + 5, 17, 3][:batch], dev) if counter else None
    window = torch.full((1,), 2, dtype=torch.int32).to(dev) if counter else None

    def call(xd, eps, second, step, ws, x0_out, known):
        kw = dict(quantile=q, x0_out=x0_out, ws=ws, **kf_of(known))
        if ms:
            ops.sampler_step_ms(xd, eps.to(dev), second, table.to(dev), step, **kw)
        elif counter:
            ops.sampler_step(xd, eps.to(dev), None, table.to(dev), step, seeds=seeds, window=window, **kw)
        else:
            ops.sampler_step(xd, eps.to(dev), second, table.to(dev), step, **kw)

    out, state = {}, {}
    for known in (True, False):
        xd = x.clone().to(dev)
        second = torch.full(shape, float("nan")).to(dev) if ms else z1.to(dev)
        step = torch.tensor([1], dtype=torch.int32).to(dev)
        ws = ops.sampler_ws(batch, n, dev)
        o = torch.empty(shape).to(dev)
        call(xd, e1, second, step, ws, o, known)
        out[known, 1] = (xd.cpu().clone(), o.cpu().clone(), second.cpu().clone(), int(step.cpu()[0]))
        state[known] = (xd, second, step, ws)
    state[False][0].copy_(state[True][0])
    if ms:
        state[False][1].copy_(state[True][1])
    for known in (True, False):
        xd, sec, step, ws = state[known]
        o = torch.empty(shape).to(dev)
        call(xd, e2, sec, step, ws, o, known)
        out[known, 2] = (xd.cpu().clone(), o.cpu().clone(), sec.cpu().clone(), int(step.cpu()[0]))
    return out


def _step_inputs(shape):
    x, e1, e2, z1 = rnd(*shape, seed=1), rnd(*shape, seed=2), rnd(*shape, seed=3), rnd(*shape, seed=4)
    if shape[0] > 1:
        x[1] *= 0.1
        e1[1] *= 0.1
    return x, e1, e2, z1


@pytest.mark.parametrize("cthw", SHAPES)
@pytest.mark.parametrize("batch", [1, 2, 3])
@pytest.mark.parametrize("dynamic", [True, False])
@pytest.mark.parametrize("op", ["step", "step_ms", "step_counter"])
def test_known_elements_step(backend, op, dynamic, batch, cthw):
    """Two steps in a row on one workspace, each against the same call without the known operands on the same inputs.  3 x 7 x 57143 =
    1 200 003 elements > 8 x 512 x 256: the loop behind the prefetched elements runs.  Batch 3 leaves the folded histogram clear."""
    dev = backend
    c, t, hw = cthw
    n = c * t * hw
    if n > 1 << 20 and not big(dev):
        pytest.skip("above 8 x 512 x 256 elements per sample: GPU only")
    q = 0.9 if dynamic else -1.0
    shape = (batch, c, t, hw)
    _, level = _tables(op)
    x, e1, e2, z1 = _step_inputs(shape)
    mask = _elem_masks(shape)
    k, z = _known_pair(shape, mask, 20)
    kf = dict(known=k.to(dev), known_noise=z.to(dev), elem_mask=mask.to(dev), level=level.to(dev))
    run = lambda: _two_steps(dev, op, q, shape, lambda known: kf if known else {}, x, e1, e2, z1)
    got = run()
    for i, (a, s) in ((1, (0.8125, 0.59)), (2, (1.0, 0.0))):
        xk, ok, hk, sk = got[True, i]
        xp, op_, hp, sp = got[False, i]
        what = "%s %s B=%d n=%d step %d" % (op, "dynamic" if dynamic else "static", batch, n, i)
        assert sk == sp == i + 1, what
        assert torch.equal(ok, op_) and torch.isfinite(ok).all(), "%s: x0_out differs" % what
        if op == "step_ms":
            assert torch.equal(hk, hp) and torch.isfinite(hk).all(), "%s: hist differs" % what
        _check_select(xk, xp, k, z, a, s, mask, what)
    assert not torch.equal(got[True, 1][0][mask], got[False, 1][0][mask]), "the conditioning did nothing"
    again = run()
    for key in got:
        for a, b in zip(got[key][:3], again[key][:3]):
            assert torch.equal(a, b), key


@pytest.mark.parametrize("cthw", SHAPES)
@pytest.mark.parametrize("batch", [1, 2, 3])
def test_known_blend_elem(backend, batch, cthw):
    from cvpr23_lfdm_amd import ops
    dev = backend
    c, t, hw = cthw
    if c * t * hw > 1 << 20 and not big(dev):
        pytest.skip("above 8 x 512 x 256 elements per sample: GPU only")
    shape = (batch, c, t, hw)
    x = rnd(*shape, seed=1)
    mask = _elem_masks(shape)
    k, z = _known_pair(shape, mask, 30)
    for a, s in ((0.3125, 0.95), (1.0, 0.0)):
        outs = []
        for _ in range(2):
            xd = x.clone().to(dev)
            ops.known_blend_elem(xd, k.to(dev), z.to(dev), mask.to(dev), a, s)
            outs.append(xd.cpu())
        assert torch.equal(outs[0], outs[1])
        _check_select(outs[0], x, k, z, a, s, mask, "known_blend_elem B=%d n=%d (%g, %g)" % (batch, c * t * hw, a, s))


def test_known_element_ops_refuse_bad_arguments(backend):
    from cvpr23_lfdm_amd import _native, ops
    dev = backend
    shape = (1, 3, 4, 25)
    x, eps = torch.zeros(shape).to(dev), torch.zeros(shape).to(dev)
    table, step = torch.zeros(1, 6).to(dev), torch.zeros(1, dtype=torch.int32).to(dev)
    level = torch.tensor([[1., 0.], [1., 0.]]).to(dev)
    mask = torch.zeros(shape, dtype=torch.bool).to(dev)
    good = dict(known=x.clone(), known_noise=x.clone(), elem_mask=mask, level=level)
    for drop in good:                                     # all of them or none
        kw = {k: v for k, v in good.items() if k != drop}
        with pytest.raises(ValueError, match="all of them or none"):
            ops.sampler_step(x, eps, None, table, step, quantile=-1.0, **kw)
        with pytest.raises(ValueError, match="all of them or none"):
            ops.sampler_step_ms(x, eps, x.clone(), table, step, quantile=-1.0, **kw)
    fmask = torch.zeros(1, 4, dtype=torch.bool).to(dev)
    for both in (dict(frame_mask=fmask, frames=4), dict(frames=4), dict(frame_mask=fmask)):       # one form or the other
        with pytest.raises(ValueError, match="exclude each other"):
            ops.sampler_step(x, eps, None, table, step, quantile=-1.0, **dict(good, **both))
        with pytest.raises(ValueError, match="exclude each other"):
            ops.sampler_step_ms(x, eps, x.clone(), table, step, quantile=-1.0, **dict(good, **both))
    for bad in (dict(elem_mask=torch.zeros(1, 4, dtype=torch.bool).to(dev)), dict(elem_mask=torch.zeros(shape).to(dev)),
                dict(elem_mask=torch.zeros(1, 3, 4, 24, dtype=torch.bool).to(dev)), dict(known=torch.zeros(1, 3, 4, 24).to(dev)),
                dict(level=torch.zeros(2, 3).to(dev)), dict(known_noise=torch.zeros(shape, dtype=torch.float64).to(dev))):
        with pytest.raises(ValueError):
            ops.sampler_step(x, eps, None, table, step, quantile=-1.0, **dict(good, **bad))
        with pytest.raises(ValueError):
            ops.sampler_step_ms(x, eps, x.clone(), table, step, quantile=-1.0, **dict(good, **bad))
    with pytest.raises(ValueError):
        ops.known_blend_elem(x, x.clone(), x.clone(), fmask, 1.0, 0.0)
    with pytest.raises(ValueError):
        ops.known_blend_elem(x, x.clone(), None, mask, 1.0, 0.0)
    with pytest.raises(ValueError, match="alias"):
        ops.known_blend_elem(x, x.clone(), x, mask, 1.0, 0.0)
    # the C entry points check for themselves: null operands, n outside (0, 2^24)
    lib = _native.library()
    ws = ops.sampler_ws(1, 300, dev)
    args = dict(x=ops._p(x), eps=ops._p(eps), batch=1, n=300, coef=ops._p(table), step_dev=ops._p(step), quantile=-1.0, advance=1, ws=ops._p(ws),
                ws_bytes=ws.numel() * 4)
    known = dict(known=ops._p(good["known"]), known_noise=ops._p(good["known_noise"]), elem_mask=ops._p(mask), level=ops._p(level))
    seeds, window = ops.seeds_tensor([5], dev), torch.zeros(1, dtype=torch.int32).to(dev)
    cargs = dict(args, seeds=ops._p(seeds), window=ops._p(window))
    hist = x.clone()
    margs = dict(args, hist=ops._p(hist), multistep=1)

    def c_step(a, k):
        return lib.lfdm_sampler_step_f32(ctypes.byref(_native.SamplerStepParams(known=_native.KnownOperands(**k), **a)), ops._stream(lib))

    def c_blend(xp, k, n):
        return lib.lfdm_known_blend_f32(xp, ctypes.byref(_native.KnownOperands(**k)), 1.0, 0.0, 1, n, ops._stream(lib))

    for a in (args, margs, cargs):
        for drop in known:
            assert c_step(a, dict(known, **{drop: None})) != 0 and b"must all be given" in lib.lfdm_last_error()
    assert c_step(dict(args, n=1 << 24), known) != 0 and b"2^24" in lib.lfdm_last_error()
    assert c_blend(ops._p(x), dict(known, elem_mask=None, level=None), 300) != 0
    assert c_blend(ops._p(x), dict(known, level=None), 1 << 24) != 0
    assert c_blend(None, dict(known, level=None), 300) != 0
    # the combinations that only the parameter struct can express: each one LFDM_EINVAL
    fmask_p = ops._p(fmask)
    noise = x.clone()
    for a, k, words in ((dict(args, seeds=ops._p(seeds)), {}, b"seeds"), (dict(args, window=ops._p(window)), {}, b"seeds"),
                        (dict(cargs, noise=ops._p(noise)), {}, b"exclude each other"), (dict(cargs, noise=ops._p(noise)), known, b"exclude each other"),
                        (dict(margs, seeds=ops._p(seeds), window=ops._p(window)), {}, b"the multistep update draws nothing"),
                        (dict(margs, seeds=ops._p(seeds), window=ops._p(window)), known, b"the multistep update draws nothing"),
                        (args, dict(known, frame_mask=fmask_p), b"exclude each other"),
                        (margs, dict(known, frame_mask=fmask_p, frames=4, frame_elems=25), b"exclude each other"),
                        (args, dict(known, frames=4), b"frames"), (cargs, dict(known, frame_elems=25), b"frame_elems"),
                        (margs, dict(known, frames=4, frame_elems=25), b"frames"),
                        (args, dict(frames=4, frame_elems=25), b"must all be given"), (args, dict(level=ops._p(level)), b"must all be given"),
                        (cargs, dict(known=known["known"], known_noise=known["known_noise"], level=known["level"], frames=4, frame_elems=25),
                         b"must all be given")):
        assert c_step(a, k) == -1 and words in lib.lfdm_last_error(), (a, k, lib.lfdm_last_error())
    for k in (dict(known, level=None, frame_mask=fmask_p), dict(known, level=None, frames=4), dict(known, level=None, frame_elems=25),
              dict(frames=4, frame_elems=25), {}):
        assert c_blend(ops._p(x), k, 300) == -1, k
    assert int(step.cpu()[0]) == 0 and not x.cpu().any()                # nothing ran


# ------------------------------------------------------------------------------------------ 2. a frame-constant element mask is the frame mask
@pytest.mark.parametrize("cthw", SHAPES)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("op", ["step", "step_ms", "step_counter"])
def test_frame_constant_element_mask_is_the_frame_mask(backend, op, batch, cthw):
    from cvpr23_lfdm_amd import ops
    dev = backend
    c, t, hw = cthw
    n = c * t * hw
    if n > 1 << 20 and not big(dev):
        pytest.skip("above 8 x 512 x 256 elements per sample: GPU only")
    shape = (batch, c, t, hw)
    _, level = _tables(op)
    x, e1, e2, z1 = _step_inputs(shape)
    fmask = torch.zeros(batch, t, dtype=torch.bool)
    fmask[0, 0] = True
    fmask[0, t - 2] = True
    if batch > 2:
        fmask[2] = True
    emask = fmask[:, None, :, None].expand(shape).contiguous()
    k, z = _known_pair(shape, emask, 20)
    common = dict(known=k.to(dev), known_noise=z.to(dev), level=level.to(dev))
    elem = dict(common, elem_mask=emask.to(dev))
    frame = dict(common, frame_mask=fmask.to(dev), frames=t)
    got = _two_steps(dev, op, 0.9, shape, lambda first: elem if first else frame, x, e1, e2, z1)
    for i in (1, 2):
        for name, a, b in zip(("x", "x0_out", "second"), got[True, i][:3], got[False, i][:3]):
            if name == "second" and op != "step_ms":
                continue
            assert torch.equal(a, b) and torch.isfinite(a).all(), "%s B=%d n=%d step %d: %s differs from the frame-mask op" % (op, batch, n, i, name)
        assert got[True, i][3] == got[False, i][3] == i + 1
    xa, xb = x.clone().to(dev), x.clone().to(dev)
    ops.known_blend_elem(xa, elem["known"], elem["known_noise"], elem["elem_mask"], 0.3125, 0.95)
    ops.known_blend(xb, frame["known"], frame["known_noise"], frame["frame_mask"], 0.3125, 0.95, t)
    assert torch.equal(xa.cpu(), xb.cpu())


# ------------------------------------------------------------------------------------------ 3. the conditioning acts
MU, SD = 0.3, 0.2
FRAMES, PIXELS = 8, 4096


def _shared_eps(x, al, sg):
    """Optimal eps predictor when all F frames of a pixel share ONE value z ~ N(MU, SD^2): x (F, P) -> eps (F, P)."""
    f = x.shape[0]
    z_hat = (MU / SD ** 2 + al * x.sum(axis=0, keepdims=True) / sg ** 2) / (1.0 / SD ** 2 + f * al ** 2 / sg ** 2)
    return (x - al * z_hat) / sg


def _shared_draws():
    """The draw of test_known_frames' closed-form set-up (seed 42: its 4096 values of N(0.3, 0.2^2) stay below 1): k (P,), x_T, known noise."""
    rng = np.random.Generator(np.random.PCG64(42))
    k = MU + SD * rng.standard_normal(PIXELS)
    return k, rng.standard_normal((FRAMES, PIXELS)), rng.standard_normal((FRAMES, PIXELS))


def _checker_mask():
    """Frames 0-3 known at the even pixels, frames 4-7 at the odd ones: no frame mask expresses it."""
    mask = np.zeros((FRAMES, PIXELS), dtype=bool)
    mask[:4, 0::2] = True
    mask[4:, 1::2] = True
    return mask


def _drive(dev, steps, mask=None, start_step=None):
    """dpmpp_1 on the shared-value data.  mask (F, P) bool: known elements (their value: k of the pixel).  start_step: the schedule is entered
    in front of that step on a * start + s * z, start = the video whose frames all equal k.  -> (the op's final x (F, P), the test's double
    recurrence, k (P,), peak |x0|)."""
    from cvpr23_lfdm_amd import ops
    d = diffusion("dpmpp_1", steps)
    _, coef = d._ms_step_tables("dpmpp_1")
    lv = ms_levels(1000, steps)
    k, x_t, kn = _shared_draws()
    shape = (1, 1, FRAMES, PIXELS)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).reshape(shape).contiguous()
    to64 = lambda t: t.double().numpy().reshape(FRAMES, PIXELS)
    first = 0 if start_step is None else start_step
    xd, x64 = f32(x_t).to(dev), to64(f32(x_t))
    if start_step is not None:
        start32 = f32(np.broadcast_to(k, (FRAMES, PIXELS)))
        z = xd.clone()
        ops.known_blend_elem(xd, start32.to(dev), z, torch.ones(shape, dtype=torch.bool).to(dev), float(np.float32(lv[first, 0])),
                             float(np.float32(lv[first, 1])))
        x64 = lv[first, 0] * to64(start32) + lv[first, 1] * x64
    level = torch.tensor(lv, dtype=torch.float64).float().contiguous()
    kf = {}
    if mask is not None:
        known32 = f32(np.where(mask, np.broadcast_to(k, mask.shape), np.nan))
        kn32 = f32(np.where(mask, kn, np.nan))
        k64, kn64 = to64(known32), to64(kn32)
        kf = dict(known=known32.to(dev), known_noise=kn32.to(dev), elem_mask=torch.from_numpy(mask).reshape(shape).contiguous().to(dev),
                  level=level.to(dev))
        ops.known_blend_elem(xd, kf["known"], kf["known_noise"], kf["elem_mask"], float(level[first, 0]), float(level[first, 1]))
        x64[mask] = lv[first, 0] * k64[mask] + lv[first, 1] * kn64[mask]
    hist = torch.full(shape, float("nan")).to(dev)
    step = torch.full((1,), first, dtype=torch.int32).to(dev)
    ws, coef_dev = ops.sampler_ws(1, FRAMES * PIXELS, dev), coef.to(dev)
    peak = 0.0
    for i in range(first, steps):
        al_s, sg_s = lv[i]
        al_n, sg_n = lv[i + 1]
        eps = _shared_eps(xd.cpu().double().numpy().reshape(FRAMES, PIXELS), al_s, sg_s)
        ops.sampler_step_ms(xd, f32(eps).to(dev), hist, coef_dev, step, quantile=-1.0, ws=ws, **kf)
        e64 = _shared_eps(x64, al_s, sg_s)
        x0 = (x64 - sg_s * e64) / al_s
        peak = max(peak, float(np.abs(x0).max()))
        x64 = (sg_n / sg_s) * x64 + (al_n - sg_n * al_s / sg_s) * np.clip(x0, -1.0, 1.0)
        if mask is not None:
            x64[mask] = al_n * k64[mask] + sg_n * kn64[mask]
    assert int(step.cpu()[0]) == steps
    assert peak < 1.0, "the clamp must stay inactive (max |x0| %.3f)" % peak
    return xd.cpu().double().numpy().reshape(FRAMES, PIXELS), x64, k, peak


@pytest.mark.parametrize("steps", [20, 50])
def test_conditioning_pulls_unknown_elements_to_the_known_ones(backend, steps):
    """F = 8 frames of a pixel share one value; every pixel is known in four of its eight frames (even pixels in frames 0-3, odd pixels in
    frames 4-7).  The unknown elements must end near k: mean |x - k| at most half of the unconditioned run's.  A double numpy model of exactly
    this set-up gives 0.0791 against 0.2178 (ratio 0.363) at 20 steps and 0.0555 against 0.2220 (0.250) at 50, peak |x0| 0.874 / 0.886."""
    dev = backend
    mask = _checker_mask()
    res = {}
    for conditioned in (True, False):
        got, model, k, peak = _drive(dev, steps, mask if conditioned else None)
        assert np.abs(got - model).max() <= 1e-5, (conditioned, np.abs(got - model).max())
        if conditioned:
            want = np.broadcast_to(k.astype(np.float32).astype(np.float64), got.shape)
            assert np.array_equal(got[mask], want[mask])
        res[conditioned] = float(np.abs(got - k)[~mask].mean())
        print("%d steps, %s: unknown elements mean |x - k| %.4f, peak |x0| %.3f"
              % (steps, "conditioned" if conditioned else "unconditioned", res[conditioned], peak))
    print("%d steps: ratio %.3f" % (steps, res[True] / res[False]))
    assert res[True] <= 0.5 * res[False], res


# ------------------------------------------------------------------------------------------ 4. start from a latent
def test_a_later_start_stays_closer_to_its_latent(backend):
    """20 steps, unconditioned; start = the video whose frames all equal k, entered in front of step k0.  The double model gives mean
    |x - start| of 0.2133, 0.1523, 0.0955 and 0.0442 for k0 = 0, 10, 15 and 18 (peak |x0| <= 0.968)."""
    dev = backend
    dist = []
    for k0 in (0, 10, 15, 18):
        got, model, k, peak = _drive(dev, 20, start_step=k0)
        assert np.abs(got - model).max() <= 1e-5, (k0, np.abs(got - model).max())
        dist.append(float(np.abs(got - k).mean()))
        print("start_step %d: mean |x - start| %.4f, peak |x0| %.3f" % (k0, dist[-1], peak))
    assert all(a > b for a, b in zip(dist, dist[1:])), dist


class _Tape:
    """A noise tape that records what was asked of it."""

    def __init__(self, seed):
        self.inner, self.drawn = synth.NoiseTape(seed), []

    def __call__(self, shape):
        self.drawn.append(self.inner(shape))
        return self.drawn[-1]


@pytest.mark.parametrize("elem", [False, True])
@pytest.mark.parametrize("sampler,first", [("reference", 0), ("reference", 3), ("dpmpp_2m", 2)])
def test_start_of_a_video_on_a_tape(backend, sampler, first, elem):
    """`_draw_start` on a hand-made plan: z (the x_T draw) is the first draw, the known noise the second; x = a_k start + s_k z on row k of the
    level table with the known content of row k on top; the step counter starts at k."""
    from cvpr23_lfdm_amd.diffusion import Request, SampleMode
    dev = backend
    d = diffusion(sampler, 5)
    shape = (2, 3, 4, 8, 8)
    lvh = d._level_table(True, sampler)
    new = lambda *s, **kw: torch.zeros(*s, **kw).to(dev)
    plan = dict(x=new(shape), noise=new(shape), step=new(1, dtype=torch.int32), known=new(shape), known_noise=new(shape),
                kmask=new(shape if elem else (2, 4), dtype=torch.bool))
    mode = SampleMode(2, 4, 8, 1, 1.0, True, 5, 0, "fp32", sampler, "torch", -1.0, True, elem)
    assert mode.known and mode.elem == elem
    mask = torch.zeros(shape, dtype=torch.bool)
    if elem:
        mask[:, 2, :, 2:5, 1:4] = True
    else:
        mask[:, :, 1] = True
    start, known = rnd(*shape, seed=5), torch.where(mask, rnd(*shape, seed=6), torch.full(shape, float("nan")))
    req = Request(shape, known.to(dev), (mask if elem else mask[:, 0, :, 0, 0].contiguous()).to(dev), None, 0, start.to(dev), first)
    d.noise_source = tape = _Tape(3)
    d._draw_start(plan, mode, req, lvh, first)
    assert len(tape.drawn) == 2 and int(plan["step"].cpu()[0]) == first
    z, kn = tape.drawn
    a, s = lvh[first].double().tolist()
    got = plan["x"].cpu()
    assert torch.isfinite(got).all()
    want = torch.where(mask, a * known.double() + s * kn.double(), a * start.double() + s * z.double())
    assert float((got.double() - want).abs().max()) <= 1e-6 * float(want.abs().max().clamp_min(1.0))
    # a plain request on the same plan draws x_T straight into x and starts at 0
    d.noise_source = tape = _Tape(3)
    d._draw_start(plan, mode._replace(known=False, elem=False), Request(shape, None, None, None, 0), lvh)
    assert len(tape.drawn) == 1 and torch.equal(plan["x"].cpu(), tape.drawn[0]) and int(plan["step"].cpu()[0]) == 0


def test_request_fields_keep_their_defaults():
    from cvpr23_lfdm_amd.diffusion import Request, SampleMode
    r = Request((1, 3, 4, 8, 8), None, None, None, 0)
    assert r.start is None and r.start_step == 0
    m = SampleMode(1, 4, 8, 1, 1.0, True, 5, 0, "fp32", "reference", "torch", -1.0, False)
    assert m.elem is False and m._fields[-1] == "elem" and Request._fields[-2:] == ("start", "start_step")


def test_sample_refuses_bad_element_and_start_arguments():
    d = diffusion("reference", 10)
    fea, cond = torch.zeros(1, 256, 8, 8), torch.zeros(1, 768)
    shape = (1, 3, 4, 8, 8)
    good = torch.zeros(shape)
    d.denoise_fn = torch.nn.Linear(1, 1)           # (a parameter to read the device from; nothing is launched)
    ok = d.check_request(shape, good, torch.zeros(shape, dtype=torch.bool))
    assert ok.known_mask.dim() == 5
    assert d.check_request(shape, good, torch.zeros(1, 1, 4, 8, 8, dtype=torch.bool)).known_mask.shape[1] == 1
    assert d.check_request(shape, good, torch.zeros(1, 4, dtype=torch.bool)).known_mask.dim() == 2
    assert d.check_request(shape, start=good, start_step=9).start_step == 9
    for m in (torch.zeros(1, 2, 4, 8, 8, dtype=torch.bool), torch.zeros(1, 3, 4, 8, dtype=torch.bool), torch.zeros(shape),
              torch.zeros(1, 3, 4, 8, 7, dtype=torch.bool), torch.zeros(2, 1, 4, 8, 8, dtype=torch.bool), torch.zeros(1, 3, 4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="known_mask"):
            d.sample(fea, cond=cond, known=good, known_mask=m)
    for kw in (dict(start_step=2), dict(start=good, start_step=10), dict(start=good, start_step=-1), dict(start=good, start_step=1.0),
               dict(start=good.double()), dict(start=good[:, :, :3]), dict(start=[0.0]), dict(start=good, start_step=True)):
        with pytest.raises(ValueError, match="start"):
            d.sample(fea, cond=cond, **kw)
        with pytest.raises(ValueError, match="start"):
            d.ddim_sample(fea, shape, cond=cond, **kw)
        if kw.get("start_step") == 10:
            kw = dict(kw, start_step=1000)          # (the ancestral loop has 1000 steps)
        with pytest.raises(ValueError, match="start"):
            d.p_sample_loop(fea, shape, cond=cond, **kw)
    assert d.check_request(shape, start=good, start_step=999, steps=d.num_timesteps).start_step == 999       # (p_sample_loop's schedule)


# ------------------------------------------------------------------------------------------ 5. whole videos against the oracle's pieces
def _skip_slow_emu(dev):
    if dev == "cpu" and os.environ.get("LFDM_EMU_E2E", "0") != "1":
        pytest.skip("end-to-end under the emulator is opt-in (LFDM_EMU_E2E=1); it runs on the GPU")


def oracle_edit_latent(kind, sd, fea, cond, shape, steps, total, cond_scale, noise_fn, known, mask, start=None, start_step=0,
                       draw_known=True, eta=1.0):
    """The sampling loop over the oracle's own pieces + the select of the contract on an element mask (B, C | 1, T, S, S) + the entry on
    `start` in front of step start_step.  kind: "ddim" | "ddpm" | "dpmpp_2m"; the first dpmpp_2m step that runs is first order."""
    b, _, frames, _, _ = shape
    mask = mask.expand(shape)
    x = noise_fn(tuple(shape))
    kn = noise_fn(tuple(shape)) if draw_known else torch.zeros(shape)
    fea_rep = fea.unsqueeze(2).repeat(1, 1, frames, 1, 1)
    first = start_step if start is not None else 0

    def enter(x, a, s):          # (a, s): the level the latent sits on in front of step `first`
        if start is not None:
            x = a * start + s * x
        return torch.where(mask, a * known + s * kn, x)

    def select(x, a, s):
        return torch.where(mask, a * known + s * kn, x)

    if kind == "ddim":
        pairs = O.ddim_time_pairs(total, steps)
        a0 = sd["alphas_cumprod_prev"][pairs[first][0]]
        x = enter(x, a0.sqrt(), (1 - a0).sqrt())
        for time, time_next in pairs[first:]:
            z = noise_fn(tuple(shape)) if time_next > 0 else None
            x, _, _ = O.ddim_step(sd, x, fea_rep, cond, time, time_next, z, eta, cond_scale, True)
            a = sd["alphas_cumprod_prev"][time_next]
            x = select(x, a.sqrt(), (1 - a).sqrt())
    elif kind == "ddpm":
        a0 = sd["alphas_cumprod"][total - 1 - first]
        x = enter(x, a0.sqrt(), (1 - a0).sqrt())
        for time in list(reversed(range(total)))[first:]:
            x, _, _ = O.ddpm_step(sd, x, fea_rep, cond, time, noise_fn(tuple(shape)), cond_scale, True)
            a = sd["alphas_cumprod_prev"][time]
            x = select(x, a.sqrt(), (1 - a).sqrt())
    else:
        lv = ms_levels(total, steps)
        pairs = O.ddim_time_pairs(total, steps)
        if start is not None:
            x = lv[first, 0] * start.double() + lv[first, 1] * x.double()
        x = torch.where(mask, lv[first, 0] * known.double() + lv[first, 1] * kn.double(), x.double()).float()
        m_prev, h_prev = None, None
        for i, (time, _) in list(enumerate(pairs))[first:]:
            last = i == len(pairs) - 1
            (al_s, sg_s), (al_n, sg_n) = lv[i], lv[i + 1]
            t = torch.full((b,), time, dtype=torch.long)
            eps = O.unet_forward_with_cond_scale(sd, torch.cat([x, fea_rep], dim=1), t, cond, cond_scale)
            m = O.dynamic_threshold(O.predict_start_from_noise(sd, x, t, eps)).double()
            k = al_n - sg_n * al_s / sg_s
            h = math.inf if last else math.log(al_n / sg_n) - math.log(al_s / sg_s)
            if i == first or last:
                new = (sg_n / sg_s) * x.double() + k * m
            else:
                r = h_prev / h
                new = (sg_n / sg_s) * x.double() + k * (1 + 1 / (2 * r)) * m - k / (2 * r) * m_prev
            x, m_prev, h_prev = torch.where(mask, al_n * known.double() + sg_n * kn.double(), new).float(), m, h
    return x


def _decode(gsd, img, x, frames):
    grid, conf = x[:, :2], (x[:, 2:3] + 1) * 0.5
    outs, warps = [], []
    for f in range(frames):
        g = O.generator_forward_with_flow(gsd, img, grid[:, :, f].permute(0, 2, 3, 1), conf[:, :, f])
        outs.append(g["prediction"])
        warps.append(g["deformed"])
    return {"sample_vid_grid": grid, "sample_vid_conf": conf, "sample_out_vid": torch.stack(outs, dim=2),
            "sample_warped_vid": torch.stack(warps, dim=2)}


def _strength(steps, start_step):
    """A strength whose start_step = steps - ceil(strength * steps) is `start_step`, away from the rounding edge."""
    return (steps - start_step - 0.5) / steps


def _sizes(dev):
    return dict(b=1, t=4, s=8, hw=32) if dev == "cpu" else dict(b=2, t=8, s=16, hw=64)


def _channel_mask(shape):
    """A box known in all three channels, and a second region where only the occlusion channel (2) is known."""
    mask = torch.zeros(shape, dtype=torch.bool)
    mask[:, :, :, 1:5, 2:6] = True
    mask[:, 2, :, 5:8, 0:3] = True
    return mask


def test_the_edit_loop_is_the_oracles_own():
    """All-False mask, no extra draw, no start: the test's DDIM loop equals O.sample bit for bit (host only, tiny UNet input)."""
    b, t, s, steps, total = 1, 2, 8, 3, 1000
    dsd = {"denoise_fn." + k: v for k, v in synth.unet_state().items()}
    sd = dict(dsd)
    sd.update(O.make_schedule(total))
    img, cond = synth.inputs(b, 32)
    fea = O.generator_compute_fea(synth.generator_state(), img)
    shape = (b, 3, t, s, s)
    mask = torch.zeros(shape, dtype=torch.bool)
    known = torch.full(shape, float("nan"))
    got = oracle_edit_latent("ddim", sd, fea, cond, shape, steps, total, 1.0, synth.NoiseTape(11), known, mask, draw_known=False)
    want = O.sample(sd, fea, cond, shape, steps, total, 1.0, 1.0, synth.NoiseTape(11))
    assert torch.equal(got, want)


@pytest.mark.parametrize("start_step", [0, 2, 5])
@pytest.mark.parametrize("cond_scale", [1.0, 2.0])
@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m", "ddpm"])
def test_sample_one_video_known_elements_and_start(backend, kind, cond_scale, start_step):
    dev = backend
    _skip_slow_emu(dev)
    z = _sizes(dev)
    steps = 6
    total = 6 if kind == "ddpm" else 1000
    m, dsd, gsd = synth.build_flow_diffusion(dev, img_size=z["s"], num_frames=z["t"], sampling_timesteps=steps, timesteps=total,
                                             sampler="dpmpp_2m" if kind == "dpmpp_2m" else "reference")
    assert m.diffusion.is_ddim_sampling == (kind != "ddpm")
    img, cond = synth.inputs(z["b"], z["hw"])
    sd = dict(dsd)
    sd.update(O.make_schedule(total))
    shape = (z["b"], 3, z["t"], z["s"], z["s"])
    mask = _channel_mask(shape)
    known = torch.where(mask, synth.NoiseTape(23)(shape).clamp(-1, 1), torch.full(shape, float("nan"))).contiguous()
    start = synth.NoiseTape(29)(shape).clamp(-1, 1).contiguous()
    fea = O.generator_compute_fea(gsd, img)
    if kind == "ddim" and cond_scale == 1.0 and start_step == 0:       # pins the loop to the oracle that is pinned to the reference, at this size too
        none = torch.zeros_like(mask)
        assert torch.equal(oracle_edit_latent("ddim", sd, fea, cond, shape, steps, total, 1.0, synth.NoiseTape(11), known, none, draw_known=False),
                           O.sample(sd, fea, cond, shape, steps, total, 1.0, 1.0, synth.NoiseTape(11)))
    lat = oracle_edit_latent(kind, sd, fea, cond, shape, steps, total, cond_scale, synth.NoiseTape(11), torch.nan_to_num(known), mask,
                             start=start, start_step=start_step)
    ref = _decode(gsd, img, lat, z["t"])
    sch = m.diffusion._schedule(kind != "ddpm", m.diffusion.sampler, torch.device(dev))
    cached = sch.coef.clone()
    m.diffusion.noise_source = synth.NoiseTape(11)
    m.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))
    m.sample_one_video(cond_scale=cond_scale, known_latent=known.to(dev), known_mask=mask.to(dev), start_latent=start.to(dev),
                       strength=_strength(steps, start_step))
    assert torch.equal(sch.coef, cached) and m.diffusion._schedule(kind != "ddpm", m.diffusion.sampler, torch.device(dev)) is sch
    what = "%s, known elements, start_step %d, cond_scale %g" % (kind, start_step, cond_scale)
    for k in ("sample_vid_grid", "sample_vid_conf", "sample_warped_vid", "sample_out_vid"):
        assert_close(getattr(m, k).cpu(), ref[k], 1e-3, "%s (%s)" % (k, what))
    got = m.sample_latent.cpu()
    assert torch.equal(got[mask], known[mask]), what
    assert float((got[~mask] - start[~mask]).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------ 6. plumbing on the GPU
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvpr23_lfdm_amd import _native
    _native._set_library_for_tests(None)


KW = dict(img_size=8, num_frames=4, sampling_timesteps=7)
SHAPE = (1, 3, 4, 8, 8)


def _box(seed, box, channels=(0, 1, 2), one_channel=False):
    """(known with NaN outside the mask, mask): latent pixels box = (y0, x0, y1, x1) of the given channels, in every frame."""
    k = synth.NoiseTape(100 + seed)(SHAPE).clamp(-1, 1)
    mask = torch.zeros(SHAPE, dtype=torch.bool)
    y0, x0, y1, x1 = box
    mask[:, list(channels), :, y0:y1, x0:x1] = True
    k = torch.where(mask, k, torch.full(SHAPE, float("nan"))).contiguous()
    return k, (mask[:, :1].contiguous() if one_channel else mask)


def _video(m, seed, known=None, mask=None, start=None, start_step=0, tape=True, seeds=None):
    img, cond = synth.inputs(1, 32, seed=seed)
    if tape is True:
        tape = synth.NoiseTape(seed)
    m.diffusion.noise_source = tape or None
    m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
    kw = {}
    if known is not None:
        kw.update(known_latent=known.cuda(), known_mask=mask.cuda())
    if start is not None:
        steps = KW["sampling_timesteps"]
        kw.update(start_latent=start.cuda(), strength=_strength(steps, start_step))
    if seeds is not None:
        kw.update(seeds=seeds)
    m.sample_one_video(cond_scale=1.0, **kw)
    return m.sample_latent.clone()


def _model(sampler, **kw):
    total = kw.pop("timesteps", 1000)
    return synth.build_flow_diffusion("cuda", sampler=sampler, timesteps=total, **dict(KW, **kw))[0]


def _start(seed=7):
    return synth.NoiseTape(200 + seed)(SHAPE).clamp(-1, 1).contiguous()


SAMPLERS = [("reference", {}), ("dpmpp_2m", {}), ("reference", dict(timesteps=7))]       # DDIM, 2M, DDPM on 7 timesteps


@pytest.mark.gpu
@pytest.mark.parametrize("sampler,extra", SAMPLERS)
def test_unconditioned_videos_are_untouched_by_an_element_conditioned_one(sampler, extra):
    _gpu()
    m = _model(sampler, **extra)
    k, mask = _box(5, (1, 2, 6, 7))
    first = _video(m, 5)
    cond = _video(m, 5, k, mask, start=_start(), start_step=2)
    third = _video(m, 5)
    assert torch.equal(first, third)
    assert torch.equal(first, _video(_model(sampler, **extra), 5))
    assert not torch.equal(first, cond) and torch.isfinite(cond).all()
    assert torch.equal(cond.cpu()[mask], k[mask])


@pytest.mark.gpu
@pytest.mark.parametrize("sampler,extra", SAMPLERS)
def test_other_mask_and_other_start_need_no_new_plan_or_capture(sampler, extra, monkeypatch):
    """One element plan, one step graph and one set of chunk graphs serve another mask, a (B, 1, T, S, S) mask, other content and every
    start_step; a frame-conditioned video in between keeps its own plan."""
    _gpu()
    monkeypatch.setenv("LFDM_GRAPH_STEPS", "3")          # 7 steps: chunks 0-2, 3-5, 6; a start at 4 replays single steps 4, 5 and chunk 6
    m = _model(sampler, **extra)
    cases = [(5, (1, 2, 6, 7), (0, 1, 2), False, 0), (6, (0, 0, 3, 8), (2,), False, 4), (5, (2, 2, 5, 5), (0, 1, 2), True, 2),
             (6, (0, 0, 8, 8), (0, 1), False, 6), (5, (1, 2, 6, 7), (0, 1, 2), False, 3)]
    got, graphs = [], None
    for seed, box, ch, one, k0 in cases:
        k, mask = _box(seed, box, ch, one)
        got.append(_video(m, seed, k, mask, start=_start(seed), start_step=k0))
        plans = [p for key, p in m.diffusion._plans.items() if key.elem]
        assert len(plans) == 1
        now = (plans[0]["graph"], dict(plans[0]["chunk_graphs"]))
        if graphs is not None:
            assert now[0] is graphs[0] and now[1].keys() == graphs[1].keys() and all(now[1][f] is graphs[1][f] for f in now[1]), \
                "start_step %d captured again" % k0
        graphs = now
        if len(got) == 2:           # a frame-masked video in between: its own plan, the element plan stays
            fm = torch.zeros(1, 4, dtype=torch.bool)
            fm[:, :2] = True
            _video(m, 5, synth.NoiseTape(105)(SHAPE).clamp(-1, 1).contiguous(), fm)
            assert sorted((key.known, key.elem) for key in m.diffusion._plans) == [(True, False), (True, True)]
    for (seed, box, ch, one, k0), g in zip(cases, got):
        k, mask = _box(seed, box, ch, one)
        assert torch.equal(g, _video(_model(sampler, **extra), seed, k, mask, start=_start(seed), start_step=k0)), (seed, box, k0)
        full = mask.expand(SHAPE)
        assert torch.equal(g.cpu()[full], k[full])
    assert not torch.equal(got[0], got[4])


@pytest.mark.gpu
def test_frame_constant_element_mask_gives_the_frame_masked_video():
    """Whole videos: a 5-D mask that is constant over each frame against the (B, T) mask, all three samplers."""
    _gpu()
    for sampler, extra in SAMPLERS:
        fm = torch.zeros(1, 4, dtype=torch.bool)
        fm[:, [0, 2]] = True
        k = synth.NoiseTape(105)(SHAPE).clamp(-1, 1)
        k = torch.where(fm[:, None, :, None, None], k, torch.full(SHAPE, float("nan"))).contiguous()
        a = _video(_model(sampler, **extra), 5, k, fm)
        b = _video(_model(sampler, **extra), 5, k, fm[:, None, :, None, None].expand(SHAPE).contiguous())
        c = _video(_model(sampler, **extra), 5, k, fm[:, None, :, None, None].expand(1, 1, 4, 8, 8).contiguous())
        assert torch.equal(a, b) and torch.equal(a, c), sampler


@pytest.mark.gpu
def test_graph_chunks_do_not_change_an_edited_video(monkeypatch):
    _gpu()
    k, mask = _box(5, (1, 2, 6, 7))
    outs = {}
    for steps in ("1", "10"):
        monkeypatch.setenv("LFDM_GRAPH_STEPS", steps)
        m = _model("dpmpp_2m")
        a = [_video(m, 5, k, mask, start=_start(), start_step=k0) for k0 in (0, 3)]
        m = _model("reference")                                 # DDIM eta 1 with torch's generator under a fixed seed
        b = []
        for k0 in (0, 3, 3):
            torch.manual_seed(77)
            b.append(_video(m, 5, k, mask, start=_start(), start_step=k0, tape=False))
        assert torch.equal(b[1], b[2]) and not torch.equal(b[0], b[1])
        outs[steps] = a + b
    for x, y in zip(outs["1"], outs["10"]):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_started_videos_draw_only_for_the_steps_they_run():
    _gpu()
    m = _model("reference")                     # DDIM, 7 steps: the last one draws nothing
    k, mask = _box(5, (1, 2, 6, 7))
    for k0, known, want in ((0, True, 2 + 6), (3, True, 2 + 3), (6, True, 2), (3, False, 1 + 3)):
        tape = _Tape(5)
        _video(m, 5, k if known else None, mask if known else None, start=_start(), start_step=k0, tape=tape)
        assert len(tape.drawn) == want, (k0, known, len(tape.drawn))


@pytest.mark.gpu
def test_dpmpp_2m_start_leaves_the_cached_tables():
    _gpu()
    m = _model("dpmpp_2m")
    sch = m.diffusion._schedule(True, "dpmpp_2m", torch.device("cuda"))
    coef = sch.coef.clone()
    assert float(coef[3, 4]) != 0.0                                   # row 3 is second order in the schedule
    a = _video(m, 5, start=_start(), start_step=3)
    assert torch.equal(sch.coef, coef) and m.diffusion._schedule(True, "dpmpp_2m", torch.device("cuda")) is sch
    full = _video(m, 5)                                               # the plan's copy is rewritten by every call
    assert torch.equal(full, _video(_model("dpmpp_2m"), 5))
    assert torch.equal(a, _video(m, 5, start=_start(), start_step=3))


@pytest.mark.gpu
def test_known_elements_compose_with_bf16_convolutions():
    _gpu()
    k, mask = _box(5, (1, 2, 6, 7))
    a = _video(_model("dpmpp_2m", conv_precision="bf16"), 5, k, mask, start=_start(), start_step=2)
    b = _video(_model("dpmpp_2m"), 5, k, mask, start=_start(), start_step=2)
    assert torch.isfinite(a).all() and not torch.equal(a, b)
    assert torch.equal(a.cpu()[mask], k[mask])


@pytest.mark.gpu
@pytest.mark.parametrize("sampler,extra", [("reference", {}), ("reference", dict(timesteps=7))])
def test_counter_edit_is_the_default_path_on_its_tape(sampler, extra):
    """noise="counter": an element-masked, started video against noise="torch" replaying counter_tape(..., known=True, start_step=k)."""
    _gpu()
    k, mask = _box(5, (1, 2, 6, 7))
    seeds = [(1 << 63) + 11]
    mc = _model(sampler, noise="counter", **extra)
    mt = _model(sampler, **extra)
    for k0 in (0, 3):
        got = _video(mc, 5, k, mask, start=_start(), start_step=k0, tape=False, seeds=seeds)
        tape = mt.diffusion.counter_tape(seeds, SHAPE, mt.diffusion.is_ddim_sampling, known=True, start_step=k0)
        want = _video(mt, 5, k, mask, start=_start(), start_step=k0, tape=tape)
        assert torch.isfinite(got).all() and torch.equal(got, want), k0
        with pytest.raises(IndexError):
            tape(SHAPE)                                                # every draw of the tape was used


@pytest.mark.gpu
def test_an_edited_video_is_its_seed():
    """noise="counter": the edited video of seed s alone and as the second of three agrees within 2e-3 (the bar of test_counter_noise)."""
    _gpu()
    k, mask = _box(5, (1, 2, 6, 7))
    start = _start()
    m = _model("reference", noise="counter")
    img, cond = synth.inputs(1, 32, seed=5)

    def run(seeds):
        b = len(seeds)
        m.set_sample_input(sample_img=img.expand(b, -1, -1, -1).contiguous().cuda(), sample_text=cond.expand(b, -1).contiguous().cuda())
        m.sample_one_video(cond_scale=1.0, known_latent=k.expand(b, -1, -1, -1, -1).contiguous().cuda(),
                           known_mask=mask.expand(b, -1, -1, -1, -1).contiguous().cuda(),
                           start_latent=start.expand(b, -1, -1, -1, -1).contiguous().cuda(), strength=_strength(7, 2), seeds=seeds)
        return {n: getattr(m, n).cpu().clone() for n in ("sample_latent", "sample_out_vid")}

    alone, three = run([77]), run([5, 77, (1 << 63) + 11])
    for n in alone:
        assert_close(three[n][1:2], alone[n], 2e-3, "%s of seed 77 alone and second of three" % n)
    assert float((three["sample_latent"][0] - three["sample_latent"][1])[~mask[0]].abs().mean()) > 1e-2


# ------------------------------------------------------------------------------------------ 7. the wrapper
S_LFAE, NF_LFAE = 32, 4          # the frozen-LFAE pass needs 128 x 128 frames (the region predictor's five halvings of the quarter-scale frame)


def _lfae_model(dev, **kw):
    m = synth.build_flow_diffusion(dev, img_size=S_LFAE, num_frames=NF_LFAE, sampling_timesteps=4, **kw)[0]
    m.region_predictor.load_state_dict(synth.region_state())
    m.bg_predictor.load_state_dict(synth.bg_state())
    return m.eval()


@pytest.mark.parametrize("residual", [False, True])
def test_encode_video_and_a_full_mask_return_the_video(backend, residual):
    """encode_video is the latent of forward()'s real_vid_grid / real_vid_conf; sampled with that latent as start AND as known content under an
    all-True mask, the model returns it bit for bit and decodes it to real_out_vid."""
    dev = backend
    _skip_slow_emu(dev)
    m = _lfae_model(dev, use_residual_flow=residual)
    ref_img, real_vid, cond = synth.train_inputs(1, NF_LFAE, 4 * S_LFAE)[:3]
    m.set_train_input(ref_img=ref_img.to(dev), real_vid=real_vid.to(dev), ref_text=cond.to(dev))
    m.forward()
    grid, conf = m.real_vid_grid.clone(), m.real_vid_conf.clone()
    if residual:
        grid = grid - O.identity_grid(1, NF_LFAE, S_LFAE, S_LFAE).to(dev)
    want = torch.cat((grid, conf * 2 - 1), dim=1)
    real_out = m.real_out_vid.clone()
    lat = m.encode_video(real_vid.to(dev), ref_img.to(dev))
    assert tuple(lat.shape) == (1, 3, NF_LFAE, S_LFAE, S_LFAE) and lat.is_contiguous() and torch.equal(lat, want)
    was = m.is_train
    m.is_train = not was                                   # (independent of is_train: nothing of the diffusion runs)
    assert torch.equal(m.encode_video(real_vid.to(dev), ref_img.to(dev)), lat)
    m.is_train = was
    m.diffusion.noise_source = synth.NoiseTape(5)
    m.set_sample_input(sample_img=ref_img.to(dev), sample_text=cond.to(dev))
    m.sample_one_video(1.0, known_latent=lat, known_mask=torch.ones(lat.shape, dtype=torch.bool).to(dev), start_latent=lat, strength=0.5)
    assert torch.equal(m.sample_latent, lat)
    assert_close(m.sample_out_vid.cpu(), real_out.cpu(), 1e-3, "decode of the returned latent against real_out_vid")


def test_wrappers_refuse_bad_edit_arguments():
    from cvpr23_lfdm_amd import FlowDiffusion
    from cvpr23_lfdm_amd.flow_diffusion import FlowDiffusionFunctional
    lat = torch.zeros(1, 3, 8, 8, 8)
    for cls in (FlowDiffusion, FlowDiffusionFunctional):
        m = cls(img_size=8, num_frames=8, sampling_timesteps=7, is_train=False, config_pth=synth.CONFIG)
        img, text = torch.zeros(1, 3, 32, 32), torch.zeros(1, 768)
        if cls is FlowDiffusion:
            m.set_sample_input(sample_img=img, sample_text=text)
            call = lambda **kw: m.sample_one_video(1.0, **kw)
        else:
            call = lambda **kw: m.sample_one_video(img, text, 1.0, **kw)
        with pytest.raises(ValueError, match="go together"):
            call(start_latent=lat)
        with pytest.raises(ValueError, match="go together"):
            call(strength=0.5)
        for bad in (0.0, -0.1, 1.5, "half", True, float("nan")):
            with pytest.raises(ValueError, match="strength"):
                call(start_latent=lat, strength=bad)
        with pytest.raises(ValueError, match="start"):
            call(start_latent=lat[:, :2], strength=0.5)
        with pytest.raises(ValueError, match="known_mask"):
            call(known_latent=lat, known_mask=torch.zeros(1, 2, 8, 8, 8, dtype=torch.bool))
        with pytest.raises(ValueError, match="go together"):
            call(known_mask=torch.zeros(1, 3, 8, 8, 8, dtype=torch.bool))


def test_strength_picks_the_start_step(monkeypatch):
    """start_step = steps - ceil(strength * steps)."""
    from cvpr23_lfdm_amd import FlowDiffusion
    m = FlowDiffusion(img_size=8, num_frames=8, sampling_timesteps=7, is_train=False, config_pth=synth.CONFIG)
    m.set_sample_input(sample_img=torch.zeros(1, 3, 32, 32), sample_text=torch.zeros(1, 768))
    seen = []

    class Stop(Exception):
        pass

    def check_request(*a, **kw):
        seen.append(a[6])
        raise Stop()

    monkeypatch.setattr(m.diffusion, "check_request", check_request)
    lat = torch.zeros(1, 3, 8, 8, 8)
    for strength, want in ((1.0, 0), (1, 0), (0.5, 3), (6 / 7, 1), (0.86, 0), (0.01, 6), (1 / 7, 6), (0.15, 5), (3 / 7, 4), (0.7, 2)):
        with pytest.raises(Stop):
            m.sample_one_video(1.0, start_latent=lat, strength=strength)
        assert seen[-1] == want, (strength, seen[-1])


def test_edit_demo_flags_parse():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "demo.py")
    spec = importlib.util.spec_from_file_location("lfdm_demo_tool_edit", path)
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    args = demo.build_parser().parse_args([])
    assert args.from_video == "" and args.strength is None and args.keep_box == "" and args.regen_box == ""
    args = demo.build_parser().parse_args(["--synthetic", "--from-video", "frames", "--strength", "0.5", "--keep-box", "0,0,16,32"])
    assert args.from_video == "frames" and args.strength == 0.5 and demo.parse_box(args.keep_box, 32) == (0, 0, 16, 32)
    assert demo.parse_box("4,4,8,8", 32) == (4, 4, 8, 8)
    for bad in ("1,2,3", "0,0,33,8", "8,0,4,8", "a,b,c,d", "0,0,0,8"):
        with pytest.raises(ValueError):
            demo.parse_box(bad, 32)
    mask = demo.box_mask((1, 3, 4, 32, 32), (0, 0, 16, 32), keep=True)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (1, 1, 4, 32, 32) and bool(mask[:, :, :, :16].all()) and not bool(mask[:, :, :, 16:].any())
    assert torch.equal(demo.box_mask((1, 3, 4, 32, 32), (0, 0, 16, 32), keep=False), ~mask)
