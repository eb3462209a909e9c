"""Sampling conditioned on known frames (replacement method) and long videos as chains of windows.  Six groups: the level
tables; one step of each op against the same call without the known operands; the conditioning acting on data with a closed-form predictor;
whole videos against a loop over the oracle's own pieces; the plumbing on the GPU; long videos.

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
    alphas_cumprod[time_next], the end of the last step on a = 1."""
    acp = O.make_schedule(total)["alphas_cumprod"].double().numpy()
    pairs = O.ddim_time_pairs(total, steps)
    a = [acp[pairs[0][0]]] + [1.0 if i == len(pairs) - 1 else acp[tn] for i, (_, tn) in enumerate(pairs)]
    return np.array([(math.sqrt(v), math.sqrt(1.0 - v)) for v in a])


# ------------------------------------------------------------------------------------------ 1. level tables (host only)
@pytest.mark.parametrize("steps", [1, 2, 3, 20, 100])
def test_level_tables(steps):
    total = 1000
    sched = O.make_schedule(total)
    pairs = O.ddim_time_pairs(total, steps)
    d = diffusion("reference", steps, total)
    before = d._step_tables(True)
    lv = d._level_table(True)
    assert lv.shape == (steps + 1, 2) and lv.dtype == torch.float32
    _, coef, _ = d._step_tables(True)
    assert torch.equal(lv[1:, 0], coef[:, 2])
    acp_prev = sched["alphas_cumprod_prev"]
    for i, (time, time_next) in enumerate(pairs):
        assert torch.equal(lv[i + 1, 0], acp_prev[time_next].sqrt())
        assert torch.equal(lv[i + 1, 1], (1 - acp_prev[time_next]).sqrt())
    assert torch.equal(lv[0, 0], acp_prev[pairs[0][0]].sqrt()) and torch.equal(lv[0, 1], (1 - acp_prev[pairs[0][0]]).sqrt())
    assert tuple(lv[-1].tolist()) == (1.0, 0.0)
    for a, b in zip(before, d._step_tables(True)):          # `_step_tables` returns what it returned
        assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b
    for sampler in ("dpmpp_1", "dpmpp_2m"):
        d = diffusion(sampler, steps, total)
        t0, c0 = d._ms_step_tables(sampler)
        lv = d._level_table(True, sampler)
        want = ms_levels(total, steps)
        assert lv.shape == (steps + 1, 2) and lv.dtype == torch.float32
        assert np.all(np.abs(lv.double().numpy() - want) <= 1e-6 * np.abs(want)), np.abs(lv.double().numpy() - want).max()
        assert tuple(lv[-1].tolist()) == (1.0, 0.0)
        t1, c1 = d._ms_step_tables(sampler)
        assert t0 == t1 and torch.equal(c0, c1)


def test_level_table_ddpm():
    total = 8
    sched = O.make_schedule(total)
    d = diffusion("reference", total, total)
    assert not d.is_ddim_sampling
    lv = d._level_table(False)
    assert lv.shape == (total + 1, 2)
    a0 = sched["alphas_cumprod"][total - 1]
    assert torch.equal(lv[0, 0], a0.sqrt()) and torch.equal(lv[0, 1], (1 - a0).sqrt())
    for i, t in enumerate(reversed(range(total))):
        a = sched["alphas_cumprod_prev"][t]
        assert torch.equal(lv[i + 1, 0], a.sqrt()) and torch.equal(lv[i + 1, 1], (1 - a).sqrt())
    assert tuple(lv[-1].tolist()) == (1.0, 0.0)
    # each step ends on the level the next one starts from: alphas_cumprod_prev[t] == alphas_cumprod[t - 1]
    assert torch.equal(sched["alphas_cumprod_prev"][1:], sched["alphas_cumprod"][:-1])


def test_level_tables_are_kept_per_sampler_and_schedule():
    d = diffusion("dpmpp_2m", 10, 50)
    levels = lambda sampler: (lambda s: (s.level_host, s.level))(d._schedule(True, sampler, torch.device("cpu"), level=True))
    h1, d1 = levels("dpmpp_2m")
    h2, d2 = levels("dpmpp_2m")
    assert h1 is h2 and d1 is d2 and torch.equal(h1, d1)
    h3, _ = levels("reference")
    assert h3 is not h1 and not torch.equal(h3, h1)
    h4, _ = levels("dpmpp_2m")
    assert torch.equal(h4, h1)
    d.alphas_cumprod.mul_(0.5)                                      # an in-place write bumps the buffer's version counter
    h5, _ = levels("dpmpp_2m")
    assert not torch.equal(h5, h1)


# ------------------------------------------------------------------------------------------ 2. one step of each op
def _masks(batch, frames):
    """Per-sample masks: sample 0 mixed, sample 1 all False, sample 2 all True."""
    m = torch.zeros(batch, frames, dtype=torch.bool)
    m[0, 0] = True
    m[0, frames - 2] = True
    if batch > 2:
        m[2] = True
    return m


def _known_pair(shape, mask, seed):
    """(known, known_noise): finite at the masked frames, NaN at every other frame."""
    k, z = rnd(*shape, seed=seed), rnd(*shape, seed=seed + 1)
    keep = mask[:, None, :, None].expand(shape)
    nan = torch.full(shape, float("nan"))
    return torch.where(keep, k, nan), torch.where(keep, z, nan)


def _check_blend(x, ref_plain, k, z, a, s, mask, what):
    keep = mask[:, None, :, None].expand(x.shape)
    assert torch.isfinite(x).all(), what
    assert torch.equal(x[~keep], ref_plain[~keep]), "%s: an unmasked frame differs from the plain call" % what
    if keep.any():
        want = a * k[keep].double() + s * z[keep].double()
        err = (x[keep].double() - want).abs()
        print("%s: masked frames max |x - (a k + s n)| %.3e" % (what, float(err.max())))
        assert bool((err <= 1e-6 * want.abs().clamp_min(1.0)).all()), (what, float(err.max()))
        if (a, s) == (1.0, 0.0):
            assert torch.equal(x[keep], k[keep]), "%s: (1, 0) row does not return the known frames bit for bit" % what


@pytest.mark.parametrize("cthw", [(3, 5, 71), (3, 7, 57143)])
@pytest.mark.parametrize("batch", [1, 2, 3])
@pytest.mark.parametrize("dynamic", [True, False])
@pytest.mark.parametrize("op", ["step", "step_ms"])
def test_known_step(backend, op, dynamic, batch, cthw):
    """Two steps in a row on one workspace (the second meets the histograms and the ticket the first one left), each against the same call
    without the known operands on the same inputs.  c_x, c_eps are powers of two as in test_step_ms.  3 x 7 x 57143 = 1 200 003 elements
    > 8 x 512 x 256: the loop behind the prefetched elements runs."""
    from cvpr23_lfdm_amd import ops
    dev = backend
    c, t, hw = cthw
    n = c * t * hw
    if n > 1 << 20 and not big(dev):
        pytest.skip("above 8 x 512 x 256 elements per sample: GPU only")
    q = 0.9 if dynamic else -1.0
    ms = op == "step_ms"
    if ms:
        table = torch.tensor([[9.] * 6, [2.0, 0.5, 0.8125, 0.37, 0.0, 0.0], [0.5, 0.25, 0.9, 0.61, -0.23, 0.0]])
    else:
        table = torch.tensor([[9.] * 6, [2.0, 0.5, 0.9, 0.3, 0.0, 0.4], [0.5, 0.25, 0.7, 0.0, 0.2, 0.0]])
    level = torch.tensor([[9., 9.], [9., 9.], [0.8125, 0.59], [1.0, 0.0]])
    shape = (batch, c, t, hw)
    x, e1, e2, z1 = rnd(*shape, seed=1), rnd(*shape, seed=2), rnd(*shape, seed=3), rnd(*shape, seed=4)
    if batch > 1:
        x[1] *= 0.1
        e1[1] *= 0.1
    mask = _masks(batch, t)
    k, z = _known_pair(shape, mask, 20)
    kf = dict(known=k.to(dev), known_noise=z.to(dev), frame_mask=mask.to(dev), level=level.to(dev), frames=t)

    def call(xd, eps, second, step, ws, x0_out, known):
        kw = dict(quantile=q, x0_out=x0_out, ws=ws, **(kf if known else {}))
        if ms:
            ops.sampler_step_ms(xd, eps.to(dev), second, table.to(dev), step, **kw)
        else:
            ops.sampler_step(xd, eps.to(dev), second, table.to(dev), step, **kw)

    def run():
        out = {}
        state = {}
        for known in (True, False):
            xd = x.clone().to(dev)
            second = torch.full(shape, float("nan")).to(dev) if ms else z1.to(dev)
            step = torch.tensor([1], dtype=torch.int32).to(dev)
            ws = ops.sampler_ws(batch, n, dev)
            o = torch.empty(shape).to(dev)
            call(xd, e1, second, step, ws, o, known)
            out[known, 1] = (xd.cpu().clone(), o.cpu().clone(), second.cpu().clone(), int(step.cpu()[0]))
            state[known] = (xd, second, step, ws)
        # second step: both calls start from the state the conditioned first step left
        xd_k, sec_k, step_k, ws_k = state[True]
        xd_p, sec_p, step_p, ws_p = state[False]
        xd_p.copy_(xd_k)
        if ms:
            sec_p.copy_(sec_k)
        for known, (xd, sec, step, ws) in ((True, (xd_k, sec_k, step_k, ws_k)), (False, (xd_p, sec_p, step_p, ws_p))):
            o = torch.empty(shape).to(dev)
            call(xd, e2, sec, step, ws, o, known)
            out[known, 2] = (xd.cpu().clone(), o.cpu().clone(), sec.cpu().clone(), int(step.cpu()[0]))
        return out

    got = run()
    for i, (a, s) in ((1, (0.8125, 0.59)), (2, (1.0, 0.0))):
        xk, ok, hk, sk = got[True, i]
        xp, op_, hp, sp = got[False, i]
        what = "%s %s B=%d n=%d step %d" % (op, "dynamic" if dynamic else "static", batch, n, i)
        assert sk == sp == i + 1, what
        assert torch.equal(ok, op_) and torch.isfinite(ok).all(), "%s: x0_out differs" % what
        if ms:
            assert torch.equal(hk, hp) and torch.isfinite(hk).all(), "%s: hist differs" % what
        _check_blend(xk, xp, k, z, a, s, mask, what)
    keep = mask[:, None, :, None].expand(shape)
    assert not torch.equal(got[True, 1][0][keep], got[False, 1][0][keep]), "the conditioning did nothing"
    again = run()
    for key in got:
        for a, b in zip(got[key][:3], again[key][:3]):
            assert torch.equal(a, b), key


@pytest.mark.parametrize("cthw", [(3, 5, 71), (3, 7, 57143)])
@pytest.mark.parametrize("batch", [1, 2, 3])
def test_known_blend(backend, batch, cthw):
    from cvpr23_lfdm_amd import ops
    dev = backend
    c, t, hw = cthw
    if c * t * hw > 1 << 20 and not big(dev):
        pytest.skip("above 8 x 512 x 256 elements per sample: GPU only")
    shape = (batch, c, t, hw)
    x = rnd(*shape, seed=1)
    mask = _masks(batch, t)
    k, z = _known_pair(shape, mask, 30)
    for a, s in ((0.3125, 0.95), (1.0, 0.0)):
        outs = []
        for _ in range(2):
            xd = x.clone().to(dev)
            ops.known_blend(xd, k.to(dev), z.to(dev), mask.to(dev), a, s, t)
            outs.append(xd.cpu())
        assert torch.equal(outs[0], outs[1])
        _check_blend(outs[0], x, k, z, a, s, mask, "known_blend B=%d n=%d (%g, %g)" % (batch, c * t * hw, a, s))


def test_known_ops_refuse_bad_arguments(backend):
    from cvpr23_lfdm_amd import ops
    dev = backend
    shape = (1, 3, 4, 25)
    x, eps = torch.zeros(shape).to(dev), torch.zeros(shape).to(dev)
    table, step = torch.zeros(1, 6).to(dev), torch.zeros(1, dtype=torch.int32).to(dev)
    level = torch.tensor([[1., 0.], [1., 0.]]).to(dev)
    mask = torch.zeros(1, 4, dtype=torch.bool).to(dev)
    good = dict(known=x.clone(), known_noise=x.clone(), frame_mask=mask, level=level, frames=4)
    for drop in good:                                     # all of them or none
        kw = {k: v for k, v in good.items() if k != drop}
        with pytest.raises(ValueError, match="all of them or none"):
            ops.sampler_step(x, eps, None, table, step, quantile=-1.0, **kw)
        with pytest.raises(ValueError, match="all of them or none"):
            ops.sampler_step_ms(x, eps, x.clone(), table, step, quantile=-1.0, **kw)
    for bad in (dict(frames=5), dict(frame_mask=torch.zeros(1, 3, dtype=torch.bool).to(dev)), dict(known=torch.zeros(1, 3, 4, 24).to(dev)),
                dict(frame_mask=torch.zeros(1, 4).to(dev)), dict(level=torch.zeros(2, 3).to(dev)),
                dict(known_noise=torch.zeros(shape, dtype=torch.float64).to(dev))):
        with pytest.raises(ValueError):
            ops.sampler_step(x, eps, None, table, step, quantile=-1.0, **dict(good, **bad))
        with pytest.raises(ValueError):
            ops.sampler_step_ms(x, eps, x.clone(), table, step, quantile=-1.0, **dict(good, **bad))
    with pytest.raises(ValueError):
        ops.known_blend(x, x.clone(), x.clone(), mask, 1.0, 0.0, 3)
    with pytest.raises(ValueError):
        ops.known_blend(x, x.clone(), None, mask, 1.0, 0.0, 4)
    # the C entry points check for themselves: a frame split that does not divide n, null operands
    from cvpr23_lfdm_amd import _native
    lib = _native.library()
    ws = ops.sampler_ws(1, 300, dev)
    args = dict(x=ops._p(x), eps=ops._p(eps), batch=1, n=300, coef=ops._p(table), step_dev=ops._p(step), quantile=-1.0, advance=1, ws=ops._p(ws),
                ws_bytes=ws.numel() * 4)
    known = dict(known=ops._p(good["known"]), known_noise=ops._p(good["known_noise"]), frame_mask=ops._p(mask), level=ops._p(level))

    def c_step(a, k):
        return lib.lfdm_sampler_step_f32(ctypes.byref(_native.SamplerStepParams(known=_native.KnownOperands(**k), **a)), ops._stream(lib))

    def c_blend(k):
        return lib.lfdm_known_blend_f32(ops._p(x), ctypes.byref(_native.KnownOperands(**k)), 1.0, 0.0, 1, 300, ops._stream(lib))

    assert c_step(args, dict(known, frames=4, frame_elems=26)) != 0 and b"frames" in lib.lfdm_last_error()
    assert c_step(args, dict(known, known_noise=None, frames=4, frame_elems=25)) != 0
    hist = x.clone()
    assert c_step(dict(args, hist=ops._p(hist), multistep=1), dict(known, frames=7, frame_elems=25)) != 0 and b"frames" in lib.lfdm_last_error()
    assert c_blend(dict(known, level=None, frame_mask=None, frames=4, frame_elems=25)) != 0
    assert c_blend(dict(known, level=None, frames=4, frame_elems=0)) != 0
    assert int(step.cpu()[0]) == 0 and not x.cpu().any()                # nothing ran


# ------------------------------------------------------------------------------------------ 3. the conditioning acts
MU, SD = 0.3, 0.2


def _shared_eps(x, al, sg):
    """Optimal eps predictor when all F frames of a pixel share ONE value z ~ N(MU, SD^2): x (F, P) -> eps (F, P)."""
    f = x.shape[0]
    z_hat = (MU / SD ** 2 + al * x.sum(axis=0, keepdims=True) / sg ** 2) / (1.0 / SD ** 2 + f * al ** 2 / sg ** 2)
    return (x - al * z_hat) / sg


def _drive_shared(dev, steps, conditioned, frames=8, n_known=4, pixels=4096):
    """-> (the op's final x (F, P), the test's double recurrence, k (P,))."""
    from cvpr23_lfdm_amd import ops
    d = diffusion("dpmpp_1", steps)
    _, coef = d._ms_step_tables("dpmpp_1")
    lv = ms_levels(1000, steps)
    # (the seed: a draw whose 4096 values of N(0.3, 0.2^2) stay below 1 - a value beyond 3.5 sd turns up in about every second draw, and with
    #  it the clamp the closed form excludes; the assertion below guards that precondition)
    rng = np.random.Generator(np.random.PCG64(42))
    k = MU + SD * rng.standard_normal(pixels)
    x_t, kn = rng.standard_normal((frames, pixels)), rng.standard_normal((frames, pixels))
    known = np.full((frames, pixels), np.nan)
    known[:n_known] = k
    kn[n_known:] = np.nan
    mask = np.zeros(frames, dtype=bool)
    mask[:n_known] = conditioned
    shape = (1, 1, frames, pixels)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).reshape(shape).contiguous()
    known32, kn32 = f32(known), f32(kn)
    k64, kn64 = known32.double().numpy().reshape(frames, pixels), kn32.double().numpy().reshape(frames, pixels)
    x64 = f32(x_t).double().numpy().reshape(frames, pixels)
    xd = f32(x_t).to(dev)
    mask_t = torch.from_numpy(mask).view(1, frames)
    level = torch.tensor(lv, dtype=torch.float64).float().contiguous()
    kf = {}
    if conditioned:
        kf = dict(known=known32.to(dev), known_noise=kn32.to(dev), frame_mask=mask_t.to(dev), level=level.to(dev), frames=frames)
        ops.known_blend(xd, kf["known"], kf["known_noise"], kf["frame_mask"], float(level[0, 0]), float(level[0, 1]), frames)
        x64[mask] = lv[0, 0] * k64[mask] + lv[0, 1] * kn64[mask]
    hist = torch.full(shape, float("nan")).to(dev)
    step = torch.zeros(1, dtype=torch.int32).to(dev)
    ws, coef_dev = ops.sampler_ws(1, frames * pixels, dev), coef.to(dev)
    peak = 0.0
    for i in range(steps):
        al_s, sg_s = lv[i]
        al_n, sg_n = lv[i + 1]
        eps = _shared_eps(xd.cpu().double().numpy().reshape(frames, pixels), al_s, sg_s)
        ops.sampler_step_ms(xd, f32(eps).to(dev), hist, coef_dev, step, quantile=-1.0, ws=ws, **kf)
        e64 = _shared_eps(x64, al_s, sg_s)
        x0 = (x64 - sg_s * e64) / al_s
        peak = max(peak, float(np.abs(x0).max()))
        x64 = (sg_n / sg_s) * x64 + (al_n - sg_n * al_s / sg_s) * np.clip(x0, -1.0, 1.0)
        if conditioned:
            x64[mask] = al_n * k64[mask] + sg_n * kn64[mask]
    assert int(step.cpu()[0]) == steps
    assert peak < 1.0, "the clamp must stay inactive (max |x0| %.3f)" % peak
    return xd.cpu().double().numpy().reshape(frames, pixels), x64, k


@pytest.mark.parametrize("steps", [20, 50])
def test_conditioning_pulls_unknown_frames_to_the_known_ones(backend, steps):
    """F = 8 frames of a pixel share one value; frames 0-3 are known to be k.  The unknown frames must end near k: mean |x - k| at most half
    of what the same run gives without conditioning.  A double numpy model of exactly this set-up gives 0.078 vs 0.218 (ratio 0.36) at 20
    steps and 0.055 vs 0.222 (0.25) at 50 steps for this draw (0.48 at 10 steps: too close to the bar to test)."""
    dev = backend
    res = {}
    for conditioned in (True, False):
        got, model, k = _drive_shared(dev, steps, conditioned)
        assert np.abs(got - model).max() <= 1e-5, (conditioned, np.abs(got - model).max())
        if conditioned:
            assert np.array_equal(got[:4], np.broadcast_to(k.astype(np.float32).astype(np.float64), got[:4].shape))
        res[conditioned] = float(np.abs(got[4:] - k).mean())
        corr = float(np.corrcoef(got[5], k)[0, 1])
        print("%d steps, %s: unknown frames mean |x - k| %.4f, correlation of frame 5 with k %.3f"
              % (steps, "conditioned" if conditioned else "unconditioned", res[conditioned], corr))
    print("%d steps: ratio %.3f" % (steps, res[True] / res[False]))
    assert res[True] <= 0.5 * res[False], res


# ------------------------------------------------------------------------------------------ 4. whole videos against the oracle's pieces
def _skip_slow_emu(dev):
    if dev == "cpu" and os.environ.get("LFDM_EMU_E2E", "0") != "1":
        pytest.skip("end-to-end under the emulator is opt-in (LFDM_EMU_E2E=1); it runs on the GPU")


def _where_frames(mask, a, b):
    return torch.where(mask[:, None, :, None, None], a, b)


def oracle_known_latent(kind, sd, fea, cond, shape, steps, total, cond_scale, noise_fn, known, mask, draw_known=True, eta=1.0):
    """The sampling loop over the oracle's own pieces + the blend of the contract.  kind: "ddim" | "ddpm" | "dpmpp_2m"."""
    b, _, frames, _, _ = shape
    x = noise_fn(tuple(shape))
    kn = noise_fn(tuple(shape)) if draw_known else torch.zeros(shape)
    fea_rep = fea.unsqueeze(2).repeat(1, 1, frames, 1, 1)

    def blend(x, a, s):
        return _where_frames(mask, a * known + s * kn, x)

    if kind == "ddim":
        pairs = O.ddim_time_pairs(total, steps)
        a0 = sd["alphas_cumprod_prev"][pairs[0][0]]
        x = blend(x, a0.sqrt(), (1 - a0).sqrt())
        for time, time_next in pairs:
            z = noise_fn(tuple(shape)) if time_next > 0 else None
            x, _, _ = O.ddim_step(sd, x, fea_rep, cond, time, time_next, z, eta, cond_scale, True)
            a = sd["alphas_cumprod_prev"][time_next]
            x = blend(x, a.sqrt(), (1 - a).sqrt())
    elif kind == "ddpm":
        a0 = sd["alphas_cumprod"][total - 1]
        x = blend(x, a0.sqrt(), (1 - a0).sqrt())
        for time in reversed(range(total)):
            x, _, _ = O.ddpm_step(sd, x, fea_rep, cond, time, noise_fn(tuple(shape)), cond_scale, True)
            a = sd["alphas_cumprod_prev"][time]
            x = blend(x, a.sqrt(), (1 - a).sqrt())
    else:
        lv = ms_levels(total, steps)
        pairs = O.ddim_time_pairs(total, steps)
        x = blend(x.double(), lv[0, 0], lv[0, 1]).float()
        m_prev, h_prev = None, None
        for i, (time, _) in enumerate(pairs):
            last = i == len(pairs) - 1
            (al_s, sg_s), (al_n, sg_n) = lv[i], lv[i + 1]
            t = torch.full((b,), time, dtype=torch.long)
            eps = O.unet_forward_with_cond_scale(sd, torch.cat([x, fea_rep], dim=1), t, cond, cond_scale)
            m = O.dynamic_threshold(O.predict_start_from_noise(sd, x, t, eps)).double()
            k = al_n - sg_n * al_s / sg_s
            h = math.inf if last else math.log(al_n / sg_n) - math.log(al_s / sg_s)
            if i == 0 or last:
                new = (sg_n / sg_s) * x.double() + k * m
            else:
                r = h_prev / h
                new = (sg_n / sg_s) * x.double() + k * (1 + 1 / (2 * r)) * m - k / (2 * r) * m_prev
            x, m_prev, h_prev = blend(new, al_n, sg_n).float(), m, h
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


def _sizes(dev):
    return dict(b=1, t=4, s=8, hw=32) if dev == "cpu" else dict(b=2, t=8, s=16, hw=64)


def test_the_loop_is_the_oracles_own():
    """All-False mask, no extra draw: the test's DDIM loop equals O.sample bit for bit (host only, tiny UNet input)."""
    b, t, s, steps, total = 1, 2, 8, 3, 1000
    dsd = {"denoise_fn." + k: v for k, v in synth.unet_state().items()}
    sd = dict(dsd)
    sd.update(O.make_schedule(total))
    img, cond = synth.inputs(b, 32)
    fea = O.generator_compute_fea(synth.generator_state(), img)
    shape = (b, 3, t, s, s)
    mask = torch.zeros(b, t, dtype=torch.bool)
    known = torch.full(shape, float("nan"))
    got = oracle_known_latent("ddim", sd, fea, cond, shape, steps, total, 1.0, synth.NoiseTape(11), known, mask, draw_known=False)
    want = O.sample(sd, fea, cond, shape, steps, total, 1.0, 1.0, synth.NoiseTape(11))
    assert torch.equal(got, want)


@pytest.mark.parametrize("cond_scale", [1.0, 2.0])
@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m", "ddpm"])
def test_sample_one_video_known_frames(backend, kind, cond_scale):
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
    known = synth.NoiseTape(23)(shape).clamp(-1, 1).contiguous()
    mask = torch.zeros(z["b"], z["t"], dtype=torch.bool)
    mask[:, :3] = True
    fea = O.generator_compute_fea(gsd, img)
    if kind == "ddim" and cond_scale == 1.0:       # pins the loop to the oracle that is pinned to the reference, at this size too
        none = torch.zeros_like(mask)
        assert torch.equal(oracle_known_latent("ddim", sd, fea, cond, shape, steps, total, 1.0, synth.NoiseTape(11), known, none, draw_known=False),
                           O.sample(sd, fea, cond, shape, steps, total, 1.0, 1.0, synth.NoiseTape(11)))
    lat = oracle_known_latent(kind, sd, fea, cond, shape, steps, total, cond_scale, synth.NoiseTape(11), known, mask)
    ref = _decode(gsd, img, lat, z["t"])
    m.diffusion.noise_source = synth.NoiseTape(11)
    m.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))
    m.sample_one_video(cond_scale=cond_scale, known_latent=known.to(dev), known_mask=mask.to(dev))
    for k in ("sample_vid_grid", "sample_vid_conf", "sample_warped_vid", "sample_out_vid"):
        assert_close(getattr(m, k).cpu(), ref[k], 1e-3, "%s (%s, known frames, cond_scale %g)" % (k, kind, cond_scale))
    assert torch.equal(m.sample_latent.cpu()[:, :, :3], known[:, :, :3])
    assert float((m.sample_latent.cpu()[:, :, 3:] - known[:, :, 3:]).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------ 5. plumbing on the GPU
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvpr23_lfdm_amd import _native
    _native._set_library_for_tests(None)


KW = dict(img_size=8, num_frames=4, sampling_timesteps=7)


def _known(seed, frames_known, nf=4, s=8, nan=True):
    shape = (1, 3, nf, s, s)
    k = synth.NoiseTape(100 + seed)(shape).clamp(-1, 1)
    mask = torch.zeros(1, nf, dtype=torch.bool)
    mask[:, list(frames_known)] = True
    if nan:
        k = torch.where(mask[:, None, :, None, None], k, torch.full(shape, float("nan")))
    return k.contiguous(), mask


def _video(m, seed, known=None, mask=None, tape=True):
    img, cond = synth.inputs(1, 32, seed=seed)
    m.diffusion.noise_source = synth.NoiseTape(seed) if tape else None
    m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
    if known is None:
        m.sample_one_video(cond_scale=1.0)
    else:
        m.sample_one_video(cond_scale=1.0, known_latent=known.cuda(), known_mask=mask.cuda())
    assert torch.equal(m.sample_vid_grid, m.sample_latent[:, :2])
    return m.sample_latent.clone()


def _model(sampler, **kw):
    total = kw.pop("timesteps", 1000)
    return synth.build_flow_diffusion("cuda", sampler=sampler, timesteps=total, **dict(KW, **kw))[0]


SAMPLERS = [("reference", {}), ("dpmpp_2m", {}), ("reference", dict(timesteps=7))]       # DDIM, 2M, DDPM on 7 timesteps


@pytest.mark.gpu
@pytest.mark.parametrize("sampler,extra", SAMPLERS)
def test_unconditioned_videos_are_untouched_by_a_conditioned_one(sampler, extra):
    _gpu()
    m = _model(sampler, **extra)
    k, mask = _known(5, (0, 1))
    first = _video(m, 5)
    cond = _video(m, 5, k, mask)
    third = _video(m, 5)
    assert torch.equal(first, third)
    assert torch.equal(first, _video(_model(sampler, **extra), 5))
    assert not torch.equal(first, cond) and torch.isfinite(cond).all()
    assert torch.equal(cond[:, :, :2].cpu(), torch.nan_to_num(k)[:, :, :2])


@pytest.mark.gpu
@pytest.mark.parametrize("sampler,extra", SAMPLERS)
def test_other_mask_and_frames_need_no_new_plan(sampler, extra):
    _gpu()
    m = _model(sampler, **extra)
    cases = [(5, (0, 1)), (6, (0, 3)), (5, (2,))]
    got = [_video(m, seed, *_known(seed, fr)) for seed, fr in cases]
    plans = [p for key, p in m.diffusion._plans.items() if key.known]
    assert len(plans) == 1
    for (seed, fr), g in zip(cases, got):
        k, mask = _known(seed, fr)
        assert torch.equal(g, _video(_model(sampler, **extra), seed, k, mask)), (seed, fr)
        assert torch.equal(g[:, :, list(fr)].cpu(), k[:, :, list(fr)])
    assert not torch.equal(got[0], got[2])


@pytest.mark.gpu
def test_graph_chunks_do_not_change_a_conditioned_video(monkeypatch):
    _gpu()
    k, mask = _known(5, (0, 1))
    outs = {}
    for steps in ("1", "3", "10"):
        monkeypatch.setenv("LFDM_GRAPH_STEPS", steps)
        m = _model("dpmpp_2m")
        a = [_video(m, 5, k, mask), _video(m, 6, k, mask)]
        m = _model("reference")                                 # DDIM eta 1 with torch's generator under a fixed seed
        b = []
        for _ in range(2):
            torch.manual_seed(77)
            b.append(_video(m, 5, k, mask, tape=False))
        assert torch.equal(b[0], b[1])
        outs[steps] = a + b
    for steps in ("3", "10"):
        for x, y in zip(outs["1"], outs[steps]):
            assert torch.equal(x, y), "LFDM_GRAPH_STEPS=%s" % steps


@pytest.mark.gpu
def test_all_false_mask_is_the_unconditioned_video():
    """dpmpp_2m draws nothing after x_T: the extra tape entry is the only difference and is never used."""
    _gpu()
    m = _model("dpmpp_2m")
    k, mask = _known(5, ())
    assert not mask.any() and torch.isnan(k).all()
    assert torch.equal(_video(m, 5, k, mask), _video(_model("dpmpp_2m"), 5))


@pytest.mark.gpu
def test_threshold_mode_is_part_of_the_plan():
    """use_dynamic_thres goes into the update kernel's arguments at capture time: changing it between two videos of one model must not
    replay a graph captured under the other mode.  T = 4, S = 8, 5 DDIM steps on tape 5, where the CPU oracle's 0.9 quantile of |x0| is
    6.92, 2.82, 1.79, 1.28, 1.01 over the steps (above 1 on every one: the two modes clamp differently, max difference 0.91 in the latent)."""
    _gpu()
    kw = dict(sampling_timesteps=5)
    m = _model("reference", **kw)
    assert m.diffusion.use_dynamic_thres and m.diffusion.dynamic_thres_percentile == 0.9
    first = _video(m, 5)
    m.diffusion.use_dynamic_thres = False
    second = _video(m, 5)
    plans = m.diffusion._plans
    assert 1 <= len(plans) <= 2 and {key.quantile for key in plans} in ({-1.0}, {-1.0, 0.9})      # two plans or one replaced, never a stale graph
    m.diffusion.use_dynamic_thres = True
    third = _video(m, 5)
    static = _model("reference", **kw)
    static.diffusion.use_dynamic_thres = False
    assert torch.equal(second, _video(static, 5))
    assert torch.equal(first, third)
    assert not torch.equal(second, first) and torch.isfinite(second).all()


@pytest.mark.gpu
def test_known_frames_compose_with_bf16_convolutions():
    _gpu()
    k, mask = _known(5, (0, 1))
    a = _video(_model("dpmpp_2m", conv_precision="bf16"), 5, k, mask)
    b = _video(_model("dpmpp_2m"), 5, k, mask)
    assert torch.isfinite(a).all() and not torch.equal(a, b)
    assert torch.equal(a[:, :, :2].cpu(), k[:, :, :2])


@pytest.mark.gpu
def test_functional_wrapper_takes_known_frames():
    _gpu()
    from cvpr23_lfdm_amd.flow_diffusion import FlowDiffusionFunctional
    m = FlowDiffusionFunctional(img_size=8, num_frames=4, sampling_timesteps=7, is_train=False, config_pth=synth.CONFIG)
    m.unet.load_state_dict(synth.unet_state())
    m.generator.load_state_dict(synth.generator_state())
    m.eval().cuda()
    k, mask = _known(5, (0, 1))
    img, cond = synth.inputs(1, 32, seed=5)
    m.diffusion.noise_source = synth.NoiseTape(5)
    out = m.sample_one_video(img.cuda(), cond.cuda(), 1.0, known_latent=k.cuda(), known_mask=mask.cuda())
    ref = _model("reference")
    assert torch.equal(out["sample_latent"], _video(ref, 5, k, mask))
    for name in ("sample_vid_grid", "sample_vid_conf", "sample_out_vid", "sample_warped_vid"):
        assert torch.equal(out[name], getattr(ref, name))


# ------------------------------------------------------------------------------------------ 6. long videos
LKW = dict(img_size=8, num_frames=8, sampling_timesteps=7)


def _long_model(**kw):
    return synth.build_flow_diffusion("cuda", **dict(LKW, **kw))[0]


def _set(m, seed=5):
    img, cond = synth.inputs(1, 32, seed=seed)
    m.diffusion.noise_source = synth.NoiseTape(seed)
    m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
    return img.cuda(), cond.cuda()


NAMES = ("sample_vid_grid", "sample_vid_conf", "sample_out_vid", "sample_warped_vid")


@pytest.mark.gpu
@pytest.mark.parametrize("total,residual", [(8, False), (13, False), (20, False), (5, False), (13, True)])
def test_long_video(total, residual):
    _gpu()
    nf, overlap = 8, 3
    kw = dict(use_residual_flow=True) if residual else {}
    m = _long_model(**kw)
    img, cond = _set(m)
    calls = []
    encode = m.generator.encode
    m.generator.encode = lambda *a, **k: (calls.append(1), encode(*a, **k))[1]
    m.sample_long_video(1.0, total, overlap=overlap)
    assert len(calls) == 1, "the LFAE encoder ran %d times" % len(calls)
    m.generator.encode = encode
    got = {k: getattr(m, k).clone() for k in NAMES + ("sample_latent",)}
    for k, ch, hw in (("sample_vid_grid", 2, 8), ("sample_vid_conf", 1, 8), ("sample_out_vid", 3, 32), ("sample_warped_vid", 3, 32),
                      ("sample_latent", 3, 8)):
        assert tuple(got[k].shape) == (1, ch, total, hw, hw) and torch.isfinite(got[k]).all(), k
    # frames 0 .. 7: the plain video on the same tape
    plain = _long_model(**kw)
    _set(plain)
    plain.sample_one_video(1.0)
    head = min(total, nf)
    for k in NAMES + ("sample_latent",):
        assert torch.equal(got[k][:, :, :head], getattr(plain, k)[:, :, :head]), k
    # the whole latent: a hand-written chain of conditioned samples on the same tape
    fresh = _long_model(**kw)
    _set(fresh)
    gen = fresh.generator
    skips = gen.encode(img.float().contiguous())
    fea = gen.compute_fea_from_skips(skips, 1, 8, 8)
    chunk = fresh.diffusion.sample(fea, cond=cond, cond_scale=1.0)
    pieces, have = [chunk], nf
    mask = torch.zeros(1, nf, dtype=torch.bool, device="cuda")
    mask[:, :overlap] = True
    while have < total:
        known = torch.full_like(chunk, float("nan"))
        known[:, :, :overlap] = chunk[:, :, nf - overlap:]
        chunk = fresh.diffusion.sample(fea, cond=cond, cond_scale=1.0, known=known, known_mask=mask)
        assert torch.equal(chunk[:, :, :overlap], known[:, :, :overlap])
        pieces.append(chunk[:, :, overlap:])
        have += nf - overlap
    latent = torch.cat(pieces, dim=2)[:, :, :total].contiguous()
    assert torch.equal(got["sample_latent"], latent)
    if total > nf:
        assert len(pieces) == {13: 2, 20: 4}[total]             # 8 + 5 = 13;  8 + 5 + 5 + 5 = 23 >= 20
    # the decoded videos: generator.decode_video on that latent's pieces
    for f0 in range(0, total, nf):
        part = latent[:, :, f0:f0 + nf].contiguous()
        n_part = part.shape[2]
        maps = part
        if residual:
            maps = torch.cat((part[:, :2] + O.identity_grid(1, n_part, 8, 8).cuda(), part[:, 2:3]), dim=1).contiguous()
        out, warped = gen.decode_video(img.float().contiguous(), skips, maps[:, 0], maps[:, 1], maps[:, 2], n_part, 8, 8,
                                       3 * n_part * 64, 64, occ_scale=0.5, occ_bias=0.5)
        sl = slice(f0, f0 + n_part)
        assert torch.equal(got["sample_out_vid"][:, :, sl], out) and torch.equal(got["sample_warped_vid"][:, :, sl], warped)
        assert torch.equal(got["sample_vid_grid"][:, :, sl], maps[:, :2])
        assert torch.equal(got["sample_vid_conf"][:, :, sl], (part[:, 2:3] + 1) * 0.5)


# ------------------------------------------------------------------------------------------ argument validation (host only)
def test_sample_refuses_bad_known_arguments():
    d = diffusion("reference", 10)
    fea = torch.zeros(1, 256, 8, 8)
    cond = torch.zeros(1, 768)
    good = torch.zeros(1, 3, 4, 8, 8)
    mask = torch.zeros(1, 4, dtype=torch.bool)
    d.denoise_fn = torch.nn.Linear(1, 1)           # (a parameter to read the device from; nothing is launched)
    for kw in (dict(known=good), dict(known_mask=mask), dict(known=good[:, :, :3], known_mask=mask), dict(known=good, known_mask=mask[:, :3]),
               dict(known=good.double(), known_mask=mask), dict(known=good, known_mask=mask.float()), dict(known=good[:, :2], known_mask=mask),
               dict(known=[0.0], known_mask=mask)):
        with pytest.raises(ValueError, match="known"):
            d.sample(fea, cond=cond, **kw)
        with pytest.raises(ValueError, match="known"):
            d.ddim_sample(fea, (1, 3, 4, 8, 8), cond=cond, **kw)
        with pytest.raises(ValueError, match="known"):
            d.p_sample_loop(fea, (1, 3, 4, 8, 8), cond=cond, **kw)


def test_wrappers_refuse_bad_arguments():
    from cvpr23_lfdm_amd import FlowDiffusion
    m = FlowDiffusion(img_size=8, num_frames=8, sampling_timesteps=7, is_train=False, config_pth=synth.CONFIG)
    assert m.sample_latent is None
    m.set_sample_input(sample_img=torch.zeros(1, 3, 32, 32), sample_text=torch.zeros(1, 768))
    with pytest.raises(ValueError, match="overlap"):
        m.sample_long_video(1.0, 20, overlap=0)
    with pytest.raises(ValueError, match="overlap"):
        m.sample_long_video(1.0, 20, overlap=8)
    with pytest.raises(ValueError, match="total_frames"):
        m.sample_long_video(1.0, 0, overlap=3)
    with pytest.raises(ValueError, match="go together"):
        m.sample_one_video(1.0, known_latent=torch.zeros(1, 3, 8, 8, 8))
    with pytest.raises(ValueError, match="go together"):
        m.sample_one_video(1.0, known_mask=torch.zeros(1, 8, dtype=torch.bool))


def test_demo_flags_parse():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "demo.py")
    spec = importlib.util.spec_from_file_location("lfdm_demo_tool", path)
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    args = demo.build_parser().parse_args([])
    assert args.total_frames == 0 and args.overlap == 8
    args = demo.build_parser().parse_args(["--total-frames", "112", "--overlap", "4"])
    assert args.total_frames == 112 and args.overlap == 4
