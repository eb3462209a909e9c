"""Progressive distillation: `GaussianDiffusion.forward` while a round is set - around stub denoisers (the diffusion edge
alone, both backends) and once through the native UNet; `FlowDiffusion.begin_distill_round`.

Bars.  Loss: 1e-5 relative against the float64 restatement of the whole step on the same draws (test_train_known.py's loss bar: the loss
kernel's own sums are double above 16 terms; the targets reach it with a few fp32 roundings each).  Convexity and the closed loop: stated at
the tests.  Through the UNet: test_unet_train's bars, 1e-3 on the loss and 2e-3 of the largest gradient."""
import copy
import os

import pytest
import torch

from cvpr23_lfdm_amd import GaussianDiffusion, ops
from test_train_known import TIMESTEPS, _StubDenoiser, _stub_diffusion, _stub_inputs
from util import rnd

E = 2.0 ** -24
N = 4               # student steps


class _Teacher(_StubDenoiser):
    """A stub whose output depends on the timestep (the two teacher evaluations differ), in the working precision of its input."""

    def forward(self, x, t, cond=None, null_cond_prob=0., none_cond_mask=None):
        shift = torch.cos(t.to(x.dtype) * 0.01).reshape(-1, 1, 1, 1, 1)
        return x[:, :3] * self.w.to(x.dtype) + 0.1 * shift


def _teacher(dev, w=0.3):
    t = _Teacher()
    t.w.fill_(w)
    return t.to(dev)


def _distilling(dev, objective, loss_type="l2", schedule="cosine_zsnr", **kw):
    set_kw = {k: kw.pop(k) for k in ("distill_weight",) if k in kw}
    d = _stub_diffusion(dev, loss_type, objective=objective, step_grid="trailing", schedule=schedule, **kw)
    d.set_distill(_teacher(dev), N, **set_kw)
    return d


def _record(monkeypatch):
    """The calls of ops.distill_step of one step: [(args, kwargs, result)]."""
    seen, real = [], ops.distill_step

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append((a, k, out))
        return out

    monkeypatch.setattr(ops, "distill_step", spy)
    return seen, real


def _restate(d, x0, fea, k, noise, dyn):
    """The whole step in float64 on the fp32-rounded tables: -> (loss, t)."""
    tabs = d.distill_tables(N, d._distill["weight"])
    b = x0.shape[0]
    shp = (b, 1, 1, 1, 1)
    col = lambda tab, rows, j: tab[rows][:, j].double().reshape(shp)
    k = k.cpu()
    t = tabs["student_times"][k]
    a, s = d.sqrt_alphas_cumprod.cpu().double()[t].reshape(shp), d.sqrt_one_minus_alphas_cumprod.cpu().double()[t].reshape(shp)
    z = a * x0.cpu().double() + s * noise.cpu().double()
    fea5 = fea.cpu().double().unsqueeze(2).expand(-1, -1, x0.shape[2], -1, -1)
    teacher, student = copy.deepcopy(d._distill["teacher"]).cpu().double(), copy.deepcopy(d.denoise_fn).cpu().double()
    cur = z
    for half in (0, 1):
        rows = 2 * k + half
        out = teacher(torch.cat([cur, fea5], dim=1), tabs["teacher_times"][rows])
        c = [col(tabs["teacher_coef"], rows, j) for j in range(6)]
        x0p = c[0] * cur - c[1] * out
        thr = torch.ones(b, dtype=torch.float64)
        if dyn:
            thr = torch.quantile(x0p.reshape(b, -1).abs(), d.dynamic_thres_percentile, dim=1).clamp(min=1.0)
        thr = thr.reshape(shp)
        cur = c[2] * torch.minimum(torch.maximum(x0p, -thr), thr) / thr + c[4] * cur
    q = [col(tabs["target_coef"], k, j) for j in range(4)]
    xt = q[0] * cur + q[1] * z
    et = q[2] * z + q[3] * xt
    target = xt if d.objective == "pred_x0" else a * et - s * xt
    out = student(torch.cat([z, fea5], dim=1), t)
    diff = target - out
    term = diff.abs() if d.loss_type == "l1" else diff * diff
    w = tabs["weight"].double()[t]
    return float((w * term.reshape(b, -1).mean(1)).mean()), t


@pytest.mark.parametrize("dyn", [False, True], ids=["static", "dynamic"])
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("objective", ["pred_v", "pred_x0"])
def test_loss_against_float64(backend, objective, loss_type, dyn):
    dev = backend
    d = _distilling(dev, objective, loss_type, use_dynamic_thres=dyn)
    shape, x0, noise, fea, _ = _stub_inputs(dev)
    torch.manual_seed(7)
    loss = d(x0, fea, None)
    torch.manual_seed(7)
    k = torch.randint(0, N, (3,), device=dev).long()
    nz = torch.randn_like(x0)
    want, t = _restate(d, x0, fea, k, nz, dyn)
    got = float(loss)
    print("distillation step %s %s %s: %.9g against %.9g, relative %.3g" % (objective, loss_type, dyn, got, want, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-5 * abs(want)
    assert torch.equal(d.sample_t.cpu(), t) and d.sample_t.dtype == torch.int64
    assert d.sample_loss.shape == (3,) and d.pred_x0.shape == shape and bool(torch.isfinite(d.pred_x0).all())
    assert float(d.pred_x0.abs().max()) <= 1.0


@pytest.mark.parametrize("objective", ["pred_v", "pred_x0"])
def test_weight_choices_and_refusals(backend, objective):
    dev = backend
    shape, x0, noise, fea, _ = _stub_inputs(dev)
    for weight in ("truncated_snr", "min_snr", None):
        d = _distilling(dev, objective, distill_weight=weight, min_snr_gamma=5.0)
        torch.manual_seed(7)
        got = float(d(x0, fea, None))
        torch.manual_seed(7)
        want, _ = _restate(d, x0, fea, torch.randint(0, N, (3,), device=dev).long(), torch.randn_like(x0), False)
        assert abs(got - want) <= 1e-5 * abs(want)
    # (each against the restatement under ITS weight table; which of the three coincide depends on the k drawn - max(snr, 1) is 1 below snr 1)
    with pytest.raises(ValueError, match="known_mask"):
        d(x0, fea, None, known_mask=torch.zeros(3, 5, dtype=torch.bool, device=dev))
    d.set_distill(None)
    assert d._distill is None and d._distill_dev == {}


@pytest.mark.parametrize("objective", ["pred_v", "pred_x0"])
def test_target_is_a_convex_combination(backend, objective):
    """In real arithmetic x_target = (K2 / k) m2 + (X2 K1 / k) m1 with K, X the k_x0, k_x of the teacher's two rows and k the student's k_x0:
    the weights sum to 1 and the z terms cancel, so x_target lies between the two thresholded teacher predictions, up to x_target's own
    bar of test_distill_ops.py for the second step, 8 E (|q0| S2 + |q0 z''| + |q1 z|).  (The first step's rounding of z' - its own bar,
    8 E S1 - is carried into z'' times |q0 X2| on top of that; m2 is computed here from the same stored z', and the bar has room for it:
    nothing is added to it.)  Every row of the round is covered."""
    dev = backend
    d = _distilling(dev, objective)
    tabs = {k: v.to(dev) for k, v in d.distill_tables(N).items()}
    shape = (N, 3, 5, 4, 4)
    z, out1, out2 = rnd(*shape, seed=41).to(dev) * 2, rnd(*shape, seed=42).to(dev) * 2, rnd(*shape, seed=43).to(dev) * 2
    k = torch.arange(N, device=dev)
    coef, row1, row2 = tabs["teacher_coef"], 2 * k, 2 * k + 1
    m1 = ops.distill_x0(z, out1, coef, row1).clamp(-1, 1)
    z1 = ops.distill_step(z, out1, coef, row1)
    m2 = ops.distill_x0(z1, out2, coef, row2).clamp(-1, 1)
    z2, x_target, _ = ops.distill_step(z1, out2, coef, row2, None, torch.empty_like(z), x_ref=z, tcoef=tabs["target_coef"], trow=k)
    shp = (N, 1, 1, 1, 1)
    c1, c2 = coef[row1].double().cpu(), coef[row2].double().cpu()
    q = tabs["target_coef"].double().cpu()
    col = lambda tab, j: tab[:, j].reshape(shp)
    big = lambda c, x, o: col(c, 2).abs() * ((col(c, 0) * x).abs() + (col(c, 1) * o).abs()) + (col(c, 4) * x).abs()
    z64, z164, z264 = z.cpu().double(), z1.cpu().double(), z2.cpu().double()
    s2 = big(c2, z164, out2.cpu().double())
    bar = 8 * E * (col(q, 0).abs() * s2 + (col(q, 0) * z264).abs() + (col(q, 1) * z64).abs())
    lo, hi = torch.minimum(m1, m2).cpu().double(), torch.maximum(m1, m2).cpu().double()
    xt = x_target.cpu().double()
    print("convexity %s: largest excess / bar = %.3g" % (objective, float(torch.maximum((lo - xt) / bar, (xt - hi) / bar).max())))
    assert bool((xt >= lo - bar).all()) and bool((xt <= hi + bar).all())
    # the weights themselves, in double on the fp32 tables: they sum to 1 up to the tables' rounding
    w2, w1 = col(c2, 2) * col(q, 0), col(c2, 4) * col(c1, 2) * col(q, 0)
    assert float((w1 + w2 - 1).abs().max()) <= 8 * 2.0 ** -24 * float((w1.abs() + w2.abs()).max())


@pytest.mark.parametrize("k0", [0, 1, N - 1])
@pytest.mark.parametrize("objective", ["pred_v", "pred_x0"])
def test_closed_loop_through_the_sampler(backend, monkeypatch, objective, k0):
    """What the student is trained to output, fed through the sampler's own update kernel on row k of the N-step "trailing" eta-0 table
    under the static clamp, lands on the teacher's z'': within 16 E (max |z''| + |k_x| max |z|) - inverting and re-applying the row cost at
    most 4 E of those terms each, a 2x margin - and twice that for "pred_v" (the round trip through v = a eps_target - s x_target and
    back through x0 = a z - s v).  |x_target| <= 1 up to rounding (convexity), so the student's clamp is the identity: no pass by clipping."""
    dev = backend
    d = _distilling(dev, objective)
    seen, real_step = _record(monkeypatch)
    real_randint = torch.randint
    monkeypatch.setattr(torch, "randint", lambda lo, hi, size, **kw: torch.full(size, k0, dtype=torch.int64, device=kw.get("device")))
    shape, x0, noise, fea, _ = _stub_inputs(dev)
    d(x0, fea, None, noise=noise)
    monkeypatch.setattr(torch, "randint", real_randint)
    (a1, _, z1), (a2, k2, (none, x_target, eps_target)) = seen
    z = a1[0]
    assert none is None and k2["x_ref"] is z and a2[0] is z1 and bool((k2["trow"] == k0).all()) and bool((a2[3] == 2 * k0 + 1).all())
    z2 = real_step(*a2[:5])             # the teacher's second step once more, with z'' stored
    t = int(d.sample_t[0])
    if objective == "pred_x0":
        value = x_target
    else:
        value = float(d.sqrt_alphas_cumprod[t]) * eps_target - float(d.sqrt_one_minus_alphas_cumprod[t]) * x_target
    sampler = GaussianDiffusion(_StubDenoiser(), image_size=4, num_frames=5, timesteps=TIMESTEPS, sampling_timesteps=N, ddim_sampling_eta=0.0,
                                loss_type="l2", objective=objective, step_grid="trailing", schedule="cosine_zsnr")
    times, coef, _ = sampler._step_tables(True)
    assert times[k0] == t
    x = z.clone()
    ops.sampler_step(x, value.contiguous(), torch.zeros_like(x), coef.to(dev), torch.tensor([k0], dtype=torch.int32, device=dev),
                     quantile=-1.0)
    bound = 16 * E * (float(z2.abs().max()) + abs(float(coef[k0, 4])) * float(z.abs().max())) * (2 if objective == "pred_v" else 1)
    err = float((x - z2).abs().max())
    print("closed loop %s k = %d: largest error %.3g, bound %.3g; max |x_target| %.6f" % (objective, k0, err, bound, float(x_target.abs().max())))
    assert float(x_target.abs().max()) <= 1.0 + 8 * E * 16
    assert err <= bound


def test_off_is_the_parents_step(backend, monkeypatch):
    """Distillation off - never set, or set and taken back: neither new op is called, and `forward` gives the loss bits it gave."""
    dev = backend

    def forbidden(*a, **k):
        raise AssertionError("a distillation op was called with distillation off")

    shape, x0, noise, fea, _ = _stub_inputs(dev)
    used = _distilling(dev, "pred_v", min_snr_gamma=5.0)
    torch.manual_seed(3)
    used(x0, fea, None)
    used.set_distill(None)
    for name in ("distill_x0", "distill_step"):
        monkeypatch.setattr(ops, name, forbidden)
    fresh = _stub_diffusion(dev, objective="pred_v", step_grid="trailing", schedule="cosine_zsnr", min_snr_gamma=5.0)
    torch.manual_seed(3)
    a = used(x0, fea, None)
    torch.manual_seed(3)
    b = fresh(x0, fea, None)
    assert torch.equal(a, b) and torch.equal(used.sample_t, fresh.sample_t)
    d = _stub_diffusion(dev)                     # the reference's step: the eager expression's bits (test_train_known.py)
    torch.manual_seed(3)
    loss = d(x0, fea, None)
    torch.manual_seed(3)
    tt = torch.randint(0, TIMESTEPS, (3,), device=dev).long()
    nz = torch.randn_like(x0)
    want = torch.nn.functional.mse_loss(nz, d.q_sample(x0, tt, nz) * 0.5 + 0.1)
    assert torch.equal(loss.detach(), want)


def test_state_dict_keeps_its_keys():
    """The teacher is no sub-module and the tables are no buffers: 324 keys before, during and after (host only)."""
    import synth
    from cvpr23_lfdm_amd import Unet3D
    unet = Unet3D(dim=64, channels=259, out_grid_dim=2, out_conf_dim=1, use_bert_text_cond=True)
    unet.load_state_dict(synth.unet_state())
    d = GaussianDiffusion(unet, image_size=8, num_frames=4, timesteps=TIMESTEPS, sampling_timesteps=10, loss_type="l2", objective="pred_v",
                          step_grid="trailing")
    keys = list(d.state_dict())
    assert len(keys) == 324
    teacher = copy.deepcopy(unet).train()
    d.set_distill(teacher, N)
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters())
    assert list(d.state_dict()) == keys and len(list(d.parameters())) == len(list(unet.parameters()))
    assert all(p.requires_grad for p in unet.parameters()) and teacher not in list(d.modules())
    d.train()
    assert not teacher.training
    d.set_distill(None)
    assert list(d.state_dict()) == keys


def test_skip_step_draws_follows(backend):
    dev = backend
    rng_state = (lambda: torch.cuda.get_rng_state()) if dev == "cuda" else torch.get_rng_state
    shape, x0, noise, fea, _ = _stub_inputs(dev, b=4)
    d = _distilling(dev, "pred_v")
    torch.manual_seed(1)
    d(x0, fea, None)
    after_step = rng_state()
    torch.manual_seed(1)
    d.skip_step_draws(4, shape[1:], dev)
    assert torch.equal(rng_state(), after_step)
    # two simulated ranks see the halves of the one-process draws
    torch.manual_seed(1)
    d(x0, fea, None)
    whole = d.sample_t.clone()
    for r in range(2):
        torch.manual_seed(1)
        d.rank_shard = (r, 2)
        d(x0[2 * r:2 * r + 2], fea[2 * r:2 * r + 2], None)
        assert torch.equal(d.sample_t, whole[2 * r:2 * r + 2]) and torch.equal(rng_state(), after_step)


# ------------------------------------------------------------------------------------------------------------------------------------
# through the native UNet

def test_unet_grads(backend, monkeypatch):
    """Loss and every parameter gradient of one distillation step through the native UNet against autograd through the oracle's UNet on
    the kernel-made targets, at test_p_losses_masked_unet_grads' bars (1e-3 forward, 2e-3 of the largest gradient).  The teacher is a copy
    of the student."""
    dev = backend
    if dev == "cpu" and os.environ.get("LFDM_EMU_E2E", "0") != "1":
        pytest.skip("UNet forward+backward under the emulator is opt-in (LFDM_EMU_E2E=1); it runs on the GPU")
    import lfdm_oracle as O
    import synth
    from cvpr23_lfdm_amd import Unet3D
    b, frames, s = (1, 2, 8) if dev == "cpu" else (2, 4, 8)
    usd = synth.unet_state()
    unet = Unet3D(dim=64, channels=259, out_grid_dim=2, out_conf_dim=1, use_bert_text_cond=True)
    unet.load_state_dict(usd)
    unet.to(dev).train()
    d = GaussianDiffusion(unet, image_size=s, num_frames=frames, timesteps=TIMESTEPS, sampling_timesteps=10, loss_type="l2", null_cond_prob=0.0,
                          objective="pred_v", step_grid="trailing", schedule="cosine_zsnr").to(dev)
    d.set_distill(copy.deepcopy(unet), N)
    x, _, cond = synth.unet_inputs(b, frames, s)
    shape = (b, 3, frames, s, s)
    x0, fea = x[:, :3].contiguous(), x[:, 3:, 0].contiguous()
    noise = synth.NoiseTape(11)(shape)
    seen, _ = _record(monkeypatch)
    unet.zero_grad()
    torch.manual_seed(9)
    loss = d(x0.to(dev), fea.to(dev), cond.to(dev), noise=noise.to(dev))
    loss.backward()
    (a1, _, _), (_, _, (_, x_target, eps_target)) = seen
    z, t = a1[0].cpu(), d.sample_t.cpu()
    sd = {"denoise_fn." + k: v.clone().requires_grad_(v.is_floating_point() and "rotary" not in k) for k, v in usd.items()}
    pred = O.unet_forward(sd, torch.cat([z, x[:, 3:]], dim=1), t, cond)
    shp = (b, 1, 1, 1, 1)
    a, sg = d.sqrt_alphas_cumprod.cpu().double()[t].reshape(shp), d.sqrt_one_minus_alphas_cumprod.cpu().double()[t].reshape(shp)
    target = a * eps_target.cpu().double() - sg * x_target.cpu().double()
    w = d.distill_tables(N)["weight"].double()[t]
    ref = (w * ((target - pred.double()) ** 2).reshape(b, -1).mean(1)).mean()
    ref.backward()
    print("distillation step through the UNet: loss %.9g against %.9g" % (float(loss.detach()), float(ref.detach())))
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-3 * max(1.0, abs(float(ref.detach())))
    worst = ("", 0.0)
    for k, p in unet.named_parameters():
        rg = sd["denoise_fn." + k].grad
        assert p.grad is not None and rg is not None, k
        err = float((p.grad.cpu().double() - rg).abs().max()) / (float(rg.abs().max()) + 1e-12)
        if err > worst[1]:
            worst = (k, err)
    assert worst[1] < 2e-3, "largest relative gradient error %.3e at %s" % (worst[1], worst[0])
    assert all(p.grad is None for p in d._distill["teacher"].parameters())


def test_begin_distill_round_trains_the_student_only(backend):
    """begin_distill_round, then two optimize_parameters() from a stored latent with EMA and the non-finite guard on: the student's weights
    move, the teacher's stay bit for bit, sampling is set to the student's schedule."""
    import synth
    from test_latent_store import _model
    dev = backend
    hw, frames = 16, 2
    m = _model(dev, hw, frames, objective="pred_v", step_grid="trailing", schedule="cosine_zsnr", ema_decay=0.9, skip_nonfinite=True,
               max_grad_norm=1.0)
    before = {k: v.detach().clone() for k, v in m.unet.named_parameters()}
    teacher = m.begin_distill_round(N)
    assert teacher is not m.unet and m.diffusion.sampling_timesteps == N and m.diffusion.ddim_sampling_eta == 0.0 and m.diffusion.is_ddim_sampling
    assert len(m.diffusion.state_dict()) == len(m.unet.state_dict()) + 12
    ref_img, _, cond, _, noise = synth.train_inputs(1, frames, hw)
    latent = (0.4 * noise).clamp(-1, 1)
    packs = []
    for seed in (5, 6):
        torch.manual_seed(seed)
        m.set_train_latent(ref_img.to(dev), latent.to(dev), cond.to(dev))
        m.optimize_parameters()
        assert bool(torch.isfinite(m.loss))
        packs.append(teacher._pk)
    # the frozen teacher is in no optimizer: it keeps its weight pack while the student's optimizer steps, and rebuilds it after a load
    assert packs[0] is not None and packs[1] is packs[0] and teacher.packed() is packs[0]
    teacher.load_state_dict(teacher.state_dict())
    assert teacher.packed() is not packs[0]
    student_pack = m.unet.packed()
    m.optimizer_diff.step()
    assert m.unet.packed() is not student_pack          # (a trained denoiser's pack still follows the optimizer)
    moved = [k for k, v in m.unet.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert len(moved) > len(before) // 2
    for k, v in teacher.named_parameters():
        assert torch.equal(v, before[k]), k
    m.end_distill()
    assert m.diffusion._distill is None
