"""Training objectives through the model: GaussianDiffusion.p_losses on the kernel route against its eager restatement;
whole videos of a "pred_v" / "pred_x0" model against a loop over the oracle's own pieces (its UNet, its threshold, its schedule) with the
textbook update of each sampler written out here; the plumbing on the GPU; the drivers' flags and the checkpoint's objective entry.
Bars are those of test_train_known.py (loss 1e-5 around the stub, 1e-3 / 2e-3 through the UNet) and of the sampling tests (1e-3; 2e-3
between batch sizes)."""
import importlib.util
import math
import os

import pytest
import torch

import lfdm_oracle as O
import synth
from cvpr23_lfdm_amd import GaussianDiffusion, ops
from test_known_frames import _decode, _gpu, _skip_slow_emu, ms_levels
from test_train_known import TIMESTEPS, _stub_diffusion, _stub_inputs
from util import assert_close

GAMMA = 5.0
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bc(v, b):
    return v.reshape(b, 1, 1, 1, 1)


def _eager(d, objective, x0, noise, t, full, denoiser, loss_type, weighted):
    """The step restated with torch: x_noisy and the target in fp32 as the kernels form them, the weighted masked mean in float64.
    -> (loss, out, pred_x0 before clipping, per-sample means); everything on the host."""
    b = x0.shape[0]
    a, s, r, m = (_bc(getattr(d, k).cpu()[t], b) for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
                                                            "sqrt_recipm1_alphas_cumprod"))
    x_noisy = torch.where(full, x0, a * x0 + s * noise)
    out = denoiser(x_noisy)
    o = out.detach()
    target = {"pred_noise": noise, "pred_x0": x0, "pred_v": a * noise - s * x0}[objective]
    pred_x0 = torch.where(full, x_noisy, {"pred_noise": r * x_noisy - m * o, "pred_x0": o, "pred_v": a * x_noisy - s * o}[objective])
    diff = target.double() - out.double()
    term = (diff.abs() if loss_type == "l1" else diff * diff) * (~full)
    means = term.reshape(b, -1).sum(1) / (~full).reshape(b, -1).sum(1).clamp(min=1)
    w = d.loss_weight.cpu()[t].double() if weighted else torch.ones(b, dtype=torch.float64)
    return (w * means).mean(), out, pred_x0, means


# ------------------------------------------------------------------------------------------ 1. training, around the stub denoiser
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("form", ["none", "frame", "elem1"])
@pytest.mark.parametrize("objective,gamma", [("pred_v", GAMMA), ("pred_v", None), ("pred_x0", GAMMA), ("pred_noise", GAMMA)])
def test_p_losses_objective_edge(backend, objective, gamma, form, loss_type):
    dev = backend
    d = _stub_diffusion(dev, loss_type, objective=objective, min_snr_gamma=gamma)
    shape, x0, noise, fea, t = _stub_inputs(dev)
    g = torch.Generator().manual_seed(5)
    mask = {"none": None, "frame": torch.rand(3, 5, generator=g) < 0.5, "elem1": torch.rand(3, 1, 5, 4, 4, generator=g) < 0.5}[form]
    full = torch.zeros(shape, dtype=torch.bool) if mask is None else (mask[:, None, :, None, None] if form == "frame" else mask).expand(shape)
    kw = {} if mask is None else dict(known_mask=mask.to(dev))
    loss = d.p_losses(x0, t, fea, noise=noise, clip_denoised=False, **kw)
    want, _, px0, means = _eager(d, objective, x0.cpu(), noise.cpu(), t.cpu(), full, lambda x: x * 0.5 + 0.1, loss_type, gamma is not None)
    print("p_losses %s gamma %s %s %s: %.9g against %.9g" % (objective, gamma, form, loss_type, float(loss), float(want)))
    assert loss.dim() == 0 and abs(float(loss) - float(want)) <= 1e-5 * abs(float(want))
    assert torch.equal(d.pred_x0.cpu(), px0)                                     # clip_denoised=False: the kernel's pred_x0 itself
    assert tuple(d.sample_loss.shape) == (3,) and d.sample_loss.device == x0.device and torch.equal(d.sample_t, t)
    assert bool(((d.sample_loss.cpu().double() - means).abs() <= 1e-5 * means.abs()).all())
    d.p_losses(x0, t, fea, noise=noise, **kw)
    assert torch.equal(d.pred_x0.cpu(), px0.clamp(-1, 1))                        # and the clipped one is that, clipped


def test_p_losses_objective_refuses(backend):
    dev = backend
    shape, x0, noise, fea, t = _stub_inputs(dev)
    for kw in (dict(objective="pred_v"), dict(min_snr_gamma=GAMMA)):
        d = _stub_diffusion(dev, per_element_loss=True, **kw)
        with pytest.raises(NotImplementedError, match="per_element_loss"):
            d.p_losses(x0, t, fea, noise=noise)


def test_defaults_with_a_mask_call_the_ops_they_called(backend, monkeypatch):
    """Default objective and no weight: a known mask takes the masked-loss ops, never the new ones."""
    dev = backend

    def forbidden(*a, **k):
        raise AssertionError("an objective op was called with the default objective")

    for name in ("objective_loss_fwd", "objective_loss_bwd"):
        monkeypatch.setattr(ops, name, forbidden)
    d = _stub_diffusion(dev)
    shape, x0, noise, fea, t = _stub_inputs(dev)
    mask = torch.zeros(3, 5, dtype=torch.bool)
    mask[:, :2] = True
    assert torch.isfinite(d.p_losses(x0, t, fea, noise=noise, known_mask=mask.to(dev)))
    assert torch.isfinite(d.p_losses(x0, t, fea, noise=noise)) and d.sample_loss is None


def test_known_policy_and_draws_are_untouched(backend, monkeypatch):
    """known_train composes: the policy's masks and the default generator's state after a step are those of the default objective, in one
    process and as one of two ranks."""
    dev = backend
    kw = dict(prob=1.0, max_frames=3, seed=11)
    shape, x0, noise, fea, t = _stub_inputs(dev, b=4)
    seen = []
    real = ops.train_qsample
    monkeypatch.setattr(ops, "train_qsample", lambda *a, **k: (seen.append(k["frame_mask"].cpu().clone()), real(*a, **k))[1])
    rng_state = (lambda: torch.cuda.get_rng_state()) if dev == "cuda" else torch.get_rng_state
    runs = {}
    for name, extra in (("default", {}), ("pred_v", dict(objective="pred_v", min_snr_gamma=GAMMA))):
        for shard in (None, (1, 2)):
            torch.manual_seed(1)
            d = _stub_diffusion(dev, known_train=kw, **extra)
            d.rank_shard = shard
            lo, hi = (0, 4) if shard is None else (2, 4)
            masks = []
            for _ in range(2):
                d(x0[lo:hi], fea[lo:hi], None)
                masks.append(seen.pop())
            runs[name, shard] = (masks, rng_state(), d.sample_t)
    for shard in (None, (1, 2)):
        (m0, s0, _), (m1, s1, t1) = runs["default", shard], runs["pred_v", shard]
        assert all(torch.equal(a, b) for a, b in zip(m0, m1)) and torch.equal(s0, s1)
    assert torch.equal(runs["pred_v", (1, 2)][2], runs["pred_v", None][2][2:])          # the rank's t: its rows of the global draw
    assert all(torch.equal(a[2:], b) for a, b in zip(runs["pred_v", None][0], runs["pred_v", (1, 2)][0]))


# ------------------------------------------------------------------------------------------ 2. training, through the native UNet
def _unet_case(dev, form):
    from cvpr23_lfdm_amd import Unet3D
    b, frames, s = (1, 2, 8) if dev == "cpu" else (2, 4, 8)
    usd = synth.unet_state()
    unet = Unet3D(dim=64, channels=259, out_grid_dim=2, out_conf_dim=1, use_bert_text_cond=True)
    unet.load_state_dict(usd)
    unet.to(dev).train()
    d = GaussianDiffusion(unet, image_size=s, num_frames=frames, timesteps=TIMESTEPS, sampling_timesteps=10, loss_type="l2", null_cond_prob=0.0,
                          objective="pred_v", min_snr_gamma=GAMMA).to(dev)
    x, time, cond = synth.unet_inputs(b, frames, s)
    shape = (b, 3, frames, s, s)
    x0, fea = x[:, :3].contiguous(), x[:, 3:, 0].contiguous()
    noise = synth.NoiseTape(11)(shape)
    g = torch.Generator().manual_seed(6)
    mask = torch.rand(b, frames, generator=g) < 0.5 if form == "frame" else None
    full = torch.zeros(shape, dtype=torch.bool) if mask is None else mask[:, None, :, None, None].expand(shape)
    sd = {"denoise_fn." + k: v.clone().requires_grad_(v.is_floating_point() and "rotary" not in k) for k, v in usd.items()}
    ref, _, _, _ = _eager(d, "pred_v", x0, noise, time, full, lambda xn: O.unet_forward(sd, torch.cat([xn, x[:, 3:]], dim=1), time, cond), "l2", True)
    ref.backward()
    unet.zero_grad()
    kw = {} if mask is None else dict(known_mask=mask.to(dev))
    loss = d.p_losses(x0.to(dev), time.to(dev), fea.to(dev), cond=cond.to(dev), noise=noise.to(dev), **kw)
    loss.backward()
    return unet, sd, loss, ref


@pytest.mark.parametrize("form", ["none", "frame"])
def test_p_losses_pred_v_unet_grads(backend, form):
    """pred_v with gamma = 5: loss and every parameter gradient through the native UNet, at test_unet_train's bars (1e-3 forward, 2e-3 of
    the largest gradient)."""
    dev = backend
    if dev == "cpu" and os.environ.get("LFDM_EMU_E2E", "0") != "1":
        pytest.skip("UNet forward+backward under the emulator is opt-in (LFDM_EMU_E2E=1); it runs on the GPU")
    unet, sd, loss, ref = _unet_case(dev, form)
    print("p_losses pred_v %s: loss %.9g against %.9g" % (form, float(loss.detach()), float(ref.detach())))
    assert abs(float(loss) - float(ref)) <= 1e-3 * max(1.0, abs(float(ref)))
    worst = ("", 0.0)
    for k, p in unet.named_parameters():
        rg = sd["denoise_fn." + k].grad
        assert p.grad is not None and rg is not None, k
        err = float((p.grad.cpu().double() - rg).abs().max()) / (float(rg.abs().max()) + 1e-12)
        if err > worst[1]:
            worst = (k, err)
    assert worst[1] < 2e-3, "largest relative gradient error %.3e at %s" % (worst[1], worst[0])


# ------------------------------------------------------------------------------------------ 3. whole videos against the oracle's pieces
def oracle_objective_latent(kind, objective, sd, fea, cond, shape, steps, total, cond_scale, noise_fn, known=None, sel=None, eta=1.0):
    """The sampling loop over the oracle's UNet, threshold and schedule with the textbook update of `kind` ("ddim" | "ddpm" | "dpmpp_2m")
    for a denoiser whose output is v ("pred_v": x0 = a x - s out) or x0 itself ("pred_x0"); a, s at alphas_cumprod[time].  DDIM adds c
    times the noise implied by the thresholded x0, (x - a x0c) / s.  known / sel: the clean select of test_known_clean.py."""
    b, _, frames, _, _ = shape
    hold = (lambda x: x) if sel is None else (lambda x: torch.where(sel, known, x))
    x = hold(noise_fn(tuple(shape)))
    fea_rep = fea.unsqueeze(2).repeat(1, 1, frames, 1, 1)

    def predict(x, time):
        t = torch.full((b,), time, dtype=torch.long)
        out = O.unet_forward_with_cond_scale(sd, torch.cat([x, fea_rep], dim=1), t, cond, cond_scale)
        a, s = sd["sqrt_alphas_cumprod"][time], sd["sqrt_one_minus_alphas_cumprod"][time]
        return O.dynamic_threshold(a * x - s * out if objective == "pred_v" else out), a.double(), s.double()

    if kind == "ddpm":
        for time in reversed(range(total)):
            z = noise_fn(tuple(shape))                      # p_sample draws on every step
            x0c, _, _ = predict(x, time)
            mean = sd["posterior_mean_coef1"][time] * x0c + sd["posterior_mean_coef2"][time] * x
            x = hold(mean + (0.0 if time == 0 else 1.0) * (0.5 * sd["posterior_log_variance_clipped"][time]).exp() * z)
        return x
    pairs = O.ddim_time_pairs(total, steps)
    if kind == "ddim":
        for time, time_next in pairs:
            z = noise_fn(tuple(shape)) if time_next > 0 else 0.0
            x0c, a, s = predict(x, time)
            alpha, alpha_next = sd["alphas_cumprod_prev"][time], sd["alphas_cumprod_prev"][time_next]
            sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            c = ((1 - alpha_next) - sigma ** 2).sqrt()
            eps_hat = (x.double() - a * x0c.double()) / s
            x = hold((alpha_next.sqrt().double() * x0c.double() + c.double() * eps_hat).float() + sigma * z)
        return x
    lv = ms_levels(total, steps)
    m_prev, h_prev = None, None
    for i, (time, _) in enumerate(pairs):
        last = i == len(pairs) - 1
        (al_s, sg_s), (al_n, sg_n) = lv[i], lv[i + 1]
        m = predict(x, time)[0].double()
        k = al_n - sg_n * al_s / sg_s
        h = math.inf if last else math.log(al_n / sg_n) - math.log(al_s / sg_s)
        if i == 0 or last:
            new = (sg_n / sg_s) * x.double() + k * m
        else:
            r = h_prev / h
            new = (sg_n / sg_s) * x.double() + k * (1 + 1 / (2 * r)) * m - k / (2 * r) * m_prev
        x, m_prev, h_prev = hold(new.float()), m, h
    return x


VIDEO_CASES = [(kind, objective, scale, False) for kind in ("ddim", "dpmpp_2m") for objective in ("pred_v", "pred_x0") for scale in (1.0, 2.0)]
VIDEO_CASES += [("ddpm", "pred_v", 1.0, False), ("ddim", "pred_v", 1.0, True)]


@pytest.mark.parametrize("kind,objective,cond_scale,clean", VIDEO_CASES)
def test_sample_one_video_objective(backend, kind, objective, cond_scale, clean):
    dev = backend
    _skip_slow_emu(dev)
    b, t, s, hw, steps = 1, 4, 8, 32, 6
    total = 6 if kind == "ddpm" else 1000
    m, dsd, gsd = synth.build_flow_diffusion(dev, img_size=s, num_frames=t, sampling_timesteps=steps, timesteps=total,
                                             sampler="dpmpp_2m" if kind == "dpmpp_2m" else "reference", objective=objective)
    assert m.diffusion.objective == objective and m.diffusion.is_ddim_sampling == (kind != "ddpm")
    img, cond = synth.inputs(b, hw)
    sd = dict(dsd)
    sd.update(O.make_schedule(total))
    shape = (b, 3, t, s, s)
    known, mask, sel, kw = None, None, None, {}
    if clean:
        known = synth.NoiseTape(23)(shape).clamp(-1, 1).contiguous()
        mask = torch.zeros(b, t, dtype=torch.bool)
        mask[:, :2] = True
        sel = mask[:, None, :, None, None].expand(shape)
        kw = dict(known_latent=known.to(dev), known_mask=mask.to(dev), known_level="clean")
    fea = O.generator_compute_fea(gsd, img)
    lat = oracle_objective_latent(kind, objective, sd, fea, cond, shape, steps, total, cond_scale, synth.NoiseTape(11), known, sel)
    ref = _decode(gsd, img, lat, t)
    m.diffusion.noise_source = synth.NoiseTape(11)
    m.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))
    m.sample_one_video(cond_scale=cond_scale, **kw)
    for name in ("sample_vid_grid", "sample_vid_conf", "sample_warped_vid", "sample_out_vid"):
        assert_close(getattr(m, name).cpu(), ref[name], 1e-3, "%s (%s, %s, cond_scale %g, clean %s)" % (name, kind, objective, cond_scale, clean))
    if clean:
        got = m.sample_latent.cpu()
        assert torch.equal(got[sel], known[sel])
        assert float((got[~sel] - known[~sel]).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------ 4. plumbing on the GPU
def _pred_v_model(sampler, noise="torch"):
    return synth.build_flow_diffusion("cuda", img_size=8, num_frames=4, sampling_timesteps=7, sampler=sampler, noise=noise, objective="pred_v")[0]


def _video(m, seed, tape=True, **kw):
    img, cond = synth.inputs(1, 32, seed=seed)
    m.diffusion.noise_source = synth.NoiseTape(seed) if tape else None
    m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
    m.sample_one_video(cond_scale=1.0, **kw)
    return m.sample_latent.clone()


@pytest.mark.gpu
def test_graph_chunks_do_not_change_a_pred_v_video(monkeypatch):
    _gpu()
    outs = {}
    for steps in ("1", "10"):
        monkeypatch.setenv("LFDM_GRAPH_STEPS", steps)
        a = _video(_pred_v_model("dpmpp_2m"), 5)
        torch.manual_seed(77)
        b = _video(_pred_v_model("reference"), 5, tape=False)          # DDIM eta 1 with torch's generator under a fixed seed
        outs[steps] = (a, b)
    for x, y in zip(outs["1"], outs["10"]):
        assert torch.isfinite(x).all() and torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", ["reference", "dpmpp_2m"])
def test_a_pred_v_counter_video_is_its_seed(sampler):
    """noise="counter": the video of seed s alone and as the second of three, within 2e-3 (launch plans differ with the batch)."""
    _gpu()
    a, s, c = (1 << 63) + 11, 77, 5
    img, cond = synth.inputs(1, 32)

    def run(seeds):
        m = _pred_v_model(sampler, noise="counter")
        n = len(seeds)
        m.set_sample_input(sample_img=img.expand(n, -1, -1, -1).contiguous().cuda(), sample_text=cond.expand(n, -1).contiguous().cuda())
        m.sample_one_video(cond_scale=1.0, seeds=seeds)
        return m.sample_latent.cpu().clone()

    alone, three = run([s]), run([a, s, c])
    assert_close(three[1:2], alone, 2e-3, "pred_v video of seed s, second of three (%s)" % sampler)
    assert float((three[0:1] - alone).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------ 5. drivers
def _tool(name):
    spec = importlib.util.spec_from_file_location("lfdm_tool_" + name, os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_flags_parse():
    train = _tool("train_dm")
    args = train.parse_args([])
    assert args.objective == "pred_noise" and args.min_snr_gamma is None and args.log_loss_quartiles is False
    args = train.parse_args(["--objective", "pred_v", "--min-snr-gamma", "5", "--log-loss-quartiles"])
    assert args.objective == "pred_v" and args.min_snr_gamma == 5.0 and args.log_loss_quartiles is True
    with pytest.raises(SystemExit):
        train.parse_args(["--objective", "pred_eps"])
    assert _tool("demo").build_parser().parse_args([]).objective is None
    assert _tool("demo").build_parser().parse_args(["--objective", "pred_x0"]).objective == "pred_x0"
    assert _tool("eval").build_parser().parse_args(["dm", "--objective", "pred_v"]).objective == "pred_v"
    assert _tool("eval").build_parser().parse_args(["dm"]).objective is None


def test_loss_quartiles_accumulate_by_timestep():
    q = _tool("train_dm").LossQuartiles(1000)
    assert all(math.isnan(v) for v in q.means())
    q.add(torch.tensor([1.0, 3.0, 10.0]), torch.tensor([0, 249, 250]))
    q.add(torch.tensor([4.0, 7.0]), torch.tensor([999, 750]))
    got = q.means()
    assert got[0] == 2.0 and got[1] == 10.0 and math.isnan(got[2]) and got[3] == 5.5
    assert all(math.isnan(v) for v in q.means())                                         # printed: it starts again


def test_checkpoint_carries_the_objective(tmp_path):
    from cvpr23_lfdm_amd import io_compat as C
    d = GaussianDiffusion(torch.nn.Identity(), image_size=8, num_frames=4, timesteps=50, sampling_timesteps=10, objective="pred_v", min_snr_gamma=GAMMA)
    path = str(tmp_path / "flowdiff.pth")
    torch.save({"example": 8, "diffusion": d.state_dict(), "objective": d.objective, "min_snr_gamma": d.min_snr_gamma}, path)
    ck = torch.load(path, map_location="cpu")
    assert ck["min_snr_gamma"] == GAMMA and "loss_weight" not in ck["diffusion"]
    assert C.checkpoint_objective(ck) == "pred_v" and C.checkpoint_objective(ck, "pred_v", path) == "pred_v"
    with pytest.raises(ValueError, match="pred_x0.*pred_v"):
        C.checkpoint_objective(ck, "pred_x0", path)
    old = {"diffusion": d.state_dict()}                                                  # the reference's checkpoints: no entry
    assert C.checkpoint_objective(old) == "pred_noise" and C.checkpoint_objective(None) == "pred_noise"
    assert C.checkpoint_objective(None, "pred_v") == "pred_v"
    with pytest.raises(ValueError, match="pred_v.*pred_noise"):
        C.checkpoint_objective(old, "pred_v")
    again = GaussianDiffusion(torch.nn.Identity(), image_size=8, num_frames=4, timesteps=50, sampling_timesteps=10,
                              objective=C.checkpoint_objective(ck))
    again.load_state_dict(ck["diffusion"])
    assert torch.equal(again._step_tables(True)[1], GaussianDiffusion(torch.nn.Identity(), image_size=8, num_frames=4, timesteps=50,
                                                                      sampling_timesteps=10, objective="pred_v")._step_tables(True)[1])
