"""Joint long videos: FlowDiffusion.sample_long_video(method="joint") against a loop written here from the oracle's
pieces - O.unet_forward_with_cond_scale per window, the fold restated in float64, O.dynamic_threshold and the schedule of O.make_schedule,
the DDIM / DDPM / 2M update written out as test_known_frames.oracle_known_latent does.  The loop is pinned first: with one window it is
torch.equal to O.sample on the same tape.  Sizes as test_known_frames._sizes; whole videos under the emulator are opt-in (LFDM_EMU_E2E=1),
as everywhere.  Window starts and weights are the design's formulas, written out in test_window_fold."""
import math
import os

import numpy as np
import pytest
import torch

import lfdm_oracle as O
import synth
from test_known_frames import _decode, _sizes, _skip_slow_emu, ms_levels
from test_window_fold import design_starts, design_table
from util import assert_close

NAMES = ("sample_vid_grid", "sample_vid_conf", "sample_warped_vid", "sample_out_vid")
STEPS = 6


def _guided(sd, xin, t, cond, cond_scale, phi):
    """O.unet_forward_with_cond_scale; with phi > 0 the guidance rescale of DESIGN.md 4.15 in float64, per row."""
    if phi == 0.0 or cond_scale in (0, 1):
        return O.unet_forward_with_cond_scale(sd, xin, t, cond, cond_scale)
    b = xin.shape[0]
    ones = torch.ones(b, dtype=torch.bool)
    c = O.unet_forward(sd, xin, t, cond, ~ones, "denoise_fn.").double()
    null = O.unet_forward(sd, xin, t, cond, ones, "denoise_fn.").double()
    g = null + (c - null) * cond_scale
    std_c, std_g = c.reshape(b, -1).std(dim=1, unbiased=True), g.reshape(b, -1).std(dim=1, unbiased=True)
    return (g * (phi * std_c / std_g + (1.0 - phi)).reshape(b, 1, 1, 1, 1)).float()


def joint_loop(kind, sd, fea, conds, total, frames, overlap, steps, timesteps, cond_scale, noise_fn, blend="ramp", phi=0.0, known=None,
               sel=None, clean=False, eta=1.0):
    """The joint sampling loop over the oracle's pieces.  conds: one condition per window.  known / sel (bool of the latent's shape):
    held on the step's level (clean: as they are), one extra draw behind x_T unless clean."""
    starts = design_starts(total, frames, overlap)
    glob = max(total, frames)
    table, _ = design_table(glob, frames, starts, blend)
    b = fea.shape[0]
    shape = (b, 3, glob) + tuple(fea.shape[2:])
    assert len(conds) == len(starts)
    x = noise_fn(shape)
    kn = None
    if known is not None:
        kn = torch.zeros(shape) if clean else noise_fn(shape)
    fea_rep = fea.unsqueeze(2).repeat(1, 1, frames, 1, 1)

    def hold(x, a, s):
        if known is None:
            return x
        a, s = (1.0, 0.0) if clean else (a, s)
        return torch.where(sel, (a * known + s * kn).to(x.dtype), x)

    def predict(x, time):
        """The window outputs folded onto the global time line: float64 sums of the fp32 weights times the fp32 outputs, rounded once."""
        t = torch.full((b,), time, dtype=torch.long)
        outs = [_guided(sd, torch.cat([x[:, :, s0:s0 + frames], fea_rep], dim=1), t, conds[w], cond_scale, phi).double()
                for w, s0 in enumerate(starts)]
        eps = torch.zeros(shape, dtype=torch.float64)
        for f in range(glob):
            for j in range(int(table["count"][f])):
                eps[:, :, f] += float(table["wgt"][f, j]) * outs[int(table["win"][f, j])][:, :, int(table["loc"][f, j])]
        return eps.float(), t

    if kind == "ddim":
        pairs = O.ddim_time_pairs(timesteps, steps)
        a0 = sd["alphas_cumprod_prev"][pairs[0][0]]
        x = hold(x, a0.sqrt(), (1 - a0).sqrt())
        for time, time_next in pairs:
            z = noise_fn(shape) if time_next > 0 else 0.0
            eps, t = predict(x, time)
            alpha, alpha_next = sd["alphas_cumprod_prev"][time], sd["alphas_cumprod_prev"][time_next]
            x0 = O.dynamic_threshold(O.predict_start_from_noise(sd, x, t, eps))
            sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            c = ((1 - alpha_next) - sigma ** 2).sqrt()
            x = hold(x0 * alpha_next.sqrt() + c * eps + sigma * z, alpha_next.sqrt(), (1 - alpha_next).sqrt())
        return x
    if kind == "ddpm":
        a0 = sd["alphas_cumprod"][timesteps - 1]
        x = hold(x, a0.sqrt(), (1 - a0).sqrt())
        for time in reversed(range(timesteps)):
            z = noise_fn(shape)
            eps, t = predict(x, time)
            x0 = O.dynamic_threshold(O.predict_start_from_noise(sd, x, t, eps))
            mean = O._bc(sd["posterior_mean_coef1"][t], b) * x0 + O._bc(sd["posterior_mean_coef2"][t], b) * x
            logvar = O._bc(sd["posterior_log_variance_clipped"][t], b)
            a = sd["alphas_cumprod_prev"][time]
            x = hold(mean + (0.0 if time == 0 else 1.0) * (0.5 * logvar).exp() * z, a.sqrt(), (1 - a).sqrt())
        return x
    lv = ms_levels(timesteps, steps)
    pairs = O.ddim_time_pairs(timesteps, steps)
    x = hold(x.double(), lv[0, 0], lv[0, 1]).float()
    m_prev, h_prev = None, None
    for i, (time, _) in enumerate(pairs):
        last = i == len(pairs) - 1
        (al_s, sg_s), (al_n, sg_n) = lv[i], lv[i + 1]
        eps, t = predict(x, time)
        m = O.dynamic_threshold(O.predict_start_from_noise(sd, x, t, eps)).double()
        k = al_n - sg_n * al_s / sg_s
        h = math.inf if last else math.log(al_n / sg_n) - math.log(al_s / sg_s)
        if i == 0 or last:
            new = (sg_n / sg_s) * x.double() + k * m
        else:
            r = h_prev / h
            new = (sg_n / sg_s) * x.double() + k * (1 + 1 / (2 * r)) * m - k / (2 * r) * m_prev
        x, m_prev, h_prev = hold(new, al_n, sg_n).float(), m, h
    return x


def test_the_loop_is_the_oracles_own():
    """One window: the joint loop equals O.sample bit for bit, DDIM and DDPM (host only, tiny UNet input)."""
    b, t, s = 1, 2, 8
    dsd = {"denoise_fn." + k: v for k, v in synth.unet_state().items()}
    img, cond = synth.inputs(b, 32)
    fea = O.generator_compute_fea(synth.generator_state(), img)
    for kind, steps, total in (("ddim", 3, 1000), ("ddpm", 3, 3)):
        sd = dict(dsd)
        sd.update(O.make_schedule(total))
        for frames_asked in (t, t - 1):
            got = joint_loop(kind, sd, fea, [cond], frames_asked, t, 1, steps, total, 1.0, synth.NoiseTape(11))
            want = O.sample(sd, fea, cond, (b, 3, t, s, s), steps, total, 1.0, 1.0, synth.NoiseTape(11))
            assert torch.equal(got, want), (kind, frames_asked)


# ------------------------------------------------------------------------------------------ whole videos against the loop
def _geometry(dev, which=0):
    """(total_frames, overlap): emulator 7 / 2 on windows of 4 - three windows, frame 3 has three contributors; GPU 13 / 3 (two windows)
    and 20 / 3 (four windows, frame 12 has three contributors) on windows of 8."""
    return (7, 2) if dev == "cpu" else ((13, 3), (20, 3))[which]


_models = {}


def _build(dev, kind, **kw):
    """One model per configuration and device for the whole module (the weights are synth's fixed ones)."""
    z = _sizes(dev)
    total = STEPS if kind == "ddpm" else 1000
    key = (dev, kind, tuple(sorted(kw.items())))
    if key not in _models:
        _models[key] = synth.build_flow_diffusion(dev, img_size=z["s"], num_frames=z["t"], sampling_timesteps=STEPS, timesteps=total,
                                                  sampler="dpmpp_2m" if kind == "dpmpp_2m" else "reference", **kw)
    m, dsd, gsd = _models[key]
    sd = dict(dsd)
    sd.update(O.make_schedule(total))
    return m, sd, gsd, total, z


def _check_video(m, ref, what, tol=1e-3):
    for k in NAMES:
        assert_close(getattr(m, k).cpu(), ref[k], tol, "%s %s" % (k, what))


CASES = [("ddim", 1.0, 0, 0.0), ("ddim", 2.0, 0, 0.0), ("ddpm", 1.0, 0, 0.0), ("ddpm", 2.0, 0, 0.0), ("dpmpp_2m", 1.0, 0, 0.0),
         ("dpmpp_2m", 2.0, 0, 0.0), ("ddim", 2.0, 0, 0.7), ("ddim", 1.0, 1, 0.0), ("dpmpp_2m", 2.0, 1, 0.0)]


@pytest.mark.parametrize("kind,cond_scale,which,phi", CASES)
def test_joint_video_against_the_loop(backend, kind, cond_scale, which, phi):
    dev = backend
    _skip_slow_emu(dev)
    if dev == "cpu" and which:
        pytest.skip("the emulator runs one geometry")
    m, sd, gsd, timesteps, z = _build(dev, kind, **(dict(guidance_rescale=phi) if phi else {}))
    total, overlap = _geometry(dev, which)
    img, cond = synth.inputs(z["b"], z["hw"])
    fea = O.generator_compute_fea(gsd, img)
    windows = len(design_starts(total, z["t"], overlap))
    lat = joint_loop(kind, sd, fea, [cond] * windows, total, z["t"], overlap, STEPS, timesteps, cond_scale, synth.NoiseTape(11), phi=phi)
    ref = _decode(gsd, img, lat, total)
    m.diffusion.noise_source = synth.NoiseTape(11)
    m.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))
    assert m.joint_windows(total, overlap) == design_starts(total, z["t"], overlap)
    m.sample_long_video(cond_scale, total, overlap=overlap, method="joint")
    assert tuple(m.sample_latent.shape) == (z["b"], 3, total, z["s"], z["s"])
    assert_close(m.sample_latent.cpu(), lat, 1e-3, "latent (%s, cond_scale %g, F %d, phi %g)" % (kind, cond_scale, total, phi))
    _check_video(m, ref, "(%s, cond_scale %g, F %d, phi %g)" % (kind, cond_scale, total, phi))


@pytest.mark.parametrize("total_off", [0, -1])
def test_one_window_is_the_chain_and_the_plain_video(backend, total_off):
    dev = backend
    _skip_slow_emu(dev)
    m, _, _, _, z = _build(dev, "ddim")
    total = z["t"] + total_off
    img, cond = synth.inputs(z["b"], z["hw"])
    m.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))
    runs = {}
    for name, call in (("joint", lambda: m.sample_long_video(1.0, total, overlap=2, method="joint")),
                       ("chain", lambda: m.sample_long_video(1.0, total, overlap=2)), ("one", lambda: m.sample_one_video(1.0))):
        m.diffusion.noise_source = synth.NoiseTape(11)
        call()
        runs[name] = {k: getattr(m, k).clone() for k in NAMES + ("sample_latent",)}
    for k in runs["joint"]:
        assert torch.equal(runs["joint"][k], runs["chain"][k]), k
        if total_off == 0:
            assert torch.equal(runs["joint"][k], runs["one"][k]), k


@pytest.mark.parametrize("level,elem", [("noised", False), ("clean", False), ("noised", True)])
def test_known_content_on_the_global_time_line(backend, level, elem):
    """Frames {0, F - 1} and one inside an overlap (or, elem: a box of every frame) come back bit for bit; the rest follows the loop."""
    dev = backend
    _skip_slow_emu(dev)
    m, sd, gsd, timesteps, z = _build(dev, "ddim")
    total, overlap = _geometry(dev)
    starts = design_starts(total, z["t"], overlap)
    img, cond = synth.inputs(z["b"], z["hw"])
    fea = O.generator_compute_fea(gsd, img)
    shape = (z["b"], 3, total, z["s"], z["s"])
    known = synth.NoiseTape(23)(shape).clamp(-1, 1).contiguous()
    if elem:
        mask = torch.zeros((z["b"], 1, total, z["s"], z["s"]), dtype=torch.bool)
        mask[:, :, :, 1:z["s"] // 2, 2:] = True
        sel = mask.expand(shape)
    else:
        mask = torch.zeros(z["b"], total, dtype=torch.bool)
        mask[:, [0, total - 1, starts[1] + 1]] = True          # (starts[1] + 1 < starts[0] + T: inside the first overlap)
        assert starts[1] + 1 < z["t"]
        sel = mask[:, None, :, None, None].expand(shape)
    lat = joint_loop("ddim", sd, fea, [cond] * len(starts), total, z["t"], overlap, STEPS, timesteps, 1.0, synth.NoiseTape(11), known=known,
                     sel=sel, clean=level == "clean")
    ref = _decode(gsd, img, lat, total)
    m.diffusion.noise_source = synth.NoiseTape(11)
    m.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))
    m.sample_long_video(1.0, total, overlap=overlap, method="joint", known_latent=known.to(dev), known_mask=mask.to(dev), known_level=level)
    got = m.sample_latent.cpu()
    assert torch.equal(got[sel], known[sel])
    assert float((got[~sel] - known[~sel]).abs().max()) > 1e-2
    _check_video(m, ref, "(known %s, elem %s)" % (level, elem))


def test_per_window_conditions(backend):
    dev = backend
    _skip_slow_emu(dev)
    m, sd, gsd, timesteps, z = _build(dev, "ddim")
    total, overlap = _geometry(dev)
    windows = len(design_starts(total, z["t"], overlap))
    img, cond = synth.inputs(z["b"], z["hw"])
    other = synth.inputs(z["b"], z["hw"], seed=3)[1]
    assert not torch.equal(cond, other)
    m.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))

    def run(**kw):
        m.diffusion.noise_source = synth.NoiseTape(11)
        m.sample_long_video(1.0, total, overlap=overlap, method="joint", **kw)
        return m.sample_latent.clone()

    plain = run()
    assert torch.equal(run(window_text=[cond.to(dev)] * windows), plain)
    conds = [cond if w % 2 == 0 else other for w in range(windows)]
    two = run(window_text=[c.to(dev) for c in conds])
    assert not torch.equal(two, plain)
    fea = O.generator_compute_fea(gsd, img)
    lat = joint_loop("ddim", sd, fea, conds, total, z["t"], overlap, STEPS, timesteps, 1.0, synth.NoiseTape(11))
    _check_video(m, _decode(gsd, img, lat, total), "(two labels)")


def test_counter_noise_is_the_replayed_tape_and_a_video_is_its_seed(backend):
    dev = backend
    _skip_slow_emu(dev)
    z = _sizes(dev)
    total, overlap = _geometry(dev)
    glob = (3, total, z["s"], z["s"])
    build = lambda noise: synth.build_flow_diffusion(dev, img_size=z["s"], num_frames=z["t"], sampling_timesteps=STEPS, noise=noise)[0]
    img, cond = synth.inputs(1, z["hw"])
    a, b = 41, (1 << 63) + 5

    def run(m, n, **kw):
        m.set_sample_input(sample_img=img.expand(n, -1, -1, -1).contiguous().to(dev), sample_text=cond.expand(n, -1).contiguous().to(dev))
        m.sample_long_video(1.0, total, overlap=overlap, method="joint", **kw)
        return {k: getattr(m, k).clone() for k in NAMES + ("sample_latent",)}

    mc = build("counter")
    alone = run(mc, 1, seed=a)
    assert torch.equal(run(mc, 1, seed=[a])["sample_latent"], alone["sample_latent"])
    mt = build("torch")
    mt.diffusion.noise_source = mc.diffusion.counter_tape([a], (1,) + glob, True)            # window = 0, the global element index
    assert torch.equal(run(mt, 1)["sample_latent"], alone["sample_latent"])
    pair = run(mc, 2, seed=[a, b])
    for k in alone:
        assert_close(pair[k][0:1], alone[k], 2e-3, "%s of seed a, first of two" % k)
    assert float((pair["sample_latent"][0] - pair["sample_latent"][1]).abs().mean()) > 1e-2


# ------------------------------------------------------------------------------------------ plumbing on the GPU
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvpr23_lfdm_amd import _native
    _native._set_library_for_tests(None)


LKW = dict(img_size=8, num_frames=8, sampling_timesteps=7)


def _small(**kw):
    m = synth.build_flow_diffusion("cuda", **dict(LKW, **kw))[0]
    img, cond = synth.inputs(1, 32, seed=5)
    m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
    return m


def _joint(m, total=13, tape=True, **kw):
    m.diffusion.noise_source = synth.NoiseTape(5) if tape else None
    m.sample_long_video(1.0, total, overlap=3, method="joint", **kw)
    return m.sample_latent.clone()


@pytest.mark.gpu
def test_graph_chunks_do_not_change_a_joint_video(monkeypatch):
    _gpu()
    got = {}
    for chunk in ("1", "10"):
        monkeypatch.setenv("LFDM_GRAPH_STEPS", chunk)
        m = _small(sampler="dpmpp_2m")           # (draws nothing after x_T: the tape does not force one step per replay)
        got[chunk] = _joint(m)
        plan = next(p for k, p in m.diffusion._plans.items() if k.joint is not None)
        assert plan["graph"] is not None and bool(plan["chunk_graphs"]) == (chunk == "10")
    assert torch.equal(got["1"], got["10"])
    monkeypatch.setenv("LFDM_GRAPH_STEPS", "10")
    m = _small()
    torch.manual_seed(3)
    first = _joint(m, tape=False)              # torch's generator: the step noise is captured with the steps
    torch.manual_seed(3)
    monkeypatch.setenv("LFDM_GRAPH_STEPS", "1")
    assert torch.equal(first, _joint(_small(), tape=False))


@pytest.mark.gpu
def test_a_joint_video_lives_beside_the_chain_and_the_plain_video(monkeypatch):
    """Chain, plain and joint videos alternate without capturing again; the joint plan's key is (total frames, starts, blend): the same
    geometry captures nothing new, another frame count is another plan.  The encoder runs once per video."""
    _gpu()
    import cvpr23_lfdm_amd.diffusion as D
    m = _small()
    captures = []
    real = D.capture_step
    monkeypatch.setattr(D, "capture_step", lambda unet, plan, mode: (captures.append(mode), real(unet, plan, mode))[1])
    encodes = []
    enc = m.generator.encode
    monkeypatch.setattr(m.generator, "encode", lambda img: (encodes.append(1), enc(img))[1])

    def chain():
        m.diffusion.noise_source = synth.NoiseTape(5)
        m.sample_long_video(1.0, 13, overlap=3)
        return m.sample_latent.clone()

    def plain():
        m.diffusion.noise_source = synth.NoiseTape(5)
        m.sample_one_video(1.0)
        return m.sample_latent.clone()

    c0, p0 = chain(), plain()
    n0 = len(captures)
    del encodes[:]
    j0 = _joint(m)
    assert len(encodes) == 1 and len(captures) == n0 + 1 and captures[-1].joint == D.JointGeometry(13, (0, 5), "ramp")
    assert not torch.equal(j0, c0) and torch.isfinite(j0).all()
    # the first joint video runs the UNet at batch B W: its scratch arenas grow ONCE, and the graphs bound to the old ones are captured
    # again at their next use (`_run_steps`).  From then on nothing is captured, whatever the order.
    assert torch.equal(chain(), c0) and torch.equal(plain(), p0)
    n1 = len(captures)
    for _ in range(2):
        assert torch.equal(_joint(m), j0) and torch.equal(chain(), c0) and torch.equal(plain(), p0) and torch.equal(_joint(m), j0)
    assert len(captures) == n1 and len(m.diffusion._plans) == 3
    _joint(m, total=12)                         # another global frame count: another plan, one more capture - and the old one is dropped
    assert len(captures) == n1 + 1 and sum(k.joint is not None for k in m.diffusion._plans) == 1
    assert torch.equal(chain(), c0) and torch.equal(plain(), p0) and len(captures) == n1 + 1
    _joint(m, blend="uniform", total=12)        # ... and so is another blend
    assert len(captures) == n1 + 2


# ------------------------------------------------------------------------------------------ refusals and drivers (host only)
def test_refusals():
    from cvpr23_lfdm_amd import FlowDiffusion
    m = FlowDiffusion(img_size=8, num_frames=8, sampling_timesteps=7, is_train=False, config_pth=synth.CONFIG)
    m.set_sample_input(sample_img=torch.zeros(1, 3, 32, 32), sample_text=torch.zeros(1, 768))
    known, mask = torch.zeros(1, 3, 13, 8, 8), torch.zeros(1, 13, dtype=torch.bool)
    text = torch.zeros(1, 768)
    with pytest.raises(ValueError, match="method='joint'"):
        m.sample_long_video(1.0, 13, overlap=3, known_latent=known, known_mask=mask)
    with pytest.raises(ValueError, match="method='joint'"):
        m.sample_long_video(1.0, 13, overlap=3, blend="uniform")
    with pytest.raises(ValueError, match="method='joint'"):
        m.sample_long_video(1.0, 13, overlap=3, window_text=[text, text])
    with pytest.raises(ValueError, match="2 windows"):
        m.sample_long_video(1.0, 13, overlap=3, method="joint", window_text=[text, text, text])
    with pytest.raises(ValueError, match="start_latent"):
        m.sample_long_video(1.0, 13, overlap=3, method="joint", start_latent=known, strength=0.5)
    with pytest.raises(ValueError, match="method must be"):
        m.sample_long_video(1.0, 13, overlap=3, method="fused")
    with pytest.raises(ValueError, match="blend"):
        m.sample_long_video(1.0, 13, overlap=3, method="joint", blend="cosine")
    with pytest.raises(ValueError, match="known"):
        m.sample_long_video(1.0, 13, overlap=3, method="joint", known_latent=known[:, :, :8], known_mask=mask)
    assert m.joint_windows(13, 3) == [0, 5] and m.joint_windows(20, 3) == [0, 5, 10, 12] and m.joint_windows(5, 3) == [0]
    d = m.diffusion
    fea = torch.zeros(1, 256, 8, 8)
    with pytest.raises(ValueError, match="start"):
        d.sample(fea, cond=text, total_frames=13, overlap=3, start=known, start_step=2)
    with pytest.raises(ValueError, match="need total_frames"):
        d.sample(fea, cond=text, overlap=3)
    with pytest.raises(ValueError, match="needs overlap"):
        d.sample(fea, cond=text, total_frames=13)
    with pytest.raises(ValueError, match="in place of cond"):
        d.sample(fea, cond=text, total_frames=13, overlap=3, window_cond=[text, text])
    with pytest.raises(ValueError, match="2\\^24"):
        FlowDiffusion(img_size=256, num_frames=40, sampling_timesteps=7, is_train=False, config_pth=synth.CONFIG).joint_windows(1400, 4)


def test_the_joint_mode_keys_the_plan():
    from cvpr23_lfdm_amd.diffusion import JointGeometry, JointMode, SampleMode
    base = SampleMode(1, 8, 8, 2, 2.0, True, 7, 1, "fp32", "reference", "torch", 0.9, False)
    g = JointGeometry(13, (0, 5), "ramp")
    j = JointMode(base, g)
    assert j.joint == g and j.latent_frames == 13 and j.frames == 8 and base.joint is None and base.latent_frames == 8
    assert j != base and base != j and j == JointMode(base, g) and hash(j) == hash(JointMode(base, g))
    assert j != JointMode(base, g._replace(blend="uniform")) and j != JointMode(base, JointGeometry(12, (0, 4), "ramp"))
    assert j.with_rescale(0.7).rescale == 0.7 and j.with_rescale(0.7) != j and j.with_rescale(0.7).joint == g
    assert j != base.with_rescale(0.7) and j._replace(batch=2).joint == g and j._replace(batch=2).batch == 2
    assert JointMode(base._replace(passes=1), g, 0.7).rescale == 0.0 and len({j: 1, base: 2}) == 2
    assert tuple(j) == tuple(base) and "joint=" in repr(j)


def _tool(name):
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", name + ".py")
    spec = importlib.util.spec_from_file_location("lfdm_%s_tool" % name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_flags_parse():
    demo = _tool("demo")
    args = demo.build_parser().parse_args([])
    assert args.long_method == "chain" and args.blend == "ramp" and args.window_labels == ""
    args = demo.build_parser().parse_args(["--total-frames", "112", "--overlap", "4", "--long-method", "joint", "--blend", "uniform",
                                           "--window-labels", "happiness,surprise,anger"])
    assert args.long_method == "joint" and args.blend == "uniform" and demo.window_labels(args, 3) == ["happiness", "surprise", "anger"]
    with pytest.raises(SystemExit):
        demo.window_labels(args, 2)
    with pytest.raises(SystemExit):
        demo.build_parser().parse_args(["--long-method", "fused"])
    ev = _tool("eval")
    args = ev.build_parser().parse_args(["ab"])
    assert args.long_method == "chain" and args.blend == "ramp" and args.total_frames == 0 and args.overlap == 8
    args = ev.build_parser().parse_args(["ab", "--total-frames", "112", "--overlap", "4", "--long-method", "joint", "--blend", "uniform"])
    assert args.long_method == "joint" and args.blend == "uniform" and args.total_frames == 112
    assert ev.parse_overrides("long_method=joint,steps=20") == {"long_method": "joint", "steps": 20}
