"""FlowDiffusion with the optimizer's averaged weights: the constructor options reach FlatAdam, `ema_weights()` swaps the
denoiser onto the average (packed weights and sampling graphs rebuild, the optimizer refuses to step) and restores it, and
`ema_state_dict()` is a diffusion.state_dict() a second model samples the same video from."""
import os

import pytest
import torch

import synth
from util import assert_close

BIAS = "init_conv.bias"


def _train_model(dev, img_size, frames, **kw):
    from cvpr23_lfdm_amd import FlowDiffusion
    m = FlowDiffusion(img_size=img_size, num_frames=frames, sampling_timesteps=5, null_cond_prob=0.0, is_train=True, lr=5e-3,
                      config_pth=synth.CONFIG, pretrained_pth="", **kw)
    m.unet.load_state_dict(synth.unet_state())
    m.generator.load_state_dict(synth.generator_state())
    m.region_predictor.load_state_dict(synth.region_state())
    m.bg_predictor.load_state_dict(synth.bg_state())
    for net in (m.generator, m.region_predictor, m.bg_predictor):
        net.eval()
        m.set_requires_grad(net, False)
    return m.to(dev)


def _synthetic_step(m, seed):
    """An optimizer step on synthetic gradients (the full training step needs the GPU: ~3 TFLOP)."""
    gen = torch.Generator().manual_seed(seed)
    m.optimizer_diff.zero_grad()
    for p in m.diffusion.parameters():
        p.grad = (torch.randn(p.shape, generator=gen) * 1e-2).to(p.device)
    m.optimizer_diff.step()


def test_flow_diffusion_ema_weights(backend):
    """Case 8, the cheap half.  Two training steps with all three options on - real optimize_parameters() steps on the GPU, optimizer steps
    on synthetic gradients under the emulator - then the context, the state dict and the restore."""
    dev = backend
    s, t = (32, 4) if dev == "cuda" else (8, 4)
    m = _train_model(dev, s, t, ema_decay=0.5, max_grad_norm=1.0, skip_nonfinite=True)
    opt = m.optimizer_diff
    assert opt.guarded and opt.ema_decay == 0.5 and opt.max_grad_norm == 1.0 and opt.skip_nonfinite
    bias = m.unet.get(BIAS)
    hist = [bias.detach().clone()]
    for step in range(2):
        if dev == "cuda":
            ref_img, real_vid, cond, _, _ = synth.train_inputs(2, t, 4 * s)
            torch.manual_seed(5 + step)
            m.set_train_input(ref_img=ref_img.to(dev), real_vid=real_vid.to(dev), ref_text=cond.to(dev))
            m.optimize_parameters()
            assert torch.isfinite(m.loss)
        else:
            _synthetic_step(m, step)
        hist.append(bias.detach().clone())
    assert opt.applied_steps() == 2 and opt.skipped_steps() == 0 and opt.last_grad_norm() > 0.0
    assert len(m.diffusion.state_dict()) == 324                        # the average is optimizer state, not a module buffer
    assert float(m.optimizer_diff.state_dict()["state"][0]["step"]) == 2.0
    raw_b = bias.detach().clone()
    ema_b = opt.state[bias]["ema"].detach().clone()
    assert_close(ema_b, 0.25 * hist[0] + 0.25 * hist[1] + 0.5 * hist[2], 1e-6, "average of init_conv.bias (decay 0.5, two steps)")
    assert float((ema_b - raw_b).abs().max()) > 1e-4
    flats = opt.ensure_flat()

    pk1 = m.unet.packed()
    assert torch.equal(pk1["init.b"], raw_b)
    with m.ema_weights():
        pk2 = m.unet.packed()
        assert pk2 is not pk1 and torch.equal(pk2["init.b"], ema_b)  # rebuilt on the averaged weights
        assert torch.equal(m.unet.get(BIAS).detach(), ema_b)
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
        with pytest.raises(RuntimeError, match="re-entrant"):
            with m.ema_weights():
                pass
    pk3 = m.unet.packed()
    assert pk3 is not pk2 and torch.equal(pk3["init.b"], raw_b)       # ... and on the raw ones again
    assert torch.equal(m.unet.get(BIAS).detach(), raw_b)
    with pytest.raises(KeyError):                                      # the restore also happens on an exception
        with m.ema_weights():
            raise KeyError("boom")
    assert torch.equal(m.unet.get(BIAS).detach(), raw_b) and torch.equal(m.unet.packed()["init.b"], raw_b)

    esd = m.ema_state_dict()
    dsd = m.diffusion.state_dict()
    assert list(esd) == list(dsd) and len(esd) == 324
    assert torch.equal(esd["denoise_fn." + BIAS], ema_b) and torch.equal(esd["betas"], dsd["betas"])
    assert esd["denoise_fn." + BIAS].data_ptr() != opt.state[bias]["ema"].data_ptr()          # copies, not views
    assert torch.equal(dsd["denoise_fn." + BIAS], raw_b)
    _synthetic_step(m, 7)                                               # the optimizer goes on, on the same flat buffers
    assert opt.ensure_flat() is flats and opt.applied_steps() == 3
    assert not torch.equal(bias.detach(), raw_b)


def test_ema_options_need_a_training_model():
    from cvpr23_lfdm_amd import FlowDiffusion
    with pytest.raises(ValueError, match="is_train"):
        FlowDiffusion(img_size=8, num_frames=4, sampling_timesteps=5, is_train=False, config_pth=synth.CONFIG, ema_decay=0.9)
    m = FlowDiffusion(img_size=8, num_frames=4, sampling_timesteps=5, is_train=True, config_pth=synth.CONFIG)
    with pytest.raises(RuntimeError, match="no average"):
        with m.ema_weights():
            pass


@pytest.mark.parametrize("sampler,conv_precision", [("reference", "fp32"), ("dpmpp_2m", "bf16")])
def test_sampling_from_ema_weights(backend, sampler, conv_precision):
    """Case 8, the sampling half: a video sampled inside ema_weights() equals (to the sampling tests' 1e-3) the video a second model loaded
    from ema_state_dict() samples from the same noise, and differs from the raw-weights video."""
    dev = backend
    if dev == "cpu" and os.environ.get("LFDM_EMU_E2E", "0") != "1":
        pytest.skip("end-to-end under the emulator is opt-in (LFDM_EMU_E2E=1); it runs on the GPU")
    z = dict(t=2, s=8, hw=32) if dev == "cpu" else dict(t=4, s=16, hw=64)
    m = _train_model(dev, z["s"], z["t"], ema_decay=0.5, max_grad_norm=1.0, skip_nonfinite=True, sampler=sampler,
                     conv_precision=conv_precision)
    for step in range(2):
        _synthetic_step(m, step)
    img, cond = synth.inputs(1, z["hw"])
    keys = ("sample_latent", "sample_vid_grid", "sample_vid_conf", "sample_warped_vid", "sample_out_vid")

    def sample(model):
        model.diffusion.noise_source = synth.NoiseTape(11)
        model.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))
        model.sample_one_video(cond_scale=1.0)
        return {k: getattr(model, k).detach().cpu().clone() for k in keys}

    raw = sample(m)
    with m.ema_weights():
        avg = sample(m)
    raw_again = sample(m)
    m2, _, _ = synth.build_flow_diffusion(dev, img_size=z["s"], num_frames=z["t"], sampling_timesteps=5, sampler=sampler,
                                          conv_precision=conv_precision)
    m2.diffusion.load_state_dict(m.ema_state_dict())
    want = sample(m2)
    for k in keys:
        assert_close(avg[k], want[k], 1e-3, "ema video: " + k)
        assert_close(raw_again[k], raw[k], 1e-3, "raw video after the context: " + k)
    gap = float((avg["sample_latent"] - raw["sample_latent"]).abs().max())
    err = float((avg["sample_latent"] - want["sample_latent"]).abs().max())
    print("ema vs raw latent: max abs difference %.3e (ema vs reloaded model: %.3e)" % (gap, err))
    assert gap > 1e-3 * max(1.0, float(raw["sample_latent"].abs().max())), gap      # beyond the equality bar: really other weights


def test_demo_use_ema_picks_the_averaged_entry():
    """tools/demo.py --use-ema: the checkpoint's "diffusion_ema" entry, and a clear error for a checkpoint trained without --ema-decay."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("lfdm_demo_tool", os.path.join(synth.REPO_ROOT, "tools", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    ck = {"example": 8, "diffusion": {"raw": 1}, "diffusion_ema": {"avg": 1}}
    assert demo.dm_state(ck, False) is ck["diffusion"] and demo.dm_state(ck, True) is ck["diffusion_ema"]
    with pytest.raises(SystemExit, match="diffusion_ema"):
        demo.dm_state({"example": 8, "diffusion": {}}, True, "old.pth")
    assert demo.build_parser().parse_args(["--use-ema"]).use_ema
