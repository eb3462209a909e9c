"""Progressive distillation: tools/distill_dm.py, the "distilled_steps" checkpoint entry and how tools/demo.py and
tools/eval.py follow it; FlatAdam.reset_moments."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import synth
from cvpr23_lfdm_amd import io_compat as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_under_test", os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_distilled_sampling_helper():
    assert C.checkpoint_distilled_steps(None) is None and C.checkpoint_distilled_steps({"diffusion": {}}) is None
    assert C.checkpoint_distilled_steps({"distilled_steps": 8}) == 8
    for bad in (0, -4, 2.0, True, "8"):
        with pytest.raises(ValueError, match="distilled_steps"):
            C.checkpoint_distilled_steps({"distilled_steps": bad})
    plain = {"diffusion": {}}
    assert C.distilled_sampling(plain, 20, "reference", "dpmpp_2m") == (20, "reference", None, None)
    assert C.distilled_sampling(None) == (None, None, None, None)
    ck = {"distilled_steps": 4}
    assert C.distilled_sampling(ck) == (4, "trailing", 0.0, None)
    assert C.distilled_sampling(ck, 4, "trailing", "reference") == (4, "trailing", 0.0, None)
    steps, grid, eta, warning = C.distilled_sampling(ck, 8, None, None, "x.pth")
    assert (steps, grid, eta) == (8, "trailing", 0.0) and "x.pth was distilled to 4 steps" in warning and "--steps 8" in warning
    with pytest.raises(ValueError, match="--step-grid reference contradicts x.pth"):
        C.distilled_sampling(ck, None, "reference", None, "x.pth")
    with pytest.raises(ValueError, match="--sampler dpmpp_2m contradicts"):
        C.distilled_sampling(ck, None, None, "dpmpp_2m")


def _checkpoint(tmp_path, **entries):
    from cvpr23_lfdm_amd import FlowDiffusion
    m = FlowDiffusion(is_train=False, img_size=8, num_frames=2, sampling_timesteps=5, config_pth=synth.CONFIG, objective="pred_v",
                      step_grid="trailing")
    m.unet.load_state_dict(synth.unet_state())
    path = str(tmp_path / "distilled.pth")
    torch.save(dict({"example": 1, "diffusion": m.diffusion.state_dict(), "objective": "pred_v", "schedule": "cosine"}, **entries), path)
    return path


def test_demo_and_eval_follow_the_checkpoint(backend, tmp_path, capsys):
    """The model tools/demo.py and tools/eval.py build for a checkpoint with "distilled_steps" - and for one without (nothing is sampled)."""
    demo = _tool("demo")
    common = ["--size", "32", "--frames", "2", "--config", synth.CONFIG]
    path = _checkpoint(tmp_path, distilled_steps=4)
    d = demo.make_model(demo.build_parser().parse_args(["--dm-ckpt", path] + common)).diffusion
    assert (d.sampling_timesteps, d.step_grid, d.ddim_sampling_eta, d.sampler, d.is_ddim_sampling) == (4, "trailing", 0.0, "reference", True)
    assert d.ddim_times() == [(999, 749), (749, 499), (499, 249), (249, -1)]
    assert "warning" not in capsys.readouterr().out
    d = demo.make_model(demo.build_parser().parse_args(["--dm-ckpt", path, "--steps", "8", "--step-grid", "trailing"] + common)).diffusion
    assert (d.sampling_timesteps, d.step_grid, d.ddim_sampling_eta) == (8, "trailing", 0.0)
    assert "was distilled to 4 steps" in capsys.readouterr().out
    for flags in (["--step-grid", "reference"], ["--sampler", "dpmpp_2m"]):
        with pytest.raises(SystemExit, match="contradicts"):
            demo.make_model(demo.build_parser().parse_args(["--dm-ckpt", path] + flags + common))
    # tools/eval.py: the same through its build_model, an --a / --b override counts as asked for
    ev = _tool("eval")
    args = ev.build_parser().parse_args(["dm", "--dm-ckpt", path] + common)
    assert (args.steps, args.sampler, args.step_grid) == (100, "reference", "reference") and not getattr(args, "explicit", None)
    model, cfg = ev.build_model(args)
    assert (model.diffusion.sampling_timesteps, model.diffusion.step_grid, cfg["steps"], cfg["sampler"]) == (4, "trailing", 4, "reference")
    with pytest.raises(SystemExit, match="contradicts"):
        ev.build_model(args, {"sampler": "dpmpp_2m"})
    model, cfg = ev.build_model(args, {"steps": 2})
    assert model.diffusion.sampling_timesteps == 2 and cfg["steps"] == 2 and "was distilled to 4 steps" in capsys.readouterr().out
    # a checkpoint without the entry: the flags and the defaults as before
    plain = _checkpoint(tmp_path)
    d = demo.make_model(demo.build_parser().parse_args(["--dm-ckpt", plain] + common)).diffusion
    assert (d.sampling_timesteps, d.step_grid, d.ddim_sampling_eta, d.sampler) == (100, "reference", 1.0, "reference")
    d = demo.make_model(demo.build_parser().parse_args(["--dm-ckpt", plain, "--steps", "20", "--sampler", "dpmpp_2m", "--step-grid", "trailing"] + common)).diffusion
    assert (d.sampling_timesteps, d.step_grid, d.sampler) == (20, "trailing", "dpmpp_2m")


def test_distill_dm_options():
    mod = _tool("distill_dm")
    a = mod.parse_args([])
    assert (a.start_steps, a.end_steps, a.objective, a.distill_weight, a.teacher_cond_scale) == (64, 4, "pred_v", "truncated_snr", 1.0)
    assert mod.round_steps(64, 4) == [64, 32, 16, 8, 4] and mod.round_steps(4, 4) == [4] and mod.round_steps(2, 1) == [2, 1]
    for start, end in ((48, 4), (4, 8), (4, 0), (6, 4)):
        with pytest.raises(SystemExit, match="power of two"):
            mod.round_steps(start, end)
    a = mod.parse_args(["--packed", "DIR", "--latents", "--resident", "--ema-decay", "0.99", "--distill-weight", "none", "--teacher-cond-scale", "2"])
    assert a.latents and a.resident and a.ema_decay == 0.99 and a.distill_weight == "none" and a.teacher_cond_scale == 2.0


def test_distill_dm_stops_on_an_empty_loader(backend, monkeypatch, tmp_path):
    """Fewer videos than --batch-size (incomplete batches are dropped): a message, not a loop that never makes a step."""
    from cvpr23_lfdm_amd import data
    mod = _tool("distill_dm")
    monkeypatch.setattr(mod.T, "make_dataset", lambda args, model=None: (data.SyntheticVideos(n=1, image_size=args.size, num_frames=args.frames), None))
    with pytest.raises(SystemExit, match="gives no batch of --batch-size 2"):
        mod.main(["--synthetic", "--size", "16", "--frames", "2", "--batch-size", "2", "--dim-mults", "1", "2", "--start-steps", "2",
                  "--end-steps", "1", "--iters-per-round", "1", "--num-workers", "0", "--out", str(tmp_path / "out")])


def test_reset_moments(backend):
    """Adam starts again: the next step is the first step of a fresh optimizer on the same weights; the average restarts from them."""
    from cvpr23_lfdm_amd.optim import FlatAdam
    dev = backend
    for kw in (dict(), dict(ema_decay=0.5, skip_nonfinite=True)):
        torch.manual_seed(3)
        a = [torch.nn.Parameter(torch.randn(5, 4, device=dev)), torch.nn.Parameter(torch.randn(7, device=dev))]
        opt = FlatAdam(a, lr=1e-2, **kw)
        grads = [[torch.randn_like(p) for p in a] for _ in range(3)]
        for g in grads[:2]:
            for p, gi in zip(a, g):
                p.grad = gi.clone()
            opt.step()
        assert opt.applied_steps() == 2
        opt.reset_moments()
        assert opt.applied_steps() == 0 and all(float(opt.state[p]["exp_avg"].abs().max()) == 0.0 for p in a)
        if "ema_decay" in kw:
            assert all(torch.equal(opt.state[p]["ema"], p.detach()) for p in a)
        b = [torch.nn.Parameter(p.detach().clone()) for p in a]
        fresh = FlatAdam(b, lr=1e-2, **kw)
        for params, o in ((a, opt), (b, fresh)):
            for p, gi in zip(params, grads[2]):
                p.grad = gi.clone()
            o.step()
        assert all(torch.equal(p, q) for p, q in zip(a, b)) and opt.applied_steps() == 1


def test_distill_dm_synthetic_rounds(backend, monkeypatch, tmp_path, capsys):
    """tools/distill_dm.py --synthetic: two rounds (2 -> 1 steps) of one iteration each; a checkpoint per round with its "distilled_steps".
    The emulator runs a two-level denoiser from a latent store at 16 pixels (--packed --latents); the GPU runs the shipped
    denoiser and the real LFAE at 128 pixels, and tools/demo.py's model then samples the last checkpoint at its recorded step count."""
    from cvpr23_lfdm_amd import FlowDiffusion, video_store
    from test_latent_store import MULTS, _stand_in_pass, _write_videos
    dev = backend
    mod = _tool("distill_dm")
    out = str(tmp_path / "out")
    size, extra = 128, []
    if dev != "cuda":           # a latent store at 16 pixels, packed as test_train_dm_from_a_latent_store packs it (--seed's random-init LFAE)
        size, src, packed = 16, str(tmp_path / "src"), str(tmp_path / "packed")
        _write_videos(src, 16)
        video_store.pack_frame_folders(src, packed, 16)
        torch.manual_seed(1234)
        np.random.seed(1234)
        packer = FlowDiffusion(is_train=False, img_size=4, num_frames=2, sampling_timesteps=1, config_pth=synth.CONFIG, dim_mults=MULTS)
        with monkeypatch.context() as mp:
            mp.setattr(FlowDiffusion, "_lfae_pass", _stand_in_pass)
            video_store.pack_latents(packer, packed, image_size=16)
        extra = ["--dim-mults", "1", "2", "--packed", packed, "--latents"]
    mod.main(["--synthetic", "--size", str(size), "--frames", "2", "--batch-size", "1", "--start-steps", "2", "--end-steps", "1",
              "--iters-per-round", "1", "--num-workers", "0", "--print-freq", "1", "--ema-decay", "0.9", "--skip-nonfinite", "--out", out] + extra)
    log = capsys.readouterr().out
    assert "round 4 -> 2 steps  iter 1/1" in log and "round 2 -> 1 steps  iter 1/1" in log, log
    assert sorted(os.listdir(out)) == ["distilled_0001_N001.pth", "distilled_0001_N002.pth"]
    for n in (1, 2):
        ck = torch.load(os.path.join(out, "distilled_0001_N%03d.pth" % n), map_location="cpu")
        assert ck["distilled_steps"] == n and ck["objective"] == "pred_v" and ck["schedule"] == "cosine" and "diffusion_ema" in ck
        assert C.distilled_sampling(ck)[:3] == (n, "trailing", 0.0)
    assert not any(k.startswith("teacher") for k in ck["diffusion"])
    if dev != "cuda":
        return
    demo = _tool("demo")
    args = demo.build_parser().parse_args(["--dm-ckpt", os.path.join(out, "distilled_0001_N002.pth"), "--size", "128", "--frames", "2", "--config", synth.CONFIG])
    model = demo.make_model(args).cuda().eval()
    assert model.diffusion.sampling_timesteps == 2 and model.diffusion.step_grid == "trailing" and model.diffusion.ddim_sampling_eta == 0.0
    ref_img, _, cond, _, _ = synth.train_inputs(1, 2, 128)
    model.set_sample_input(sample_img=ref_img.cuda(), sample_text=cond.cuda())
    model.sample_one_video(cond_scale=1.0)
    assert tuple(model.sample_latent.shape) == (1, 3, 2, 32, 32) and bool(torch.isfinite(model.sample_latent).all())
