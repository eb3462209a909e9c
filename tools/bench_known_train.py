#!/usr/bin/env python
"""Random-mask training at the shipped training shape (40 frames, 128x128, synthetic weights), on ONE box, alternating:
    tools/bench_known_train.py [--batch 8] [--steps 10] [--rounds 5] [--edge-iters 200] [--skip-step]
1. the diffusion edge on its own, (B, 3, 40, 32, 32): the three launches of csrc/train_diffusion.hip (q_sample with a frame mask, masked loss
   forward with pred_x0, masked loss backward) next to the eager torch sequence they replace (q_sample, mse_loss + its backward,
   predict_start_from_noise - unmasked: the parent's step) and next to the same masked arithmetic written in eager torch; per variant the
   host time of --edge-iters back-to-back repetitions ending in a synchronise, median over --rounds, alternating;
2. the whole training step, B = --batch: the policy off and on (prob 0.5, the default kinds) in one process, alternating windows of
   --steps steps, median ms per step over --rounds.
GPU only."""
import argparse
import contextlib
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))

FRAMES, LATENT, IMAGE = 40, 32, 128


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def report(name, t, unit="ms"):
    print("%-58s median %9.4f %s, min %9.4f, max %9.4f over %d (%s)" % (name, statistics.median(t), unit, min(t), max(t), len(t),
                                                                       " ".join("%.4f" % v for v in t)), flush=True)
    return statistics.median(t)


def edge(a):
    from cvpr23_lfdm_amd import GaussianDiffusion, ops
    d = GaussianDiffusion(torch.nn.Identity(), image_size=LATENT, num_frames=FRAMES, timesteps=1000, sampling_timesteps=100, loss_type="l2").cuda()
    shape = (a.batch, 3, FRAMES, LATENT, LATENT)
    g = torch.Generator(device="cuda").manual_seed(1)
    x0, noise = torch.randn(shape, device="cuda", generator=g), torch.randn(shape, device="cuda", generator=g)
    pred0 = torch.randn(shape, device="cuda", generator=g)
    t = torch.randint(0, 1000, (a.batch,), device="cuda", generator=g)
    mask = torch.zeros(a.batch, FRAMES, dtype=torch.bool, device="cuda")
    mask[::2, :8] = True
    full = mask[:, None, :, None, None].expand(shape)
    one = torch.ones((), device="cuda")
    tabs = (d.sqrt_recip_alphas_cumprod, d.sqrt_recipm1_alphas_cumprod)

    def kernels():
        x_noisy = ops.train_qsample(x0, noise, t, d.sqrt_alphas_cumprod, d.sqrt_one_minus_alphas_cumprod, frame_mask=mask)
        _, inv, _ = ops.masked_loss_fwd(noise, pred0, x_noisy, t, *tabs, loss_type="l2", frame_mask=mask)
        ops.masked_loss_bwd(noise, pred0, inv, one.reshape(1), loss_type="l2", frame_mask=mask)

    def eager_unmasked():
        x_noisy = d.q_sample(x0, t, noise)
        pred = pred0.detach().requires_grad_(True)
        F.mse_loss(noise, pred).backward()
        d.predict_start_from_noise(x_noisy, t, pred.detach())

    def eager_masked():
        x_noisy = torch.where(full, x0, d.q_sample(x0, t, noise))
        pred = pred0.detach().requires_grad_(True)
        unknown = ~full
        count = unknown.reshape(a.batch, -1).sum(1).clamp(min=1)
        ((((noise - pred) ** 2) * unknown).reshape(a.batch, -1).sum(1) / count).mean().backward()
        torch.where(full, x_noisy, d.predict_start_from_noise(x_noisy, t, pred.detach()))

    runs = {"three kernels (frame mask)": kernels, "eager torch, unmasked (the parent's edge)": eager_unmasked,
            "eager torch, the same masked arithmetic": eager_masked}
    for fn in runs.values():
        timed(fn, 20)
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, fn in runs.items():
            times[name].append(timed(fn, a.edge_iters) * 1e3)
    for name, tt in times.items():
        report("edge B = %d: %s" % (a.batch, name), tt, "us")


def step(a):
    import synth
    from cvpr23_lfdm_amd import FlowDiffusion
    from cvpr23_lfdm_amd.diffusion import KnownMaskPolicy
    torch.manual_seed(4321)
    with contextlib.redirect_stdout(sys.stderr):
        m = FlowDiffusion(img_size=LATENT, num_frames=FRAMES, sampling_timesteps=1000, null_cond_prob=0.1, is_train=True, lr=1e-4,
                          config_pth=synth.CONFIG, pretrained_pth="")
    m.unet.load_state_dict(synth.unet_state())
    m.generator.load_state_dict(synth.generator_state())
    m.region_predictor.load_state_dict(synth.region_state())
    m.bg_predictor.load_state_dict(synth.bg_state())
    for net in (m.generator, m.region_predictor, m.bg_predictor):
        net.eval()
        m.set_requires_grad(net, False)
    m.cuda()
    ref_img, real_vid, cond, _, _ = synth.train_inputs(a.batch, FRAMES, IMAGE, seed=100)
    m.set_train_input(ref_img=ref_img.cuda(), real_vid=real_vid.cuda(), ref_text=cond.cuda())
    policy = KnownMaskPolicy(FRAMES, prob=0.5, max_frames=8, seed=0)
    modes = {"policy off": None, "policy on (prob 0.5)": policy}
    for p in modes.values():
        m.diffusion.known_policy = p
        timed(m.optimize_parameters, 3)
    times = {k: [] for k in modes}
    for _ in range(a.rounds):
        for name, p in modes.items():
            m.diffusion.known_policy = p
            times[name].append(timed(m.optimize_parameters, a.steps))
    med = {name: report("training step B = %d: %s" % (a.batch, name), tt) for name, tt in times.items()}
    print("training step: on - off = %+.3f ms per step (%.4f of the step with the policy off)"
          % (med["policy on (prob 0.5)"] - med["policy off"], med["policy on (prob 0.5)"] / med["policy off"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--edge-iters", type=int, default=200)
    ap.add_argument("--skip-step", action="store_true", help="the edge alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "GPU only"
    edge(a)
    if not a.skip_step:
        step(a)


if __name__ == "__main__":
    main()
