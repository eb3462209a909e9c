#!/usr/bin/env python
"""Training objectives and min-SNR loss weights at the shipped training shape (40 frames, 128x128, synthetic weights), on
ONE box, alternating:
    tools/bench_objective.py [--batch 8] [--steps 10] [--rounds 5] [--edge-iters 200] [--skip-step]
1. the diffusion edge on its own, (B, 3, 40, 32, 32), per objective: the three launches of csrc/train_diffusion.hip (q_sample, objective
   loss forward with pred_x0 and the per-sample means, objective loss backward; l2, gamma = 5, no mask) next to the same arithmetic in eager
   torch (q_sample, the target, the weighted per-sample mean and its backward, pred_x0); per variant the host time of --edge-iters
   back-to-back repetitions ending in a synchronise, median over --rounds, alternating;
2. the whole training step, B = --batch, for four settings of one model in one process - the default (the reference's step), pred_v,
   pred_v with gamma = 5, and that with known_train (prob 0.5) - alternating windows of --steps steps, median ms per step over --rounds.
GPU only."""
import argparse
import contextlib
import os
import sys

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
sys.path.insert(0, os.path.join(R, "tools"))

from bench_known_train import FRAMES, IMAGE, LATENT, report, timed  # noqa: E402

GAMMA = 5.0


def edge(a):
    from cvpr23_lfdm_amd import GaussianDiffusion, ops
    shape = (a.batch, 3, FRAMES, LATENT, LATENT)
    g = torch.Generator(device="cuda").manual_seed(1)
    x0, noise = torch.randn(shape, device="cuda", generator=g), torch.randn(shape, device="cuda", generator=g)
    out0 = torch.randn(shape, device="cuda", generator=g)
    t = torch.randint(0, 1000, (a.batch,), device="cuda", generator=g)
    one = torch.ones(1, device="cuda")
    runs = {}
    for objective in GaussianDiffusion.OBJECTIVES:
        d = GaussianDiffusion(torch.nn.Identity(), image_size=LATENT, num_frames=FRAMES, timesteps=1000, sampling_timesteps=100, loss_type="l2",
                              objective=objective, min_snr_gamma=GAMMA).cuda()
        tabs = (d.sqrt_alphas_cumprod, d.sqrt_one_minus_alphas_cumprod, d.sqrt_recip_alphas_cumprod, d.sqrt_recipm1_alphas_cumprod)

        def kernels(d=d, tabs=tabs, objective=objective):
            x_noisy = ops.train_qsample(x0, noise, t, tabs[0], tabs[1])
            _, inv, _, _ = ops.objective_loss_fwd(objective, x0, noise, out0, x_noisy, t, *tabs, d.loss_weight, loss_type="l2")
            ops.objective_loss_bwd(objective, x0, noise, out0, t, tabs[0], tabs[1], d.loss_weight, inv, one, loss_type="l2")

        def eager(d=d, objective=objective):
            x_noisy = d.q_sample(x0, t, noise)
            out = out0.detach().requires_grad_(True)
            target = noise if objective == "pred_noise" else x0 if objective == "pred_x0" else d.predict_v(x0, t, noise)
            means = ((target - out) ** 2).reshape(a.batch, -1).mean(1)
            (d.loss_weight[t] * means).mean().backward()
            o = out.detach()
            o if objective == "pred_x0" else d.predict_start_from_noise(x_noisy, t, o) if objective == "pred_noise" \
                else d.predict_start_from_v(x_noisy, t, o)

        runs["%s: three kernels" % objective] = kernels
        runs["%s: eager torch, the same arithmetic" % objective] = eager
    for fn in runs.values():
        timed(fn, 20)
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, fn in runs.items():
            times[name].append(timed(fn, a.edge_iters) * 1e3)
    for name, tt in times.items():
        report("edge B = %d, gamma = %g, %s" % (a.batch, GAMMA, name), tt, "us")


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
    d = m.diffusion

    def configure(objective, gamma, known):
        # (a benchmark's shortcut: the package builds one diffusion per objective)
        d.objective, d.min_snr_gamma, d.known_policy = objective, gamma, known
        d.loss_weight.copy_(d._loss_weight_table())

    modes = {"default (pred_noise, weight 1)": ("pred_noise", None, None), "pred_v": ("pred_v", None, None),
             "pred_v, gamma 5": ("pred_v", GAMMA, None), "pred_v, gamma 5, known_train (prob 0.5)": ("pred_v", GAMMA, policy)}
    for cfg in modes.values():
        configure(*cfg)
        timed(m.optimize_parameters, 3)
    times = {k: [] for k in modes}
    for _ in range(a.rounds):
        for name, cfg in modes.items():
            configure(*cfg)
            times[name].append(timed(m.optimize_parameters, a.steps))
    med = {name: report("training step B = %d: %s" % (a.batch, name), tt) for name, tt in times.items()}
    base = med["default (pred_noise, weight 1)"]
    for name, v in med.items():
        print("training step: %s - default = %+.3f ms per step (%.4f of the default step)" % (name, v - base, v / base))


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
