#!/usr/bin/env python
"""Discretisation error of the multistep samplers on the SYNTHETIC UNet (random weights: no trained score, no quality claim), C2 shape,
one fixed x_T:  max / mean |latent - fine|  for "dpmpp_1" and "dpmpp_2m" at --steps, fine = "dpmpp_1" at 999 steps - the same ODE, dynamic
thresholding included.  The reference's DDIM row (eta = 0) is listed for information only: once the clamp is active it pairs the thresholded
x0 with the raw eps on shifted levels, which is a different map, so its distance to `fine` does not go to zero.
    tools/sampler_discretisation.py [--steps 10 20 25 50 100] [--seed 11] [--frames 40] [--latent 32]        GPU only."""
import argparse
import os
import sys

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, nargs="+", default=[10, 20, 25, 50, 100])
    ap.add_argument("--fine", type=int, default=999)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--latent", type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "GPU only"
    import synth
    m, _, _ = synth.build_flow_diffusion("cuda", img_size=a.latent, num_frames=a.frames, sampling_timesteps=a.fine, timesteps=1000,
                                         ddim_sampling_eta=0.0)
    img, cond = synth.inputs(1, 4 * a.latent)
    fea = m.generator.compute_fea(img.cuda())
    d = m.diffusion

    def latent(sampler, steps):
        d.sampler, d.sampling_timesteps = sampler, steps         # (tables and plans are keyed on both)
        d.noise_source = synth.NoiseTape(a.seed)                 # the same x_T every time
        return d.sample(fea, cond=cond.cuda(), cond_scale=1.0).double()

    fine = latent("dpmpp_1", a.fine)
    half = latent("dpmpp_1", a.fine // 2)
    print("# C2 shape (B = 1, %d frames, %dx%d latent), synthetic weights, x_T = NoiseTape(%d); fine = dpmpp_1 at %d steps, |fine| max %.3f mean %.3f"
          % (a.frames, a.latent, a.latent, a.seed, a.fine, float(fine.abs().max()), float(fine.abs().mean())))
    e = (half - fine).abs()
    print("# dpmpp_1 at %d steps against fine: max %.3e mean %.3e (how converged `fine` itself is)" % (a.fine // 2, float(e.max()), float(e.mean())))
    print("%6s  %-22s  %-22s  %-22s" % ("steps", "dpmpp_1 max / mean", "dpmpp_2m max / mean", "reference DDIM eta=0 (info)"))
    for n in a.steps:
        cells = []
        for sampler in ("dpmpp_1", "dpmpp_2m", "reference"):
            e = (latent(sampler, n) - fine).abs()
            cells.append("%.3e / %.3e" % (float(e.max()), float(e.mean())))
        print("%6d  %-22s  %-22s  %-22s" % (n, *cells), flush=True)


if __name__ == "__main__":
    main()
