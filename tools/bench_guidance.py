#!/usr/bin/env python
"""Guidance rescale and trailing step grid, on ONE box, alternating the variants in one process:
    tools/bench_guidance.py [--batches 1 8] [--iters 200] [--rounds 7] [--videos 5] [--skip-videos]
1. the two launches of ops.cfg_combine_rescale at (B, 3, 40, 32, 32) next to ops.cfg_combine alone and next to the same arithmetic in eager
   torch; per variant the host time of --iters back-to-back repetitions ending in a synchronise, median over --rounds, and the bytes/s that
   time means over 4 reads and 1 write of every element (cond and null read by both launches, out written once);
2. whole C2 videos (B = 1, 40 frames, 32x32 latent, synthetic weights) at cond_scale = 2: DDIM-100 with guidance_rescale 0 against 0.7,
   and 20-step dpmpp_2m on the reference grid against the trailing grid (the same launches: the grid is table work).
GPU only."""
import argparse
import os
import statistics
import sys
import time

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
sys.path.insert(0, os.path.join(R, "tools"))

from bench_known_train import FRAMES, LATENT, report, timed  # noqa: E402

SCALE, PHI = 2.0, 0.7


def launches(a):
    from cvpr23_lfdm_amd import ops
    for batch in a.batches:
        shape = (batch, 3, FRAMES, LATENT, LATENT)
        n = shape[1] * shape[2] * shape[3] * shape[4]
        g = torch.Generator(device="cuda").manual_seed(1)
        cond = torch.randn(shape, device="cuda", generator=g)
        null = 0.6 * torch.randn(shape, device="cuda", generator=g) + 0.3
        out = torch.empty_like(cond)
        ws = ops.cfg_rescale_ws(batch, n, "cuda")

        def eager():
            gd = null + (cond - null) * SCALE
            f = PHI * cond.reshape(batch, -1).std(dim=1) / gd.reshape(batch, -1).std(dim=1) + (1.0 - PHI)
            return gd * f.reshape(batch, 1, 1, 1, 1)

        runs = {"cfg_combine (one launch)": lambda: ops.cfg_combine(cond, null, SCALE, out),
                "cfg_combine_rescale (two launches)": lambda: ops.cfg_combine_rescale(cond, null, SCALE, PHI, out, ws=ws),
                "eager torch, the same arithmetic": eager}
        for fn in runs.values():
            timed(fn, 20)
        times = {k: [] for k in runs}
        for _ in range(a.rounds):
            for name, fn in runs.items():
                times[name].append(timed(fn, a.iters) * 1e3)
        for name, tt in times.items():
            med = report("B = %d (%.2f MB per operand): %s" % (batch, batch * n * 4 / 1e6, name), tt, "us")
            if "rescale" in name:
                print("    %.1f GB/s over 4 reads + 1 write of %d elements" % (5 * batch * n * 4 / (med * 1e-6) / 1e9, batch * n), flush=True)


def videos(a):
    import synth
    modes = {"DDIM-100, guidance_rescale 0": dict(sampling_timesteps=100), "DDIM-100, guidance_rescale 0.7": dict(sampling_timesteps=100, guidance_rescale=PHI),
             "dpmpp_2m-20, reference grid": dict(sampling_timesteps=20, sampler="dpmpp_2m"),
             "dpmpp_2m-20, trailing grid": dict(sampling_timesteps=20, sampler="dpmpp_2m", step_grid="trailing")}
    models = {}
    for name, kw in modes.items():
        m, _, _ = synth.build_flow_diffusion("cuda", img_size=LATENT, num_frames=FRAMES, timesteps=1000, **kw)
        img, cond = synth.inputs(1, 4 * LATENT)
        m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
        models[name] = m
    torch.manual_seed(0)
    for m in models.values():                  # warm-up: graph capture, then one replayed video
        for _ in range(2):
            m.sample_one_video(cond_scale=SCALE)
    torch.cuda.synchronize()
    times = {k: [] for k in models}
    for _ in range(a.videos):
        for name, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.sample_one_video(cond_scale=SCALE)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    med = {name: report("C2 video, cond_scale %g: %s" % (SCALE, name), tt) for name, tt in times.items()}
    d = med["DDIM-100, guidance_rescale 0.7"] - med["DDIM-100, guidance_rescale 0"]
    print("guidance_rescale 0.7 - 0: %+.3f ms per video, %+.2f us per step (%.4f of the video)" % (d, d * 10.0, med["DDIM-100, guidance_rescale 0.7"] / med["DDIM-100, guidance_rescale 0"]))
    print("trailing / reference grid, dpmpp_2m-20: %.4f" % (med["dpmpp_2m-20, trailing grid"] / med["dpmpp_2m-20, reference grid"]))
    print("spread of each mode (max - min) / median: %s" % ", ".join("%.4f" % ((max(t) - min(t)) / statistics.median(t)) for t in times.values()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--videos", type=int, default=5)
    ap.add_argument("--skip-videos", action="store_true", help="the launches alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "GPU only"
    launches(a)
    if not a.skip_videos:
        videos(a)


if __name__ == "__main__":
    main()
