#!/usr/bin/env python
"""Whole C2 videos (configs[1]: B = 1, 40 frames, 32x32 latent, synthetic weights, sample_one_video) per sampler and step count, on ONE
box, alternating:
    tools/bench_samplers.py [--modes reference:100 dpmpp_2m:100 dpmpp_2m:50 dpmpp_2m:25 dpmpp_2m:20] [--videos 7] [--conv-precision fp32]
One model per mode (same weights), graph capture in the warm-up, then --videos rounds over all modes; median / min / max ms per video and the
step time the pair of longest and shortest dpmpp_2m runs implies (video = fixed + steps x step).  GPU only."""
import argparse
import os
import statistics
import sys
import time

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))

FRAMES, LATENT = 40, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", nargs="+", default=["reference:100", "dpmpp_2m:100", "dpmpp_2m:50", "dpmpp_2m:25", "dpmpp_2m:20"])
    ap.add_argument("--videos", type=int, default=7)
    ap.add_argument("--conv-precision", default="fp32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "GPU only"
    import synth
    models = {}
    for mode in a.modes:
        sampler, steps = mode.split(":")
        m, _, _ = synth.build_flow_diffusion("cuda", img_size=LATENT, num_frames=FRAMES, sampling_timesteps=int(steps), timesteps=1000,
                                             conv_precision=a.conv_precision, sampler=sampler)
        img, cond = synth.inputs(1, 4 * LATENT)
        m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
        models[mode] = m
    torch.manual_seed(0)
    for m in models.values():                  # warm-up: graph capture, then one replayed video
        for _ in range(2):
            m.sample_one_video(cond_scale=1.0)
    torch.cuda.synchronize()
    times = {k: [] for k in models}
    for _ in range(a.videos):
        for mode, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.sample_one_video(cond_scale=1.0)
            torch.cuda.synchronize()
            times[mode].append((time.perf_counter() - t0) * 1e3)
    med = {}
    for mode, t in times.items():
        med[mode] = statistics.median(t)
        print("C2 video (B = 1, conv %s) %-14s median %7.2f ms, min %7.2f, max %7.2f over %d (%s)" %
              (a.conv_precision, mode, med[mode], min(t), max(t), len(t), " ".join("%.1f" % v for v in t)), flush=True)
    two = sorted((int(k.split(":")[1]), v) for k, v in med.items() if k.startswith("dpmpp_2m:"))
    if len(two) >= 2:
        (n0, t0), (n1, t1) = two[0], two[-1]
        step = (t1 - t0) / (n1 - n0)
        print("dpmpp_2m: %.3f ms per step between %d and %d steps, %.2f ms outside the steps" % (step, n0, n1, t0 - n0 * step))
    if "reference:100" in med and "dpmpp_2m:100" in med:
        print("dpmpp_2m:100 / reference:100 video time: %.4f" % (med["dpmpp_2m:100"] / med["reference:100"]))


if __name__ == "__main__":
    main()
