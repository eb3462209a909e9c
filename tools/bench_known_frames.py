#!/usr/bin/env python
"""Known-frame conditioning and long videos at the C2 shape (B = 1, 40 frames, 32x32 latent, synthetic weights), on ONE box, alternating:
    tools/bench_known_frames.py [--modes reference:100 dpmpp_2m:20] [--videos 7] [--known 8] [--long-frames 112] [--overlap 4] [--elements]
Per mode one model runs, in turn, an unconditioned video, a video with the first --known frames known, and (unless --long-frames 0) one long
video; with --elements also a video with a box (the upper left quarter of every frame) known through an element mask and one started from a
latent at --strength; graph capture of both plans in the warm-up; median / min / max ms over --videos rounds.  --plain-only times the unconditioned video
alone (the call every tree has: for process-level alternation with another tree).  GPU only."""
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", nargs="+", default=["reference:100", "dpmpp_2m:20"])
    ap.add_argument("--videos", type=int, default=7)
    ap.add_argument("--known", type=int, default=8)
    ap.add_argument("--long-frames", type=int, default=112)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--elements", action="store_true", help="also: a known box through an element mask, and a start from a latent")
    ap.add_argument("--strength", type=float, default=0.5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "GPU only"
    import synth
    runs = {}
    for mode in a.modes:
        sampler, steps = mode.split(":")
        m, _, _ = synth.build_flow_diffusion("cuda", img_size=LATENT, num_frames=FRAMES, sampling_timesteps=int(steps), timesteps=1000,
                                             sampler=sampler)
        img, cond = synth.inputs(1, 4 * LATENT)
        m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
        runs[mode + " plain"] = lambda m=m: m.sample_one_video(cond_scale=1.0)
        if a.plain_only:
            continue
        known = torch.rand(1, 3, FRAMES, LATENT, LATENT, device="cuda") * 2 - 1
        mask = torch.zeros(1, FRAMES, dtype=torch.bool, device="cuda")
        mask[:, :a.known] = True
        runs[mode + " %d known" % a.known] = lambda m=m, k=known, mk=mask: m.sample_one_video(cond_scale=1.0, known_latent=k, known_mask=mk)
        if a.elements:
            box = torch.zeros(1, 1, FRAMES, LATENT, LATENT, dtype=torch.bool, device="cuda")
            box[..., :LATENT // 2, :LATENT // 2] = True
            runs[mode + " box known"] = lambda m=m, k=known, mk=box: m.sample_one_video(cond_scale=1.0, known_latent=k, known_mask=mk)
            runs[mode + " start %.2f" % a.strength] = lambda m=m, k=known: m.sample_one_video(cond_scale=1.0, start_latent=k, strength=a.strength)
        if a.long_frames > 0:
            runs[mode + " long %d" % a.long_frames] = lambda m=m: m.sample_long_video(1.0, a.long_frames, overlap=a.overlap)
    torch.manual_seed(0)
    for fn in runs.values():                   # warm-up: graph capture, then one replayed video
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.videos):
        for name, fn in runs.items():
            times[name].append(timed(fn))
    med = {}
    for name, t in times.items():
        med[name] = statistics.median(t)
        print("C2 video (B = 1) %-26s median %8.2f ms, min %8.2f, max %8.2f over %d (%s)" %
              (name, med[name], min(t), max(t), len(t), " ".join("%.1f" % v for v in t)), flush=True)
    for mode in a.modes:
        plain, steps = med[mode + " plain"], int(mode.split(":")[1])
        cond = med.get(mode + " %d known" % a.known)
        if cond is not None:
            print("%s: conditioned - plain = %+.3f ms per video, %+.2f us per step" % (mode, cond - plain, (cond - plain) * 1e3 / steps))
        for name in ("box known", "start %.2f" % a.strength):
            if mode + " " + name in med:
                t = med[mode + " " + name]
                print("%s: %s - plain = %+.3f ms per video (%.3f of the plain video)" % (mode, name, t - plain, t / plain))
        long = med.get(mode + " long %d" % a.long_frames)
        if long is not None:
            chunks = 1 + max(0, -(-(a.long_frames - FRAMES) // (FRAMES - a.overlap)))
            print("%s: %d frames in %d chunks: %.2f ms, %.1f new frames per second; %d plain videos: %.2f ms (difference %+.2f ms)"
                  % (mode, a.long_frames, chunks, long, a.long_frames / long * 1e3, chunks, chunks * plain, long - chunks * plain))


if __name__ == "__main__":
    main()
