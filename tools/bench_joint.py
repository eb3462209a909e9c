#!/usr/bin/env python
"""Long videos by chained windows against jointly denoised windows at the C2 shape (B = 1, windows of 40 frames, 32x32
latent, synthetic weights), on ONE box, alternating in one process:
    tools/bench_joint.py [--modes reference:100 dpmpp_2m:20] [--videos 7] [--frames 112] [--overlap 4] [--long-attention] [--out FILE]
Per mode one model runs, in turn, sample_long_video(method="chain") and (method="joint") of --frames frames; with --long-attention a
second model built with long_attention=True samples the whole video as ONE window of --frames frames (exact, but it needs a checkpoint
trained at that length).  Graph capture in the warm-up; median / min / max ms over --videos rounds.  Then the gather and the fold launches
alone at the joint video's shapes, back to back between two events.  Everything printed is also written to --out (default
profiles/joint_bench.txt).  Reads nothing outside the repository.  GPU only."""
import argparse
import os
import statistics
import sys
import time

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))

WINDOW, LATENT = 40, 32


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def launches_us(fn, reps=200, rounds=7):
    """Median over `rounds` of the mean time of `reps` back-to-back launches, in us."""
    out = []
    for _ in range(rounds):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(end) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", nargs="+", default=["reference:100", "dpmpp_2m:20"])
    ap.add_argument("--videos", type=int, default=7)
    ap.add_argument("--frames", type=int, default=112)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--long-attention", action="store_true", help="also: the whole video as one window of a long_attention model")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "joint_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "GPU only"
    import synth
    from cvpr23_lfdm_amd import _build, ops
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("# tools/bench_joint.py: %d frames, windows of %d, overlap %d, B = 1, %dx%d latent, synthetic weights; build %s; %s"
        % (a.frames, WINDOW, a.overlap, LATENT, LATENT, _build.source_fingerprint(), torch.cuda.get_device_name(0)))
    runs, windows = {}, None
    for mode in a.modes:
        sampler, steps = mode.split(":")
        m, _, _ = synth.build_flow_diffusion("cuda", img_size=LATENT, num_frames=WINDOW, sampling_timesteps=int(steps), timesteps=1000,
                                             sampler=sampler)
        img, cond = synth.inputs(1, 4 * LATENT)
        m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
        windows = len(m.joint_windows(a.frames, a.overlap))
        runs[mode + " chain"] = lambda m=m: m.sample_long_video(1.0, a.frames, overlap=a.overlap)
        runs[mode + " joint"] = lambda m=m: m.sample_long_video(1.0, a.frames, overlap=a.overlap, method="joint")
        if a.long_attention:
            ml, _, _ = synth.build_flow_diffusion("cuda", img_size=LATENT, num_frames=a.frames, sampling_timesteps=int(steps), timesteps=1000,
                                                  sampler=sampler, long_attention=True)
            ml.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
            runs[mode + " one window"] = lambda ml=ml: ml.sample_one_video(cond_scale=1.0)
    torch.manual_seed(0)
    for fn in runs.values():                   # warm-up: graph capture, then one replayed video
        for _ in range(2):
            fn()
    for fn in runs.values():                   # (the joint video's larger batch moves the UNet's arenas once: the chain captures again here)
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.videos):
        for name, fn in runs.items():
            times[name].append(timed(fn))
    med = {}
    for name, t in times.items():
        med[name] = statistics.median(t)
        say("%d frames (B = 1) %-26s median %8.2f ms, min %8.2f, max %8.2f over %d (%s)"
            % (a.frames, name, med[name], min(t), max(t), len(t), " ".join("%.1f" % v for v in t)))
    for mode in a.modes:
        steps = int(mode.split(":")[1])
        chain, joint = med[mode + " chain"], med[mode + " joint"]
        say("%s: joint / chain = %.3f (%+.2f ms per video); per step and window: chain %.3f ms, joint %.3f ms (%d windows)"
            % (mode, joint / chain, joint - chain, chain / steps / windows, joint / steps / windows, windows))
        if mode + " one window" in med:
            say("%s: one window of %d frames (long_attention): %.2f ms, %.3f of the chain" % (mode, a.frames, med[mode + " one window"],
                                                                                            med[mode + " one window"] / chain))
    # the two launches alone, at the joint video's shapes
    starts, table = ops.joint_windows(a.frames, WINDOW, a.overlap)
    x = torch.randn(1, 3, a.frames, LATENT, LATENT, device="cuda")
    st, tb = ops.WindowStarts(starts, "cuda"), ops.WindowTable(table, "cuda")
    xw = torch.empty(len(starts), 3, WINDOW, LATENT, LATENT, device="cuda")
    out = torch.empty_like(x)
    lib = ops._lib()
    stream = ops._stream(lib)
    p = ops._p
    import ctypes
    sh, ch = ctypes.c_void_p(st.host.ctypes.data), ctypes.c_void_p(tb.host["count"].ctypes.data)
    gather = lambda: lib.lfdm_window_gather_f32(p(x), p(st.dev), sh, p(xw), 1, len(starts), 3, a.frames, WINDOW, LATENT * LATENT, stream)
    fold = lambda: lib.lfdm_window_fold_f32(p(xw), p(tb.dev["count"]), p(tb.dev["win"]), p(tb.dev["loc"]), p(tb.dev["wgt"]), ch, p(out), 1,
                                            len(starts), 3, a.frames, WINDOW, LATENT * LATENT, stream)
    assert gather() == 0 and fold() == 0
    for name, fn, nbytes in (("window_gather", gather, 2 * xw.numel() * 4), ("window_fold", fold, (xw.numel() + out.numel()) * 4)):
        m_, lo, hi = launches_us(fn)
        say("%s launch alone (entry point, back to back): median %.3f us, min %.3f, max %.3f over 7 x 200; %.2f MB moved, %.1f GB/s"
            % (name, m_, lo, hi, nbytes / 1e6, nbytes / m_ / 1e3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
