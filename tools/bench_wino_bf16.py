#!/usr/bin/env python
"""fp32 against bf16 operands on the Winograd F(2x2,3x3) schedule (lfdm_conv2d_cl_f32 / lfdm_conv2d_cl_wino_bf16), on ONE box, alternating.
    tools/bench_wino_bf16.py [--rounds 5] [--iters 50] [--videos 5] [--no-shapes] [--no-videos] [--vlds]
Per shape: every Winograd launch shape of a C2 sampler step (B = 1, 40 frames, 32x32 latent), set up as Unet3D._conv sets it up (tile counters,
slab buffer: the in-launch reduction / balanced launch), each mode timed over --iters back-to-back launches per round, the two modes alternating
for --rounds rounds; median and spread of the per-launch times.  Videos: whole C2 videos (DDIM-100, B = 1, sample_one_video) of two models with
the same weights, one per mode, alternating.  --vlds (a library built with --knobs, e.g. through LFDM_HIP_LIB): per shape, the two layouts of V
in LDS of the bf16 kernel (bf16 / fp32 with the conversion at the A-fragment load, LFDM_WINO_BF16_VF32) instead of fp32 against bf16.  GPU only."""
import argparse
import os
import statistics
import sys
import time

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
from cvpr23_lfdm_amd import ops  # noqa: E402

FRAMES, LATENT = 40, 32
# (name, c0, c1, cout, size, groups, gn, launches per step) - the 3x3 convolutions of one B = 1 step on the Winograd schedule
SHAPES = [      # 38 launches: downs / mid / ups ResnetBlocks (block1 of an up level's first block reads cat(x, skip)), the merged output heads
    ("64->64 @32", 64, 0, 64, 32, 1, True, 7), ("64+64->64 @32", 64, 64, 64, 32, 1, True, 1),
    ("64->128 @16", 64, 0, 128, 16, 1, True, 1), ("128->128 @16", 128, 0, 128, 16, 1, True, 3), ("64->64 @16", 64, 0, 64, 16, 1, True, 3),
    ("128+128->64 @16", 128, 128, 64, 16, 1, True, 1),
    ("128->256 @8", 128, 0, 256, 8, 1, True, 1), ("256->256 @8", 256, 0, 256, 8, 1, True, 3), ("128->128 @8", 128, 0, 128, 8, 1, True, 3),
    ("256+256->128 @8", 256, 256, 128, 8, 1, True, 1),
    ("256->512 @4", 256, 0, 512, 4, 1, True, 1), ("512->512 @4", 512, 0, 512, 4, 1, True, 7), ("256->256 @4", 256, 0, 256, 4, 1, True, 3),
    ("512+512->256 @4", 512, 512, 256, 4, 1, True, 1),
    ("heads 64+64->128 @32", 64, 64, 128, 32, 1, True, 1), ("heads grouped 2x64 @32", 128, 0, 128, 32, 2, True, 1),
]


def make_launch(name, c0, c1, cout, s, groups, gn):
    dev = "cuda"
    n = FRAMES
    x0 = torch.randn(n * s * s, c0, device=dev)
    x1 = torch.randn(n * s * s, c1, device=dev) if c1 else None
    cin = c0 + c1
    bias = torch.randn(cout, device=dev)
    if groups > 1:
        ws = [torch.randn(cout // groups, cin // groups, 3, 3, device=dev) * (cin // groups * 9) ** -0.5 for _ in range(groups)]
        ww, wwb, wd = ops.pack_wino_weight_grouped(ws), ops.pack_wino_weight_grouped_bf16(ws), None
    else:
        w = torch.randn(cout, cin, 3, 3, device=dev) * (cin * 9) ** -0.5
        ww, wwb, wd = ops.pack_wino_weight(w), ops.pack_wino_weight_bf16(w), ops.pack_conv_weight(w)
    counters = torch.zeros(8192, dtype=torch.int32, device=dev)
    p, out = ops.conv_params(x0, ww if wd is None else wd, cout, 3, 3, n, s, s, src1=x1, bias=bias, weight_wino=ww, groups=groups,
                             tile_counters=counters)
    assert ops.conv_schedule(p) == 2, name
    if gn:
        p.gn_partial = 1
    tile_rows, ksplit = ops.conv_plan(p)
    need = ops.conv_partial_floats(p)
    part = torch.empty(max(need, 1), device=dev)
    p.partial = part.data_ptr() if need else None
    gnp = torch.empty(2 * 16 * (n * s * s // tile_rows) * 4, device=dev)
    p.gn_partial = gnp.data_ptr() if gn else None
    p.gn_groups, p.gn_pixels = (16 if groups > 1 else 8), n * s * s
    keep = (x0, x1, bias, ww, wwb, wd, counters, part, gnp, out)
    return p, wwb, keep, (tile_rows, ksplit, ops.conv_plan_slabs(p))


def time_launches(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def bench_shapes(a):
    modes = (("vf32", lambda p, wb: (os.environ.__setitem__("LFDM_WINO_BF16_VF32", "1"), ops.conv_launch_wino_bf16(p, wb))),
             ("vb16", lambda p, wb: (os.environ.__setitem__("LFDM_WINO_BF16_VF32", "0"), ops.conv_launch_wino_bf16(p, wb)))) if a.vlds else \
            (("fp32", lambda p, wb: ops.conv_launch(p)), ("bf16", lambda p, wb: ops.conv_launch_wino_bf16(p, wb)))
    print("%-24s %-14s %10s %10s %10s %10s %7s %6s" % ("shape", "plan", modes[0][0] + " us", "spread", modes[1][0] + " us", "spread", "ratio", "/step"))
    tot = [0.0, 0.0]
    for name, c0, c1, cout, s, groups, gn, count in SHAPES:
        p, wwb, keep, plan = make_launch(name, c0, c1, cout, s, groups, gn)
        for _, fn in modes:                  # warm-up (and the first launch of each instantiation)
            for _ in range(3):
                fn(p, wwb)
        torch.cuda.synchronize()
        times = ([], [])
        for _ in range(a.rounds):
            for i, (_, fn) in enumerate(modes):
                times[i].append(time_launches(lambda: fn(p, wwb), a.iters))
        med = [statistics.median(t) for t in times]
        spread = [max(t) - min(t) for t in times]
        tot[0] += count * med[0]
        tot[1] += count * med[1]
        print("%-24s %-14s %10.2f %10.2f %10.2f %10.2f %7.3f %6d" % (name, "rows%d k%d s%d" % plan, med[0], spread[0], med[1], spread[1],
                                                                  med[1] / med[0], count), flush=True)
        del keep
    print("%-24s %-14s %10.1f %10s %10.1f %10s %7.3f" % ("per step (x count)", "", tot[0], "", tot[1], "", tot[1] / tot[0]), flush=True)


def bench_videos(a):
    import synth
    kw = dict(img_size=LATENT, num_frames=FRAMES, sampling_timesteps=100, timesteps=1000)
    models = {}
    for prec in ("fp32", "bf16"):
        m, _, _ = synth.build_flow_diffusion("cuda", conv_precision=prec, **kw)
        img, cond = synth.inputs(1, 4 * LATENT)
        m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
        models[prec] = m
    for prec, m in models.items():            # warm-up: graph capture
        m.sample_one_video(cond_scale=1.0)
    torch.cuda.synchronize()
    times = {k: [] for k in models}
    for _ in range(a.videos):
        for prec, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.sample_one_video(cond_scale=1.0)
            torch.cuda.synchronize()
            times[prec].append((time.perf_counter() - t0) * 1e3)
    for prec, t in times.items():
        print("C2 video (DDIM-100, B = 1, sample_one_video) %s: median %.2f ms, min %.2f, max %.2f over %d (%s)" %
              (prec, statistics.median(t), min(t), max(t), len(t), " ".join("%.1f" % v for v in t)), flush=True)
    print("bf16 / fp32 video time: %.4f" % (statistics.median(times["bf16"]) / statistics.median(times["fp32"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--videos", type=int, default=5)
    ap.add_argument("--no-shapes", action="store_true")
    ap.add_argument("--no-videos", action="store_true")
    ap.add_argument("--vlds", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "GPU only"
    torch.manual_seed(0)
    if not a.no_shapes:
        bench_shapes(a)
    if not a.no_videos and not a.vlds:
        bench_videos(a)


if __name__ == "__main__":
    main()
