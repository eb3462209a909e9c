#!/usr/bin/env python
"""Long attention (65 .. 256 tokens per sequence, csrc/attention_long.hip): per-launch times of the forward and the backward at mode 0, as
fractions of the fp32-MFMA peak, next to attention_kernel<64> at L = 64; and end to end, a 128-frame / 112-frame model next to the
40-frame one of the same build.

Method: every case owns several copies of its operands that together exceed the 256 MB of last-level cache and walks them round robin, so
no launch finds its inputs where the previous one left them; warm-up launches first; per-launch device-event times, reported as the median
with min / max.  Nothing here is a pass / fail bar.

    python tools/bench_attn_long.py [--iters 40] [--skip-e2e] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvpr23_lfdm_amd import ops, train_ops  # noqa: E402

PEAK_TFLOPS = 157.3          # fp32 MFMA, MI355X
CACHE_BYTES = 256 << 20


def attention_flop(nseq, seq, sweeps):
    """4 * L^2 * 32 FLOP per (sequence, head) = one K Q^T and one P V; `sweeps` counts the executed work in units of one L x L x 32 product
    (forward with the two-sweep softmax: 3; backward: phase Q 3 + 2 + 1 and phase KV 4 = 10)."""
    return nseq * 8 * 2 * seq * seq * 32 * sweeps


def tables(seq):
    ang = torch.arange(seq, device="cuda").float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2, device="cuda").float() / 32)))[None]
    return dict(bias=torch.randn(8, seq, seq, device="cuda"), rot_cos=ang.cos().contiguous(), rot_sin=ang.sin().contiguous())


def time_launches(make_call, sets, iters, warmup=5):
    """make_call(i) launches on operand set i % sets -> per-launch times in us."""
    for i in range(warmup):
        make_call(i)
    torch.cuda.synchronize()
    times = []
    for i in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        make_call(i)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return times


def summarise(times):
    return dict(median_us=statistics.median(times), min_us=min(times), max_us=max(times))


def bench_kernel(seq, hw, iters):
    rows = seq * hw
    per_set = rows * (768 * 2 + 256 * 2) * 4
    sets = max(2, CACHE_BYTES // per_set + 1)
    qkv = [torch.randn(rows, 768, device="cuda") for _ in range(sets)]
    out = [torch.empty(rows, 256, device="cuda") for _ in range(sets)]
    dout = [torch.randn(rows, 256, device="cuda") for _ in range(sets)]
    dqkv = [torch.empty(rows, 768, device="cuda") for _ in range(sets)]
    kw = tables(seq)
    res = dict(L=seq, hw=hw, operand_sets=sets)
    if seq <= 64:
        fwd = lambda i: ops.attention_cl(qkv[i % sets], 1, seq, hw, 0, out=out[i % sets], **kw)
        bwd = lambda i: train_ops.attention_bwd(qkv[i % sets], dout[i % sets], 1, seq, hw, 0, **kw)
        fsweeps, bsweeps = 2, 5
    else:
        fwd = lambda i: ops.attention_long_cl(qkv[i % sets], 1, seq, hw, 0, out=out[i % sets], **kw)
        bwd = lambda i: train_ops.attention_long_bwd(qkv[i % sets], dout[i % sets], 1, seq, hw, 0, dqkv=dqkv[i % sets], **kw)
        fsweeps, bsweeps = 3, 10
    for name, call, sweeps in (("forward", fwd, fsweeps), ("backward", bwd, bsweeps)):
        s = summarise(time_launches(call, sets, iters))
        s["executed_gflop"] = attention_flop(hw, seq, sweeps) / 1e9
        s["fraction_of_fp32_mfma_peak"] = s["executed_gflop"] / 1e3 / (s["median_us"] * 1e-6) / PEAK_TFLOPS
        res[name] = s
    return res


def bench_model(frames, steps, long_attention, repeats=3):
    """ms per video and per DDIM step of a synthetic-weight model at the 32 x 32 latent, B = 1 (graph replay, after one warm-up video)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    m, _, _ = synth.build_flow_diffusion("cuda", img_size=32, num_frames=frames, sampling_timesteps=steps, long_attention=long_attention)
    img, cond = synth.inputs(1, 128)
    m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
    m.sample_one_video(cond_scale=1.0)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        m.sample_one_video(cond_scale=1.0)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ms)
    return dict(frames=frames, steps=steps, long_attention=long_attention, video_ms_median=med, video_ms_min=min(ms), video_ms_max=max(ms),
                ms_per_step=med / steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_attn_long.py needs a GPU: it measures liblfdm_hip.so")
    result = {"kernels": [], "end_to_end": []}
    for seq, hw in ((64, 1024), (80, 1024), (128, 1024), (256, 1024), (128, 256)):
        r = bench_kernel(seq, hw, args.iters)
        result["kernels"].append(r)
        print("L %3d hw %4d: forward %8.1f us [%8.1f, %8.1f] %5.1f %% of peak   backward %8.1f us [%8.1f, %8.1f] %5.1f %% of peak" % (
            seq, hw, r["forward"]["median_us"], r["forward"]["min_us"], r["forward"]["max_us"], 100 * r["forward"]["fraction_of_fp32_mfma_peak"],
            r["backward"]["median_us"], r["backward"]["min_us"], r["backward"]["max_us"], 100 * r["backward"]["fraction_of_fp32_mfma_peak"]))
    by = {(r["L"], r["hw"]): r for r in result["kernels"]}
    print("forward L = 128: %.1f us next to 4 x attention_kernel<64> at L = 64 = %.1f us (the same K Q^T + P V work per launch)"
          % (by[(128, 1024)]["forward"]["median_us"], 4 * by[(64, 1024)]["forward"]["median_us"]))
    if not args.skip_e2e:
        for frames, steps, la in ((40, 20, False), (128, 20, True), (112, 100, True)):
            r = bench_model(frames, steps, la)
            result["end_to_end"].append(r)
            print("%3d frames, DDIM %3d%s: %8.1f ms per video [%8.1f, %8.1f], %6.2f ms per step" % (
                frames, steps, ", long_attention" if la else "", r["video_ms_median"], r["video_ms_min"], r["video_ms_max"], r["ms_per_step"]))
        e = result["end_to_end"]
        print("128-frame step %.2f ms next to 3.2 x the 40-frame step = %.2f ms" % (e[1]["ms_per_step"], 3.2 * e[0]["ms_per_step"]))
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
