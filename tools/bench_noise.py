#!/usr/bin/env python
"""What counter-based noise (noise="counter") costs or saves at C2 (B = 1, 40 frames of 32x32 latent, DDIM-100), three
pairs timed ALTERNATING in one process so that clock drift hits both sides alike:

  video   sample_one_video under noise="torch" against noise="counter" (ms per video, host clock around a device synchronise)
  update  one sampler step's four launches on the latent, reading a noise tensor against computing it (a captured graph of many
          calls, device events around its replay); the torch side's per-step cost also includes the normal_() launch that fills
          the tensor, timed next to it
  fill    ops.philox_normal at the latent size against torch's normal_()

Needs a GPU.  Prints a small table; --out also writes it to a file (profiles/noise_bench.txt is this tool's output).

    python tools/bench_noise.py --videos 6 --out profiles/noise_bench.txt
"""
import argparse
import contextlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def graph_of(fn, calls):
    """`calls` back-to-back calls of fn captured as one graph: a replay is the device's time, not the host's launch rate (an eager loop of
    launches this short measures the Python wrapper)."""
    for _ in range(3):              # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    return g


def alternate(pairs, rounds, calls):
    """{name: [ms per call, one per round]}: every candidate's graph replayed once per round, one after the other (device events)."""
    graphs = [(name, graph_of(fn, calls)) for name, fn in pairs]
    out = {name: [] for name, _ in pairs}
    for name, g in graphs:
        g.replay()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, g in graphs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / calls)
    return out


def fmt(name, xs, unit="ms"):
    return "%-44s median %9.4f %s   min %9.4f   max %9.4f   (%d rounds)" % (name, statistics.median(xs), unit, min(xs), max(xs), len(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--latent", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--videos", type=int, default=6, help="timed videos per noise mode (alternating), after one warm-up video each")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200, help="calls per captured graph of the kernel-level pairs")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_noise.py needs a GPU: it times liblfdm_hip.so")
    import synth
    from cvpr23_lfdm_amd import ops
    from cvpr23_lfdm_amd._build import source_fingerprint
    dev = "cuda"
    lines = ["counter-based noise at B = 1, %d frames of %dx%d latent, DDIM-%d  (build %s, %s)"
             % (args.frames, args.latent, args.latent, args.steps, source_fingerprint(), torch.cuda.get_device_name(0))]

    # ---- whole videos
    models = {}
    img, cond = synth.inputs(1, 4 * args.latent)
    for mode in ("torch", "counter"):
        with contextlib.redirect_stdout(sys.stderr):
            m = synth.build_flow_diffusion(dev, img_size=args.latent, num_frames=args.frames, sampling_timesteps=args.steps, noise=mode)[0]
        m.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))
        models[mode] = m
    torch.manual_seed(1237)

    def video(mode, k):
        kw = dict(seeds=[1000 + k]) if mode == "counter" else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        models[mode].sample_one_video(cond_scale=1.0, **kw)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    times = {"torch": [], "counter": []}
    for mode in times:
        video(mode, 0)              # capture + warm-up
    for k in range(args.videos):
        for mode in times:
            times[mode].append(video(mode, k + 1))
    lines.append("")
    lines.append("whole video (ms, host clock around a synchronise; alternating, %d each):" % args.videos)
    for mode in times:
        lines.append("  " + fmt('noise="%s"' % mode, times[mode]))
    lines.append("  per video: counter - torch = %+.3f ms (median), i.e. %+.2f us per step"
                 % (statistics.median(times["counter"]) - statistics.median(times["torch"]),
                    1e3 * (statistics.median(times["counter"]) - statistics.median(times["torch"])) / args.steps))
    del models
    torch.cuda.empty_cache()

    # ---- the sampler step's launches alone
    shape = (1, 3, args.frames, args.latent, args.latent)
    n = shape[1] * shape[2] * shape[3] * shape[4]
    g = torch.Generator(device=dev).manual_seed(5)
    x, eps, noise = (torch.randn(shape, device=dev, generator=g) for _ in range(3))
    coef = torch.tensor([[1.01, 0.1, 0.99, 0.05, 0.0, 0.02]], device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = ops.sampler_ws(1, n, dev)
    seeds, window = ops.seeds_tensor([1234], dev), torch.zeros(1, dtype=torch.int32, device=dev)
    pairs = [("step, noise read (sampler_step)", lambda: ops.sampler_step(x, eps, noise, coef, step, quantile=0.9, advance=False, ws=ws)),
             ("step, noise computed (seeds=)", lambda: ops.sampler_step(x, eps, None, coef, step, quantile=0.9, advance=False, ws=ws,
                                                                        seeds=seeds, window=window)),
             ("normal_() + step, noise read", lambda: (noise.normal_(), ops.sampler_step(x, eps, noise, coef, step, quantile=0.9, advance=False,
                                                                                        ws=ws)))]
    res = alternate(pairs, args.rounds, args.calls)
    lines.append("")
    lines.append("one sampler step on the latent (four launches: pass 0, two select passes, update; us per call, %d calls per graph replay):" % args.calls)
    for name, _ in pairs:
        lines.append("  " + fmt(name, [1e3 * v for v in res[name]], "us"))

    # ---- filling a latent-sized tensor
    out = torch.empty(shape, device=dev)
    pairs = [("torch normal_()", lambda: out.normal_()),
             ("ops.philox_normal", lambda: ops.philox_normal(out, seeds, stream=ops.NOISE_STREAM_STEP, step=3))]
    res = alternate(pairs, args.rounds, args.calls)
    lines.append("")
    lines.append("filling %d floats (us per call, %d calls per graph replay):" % (n, args.calls))
    for name, _ in pairs:
        lines.append("  " + fmt(name, [1e3 * v for v in res[name]], "us"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
