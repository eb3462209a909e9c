#!/usr/bin/env python
"""What the demo spends between `sample_*` and the GIF, host path against device path, on ONE sampled synthetic video
per frame count, all on the same machine.  Needs a GPU.

  (a) the render launches alone (flow_to_color_u8 + render_strip), device events after warm-up, median; also as bytes moved / time
  (b) FlowDiffusion.render_sample_host end to end (launches + one pinned copy + one synchronise), host clock, median
  (c) io_compat.video_strip on the same tensors (numpy + matplotlib per frame), host clock
  (d) io_compat.mimsave (RGB frames, PIL quantises) against io_compat.mimsave_indexed (the device's palette indices), host clock
and the demo's wall time per video before (sample + c + mimsave of c's frames) and after (sample + b + mimsave_indexed).

    python tools/bench_render.py [--frames 40 112] [--steps 100] [--reps 50] [--out profiles/render_c2.json]
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402
from cvpr23_lfdm_amd import _build, io_compat as IO, ops  # noqa: E402


def render_bytes(b, t, size, panels, indexed):
    """Bytes the two launches must move, from the shapes: every fp32 operand read once (the source image is re-read per frame from
    cache and counted once), the colour image written and read, the strip written."""
    s = size // 4
    n = 0
    if "flow" in panels:
        n += b * 2 * t * s * s * 4 * 2 + 2 * b * t * s * s * 3          # grid read by both passes; colour written, then read
    n += sum(b * 3 * t * size * size * 4 for p in panels if p in ("out", "warped"))
    if "source" in panels:
        n += b * 3 * size * size * 4
    if "conf" in panels:
        n += b * t * s * s * 4
    return n + b * t * size * len(panels) * size * (1 if indexed else 3)


def host_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def device_ms(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def summary(ts, digits=3):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits), "max": round(max(ts), digits), "n": len(ts)}


def measure(model, ref, frames, a, tmp):
    nf = model.diffusion.num_frames

    def sample():
        if frames > nf:
            model.sample_long_video(1.0, frames, overlap=a.overlap)
        else:
            model.sample_one_video(cond_scale=1.0)

    sample()                                                  # warm-up: plans, graphs
    t_sample = host_ms(sample, 2)
    b, size = ref.shape[0], ref.shape[-1]
    row = {"frames": frames, "batch": b, "size": size, "sample_ms": summary(t_sample, 1)}
    for indexed in (False, True):
        name = "indexed" if indexed else "rgb"
        for _ in range(5):                                    # warm-up: code objects, the pinned buffer
            model.render_sample_host(indexed=indexed)
        dev = device_ms(lambda: model.render_sample(indexed=indexed), a.reps)
        nbytes = render_bytes(b, frames, size, ops.PANELS, indexed)
        row["a_launches_ms_" + name] = summary(dev, 4)
        row["a_bytes_" + name] = nbytes
        row["a_tb_per_s_" + name] = round(nbytes / (statistics.median(dev) * 1e-3) / 1e12, 4)
        row["b_render_sample_host_ms_" + name] = summary(host_ms(lambda: model.render_sample_host(indexed=indexed), a.reps))
    IO.video_strip(model, ref)                                # first call: matplotlib's own start-up
    t_c, host_frames = [], None
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        host_frames = IO.video_strip(model, ref)
        t_c.append((time.perf_counter() - t0) * 1e3)
    row["c_video_strip_ms"] = summary(t_c, 1)
    rgb = [f.copy() for f in IO.video_strip_device(model, ref)]
    idx = [f.copy() for f in IO.video_strip_device(model, ref, indexed=True)]
    writes = {"d_mimsave_host_frames_ms": lambda: IO.mimsave(os.path.join(tmp, "h.gif"), host_frames),
              "d_mimsave_rgb_device_frames_ms": lambda: IO.mimsave(os.path.join(tmp, "r.gif"), rgb),
              "d_mimsave_indexed_ms": lambda: IO.mimsave_indexed(os.path.join(tmp, "i.gif"), idx)}
    for key, fn in writes.items():
        ts = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        row[key] = summary(ts, 1)
    row["gif_bytes"] = {k: os.path.getsize(os.path.join(tmp, k + ".gif")) for k in ("h", "r", "i")}
    med = lambda key: row[key]["median"]
    row["demo_wall_ms_before"] = round(med("sample_ms") + med("c_video_strip_ms") + med("d_mimsave_host_frames_ms"), 1)
    row["demo_wall_ms_after_rgb"] = round(med("sample_ms") + med("b_render_sample_host_ms_rgb") + med("d_mimsave_rgb_device_frames_ms"), 1)
    row["demo_wall_ms_after_indexed"] = round(med("sample_ms") + med("b_render_sample_host_ms_indexed") + med("d_mimsave_indexed_ms"), 1)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, nargs="+", default=[40, 112])
    ap.add_argument("--window", type=int, default=40, help="the model's num_frames")
    ap.add_argument("--overlap", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_render.py needs a GPU: nothing here is estimated")
    torch.cuda.set_device(0)
    with contextlib.redirect_stdout(sys.stderr):
        model = synth.build_flow_diffusion("cuda:0", img_size=a.size // 4, num_frames=a.window, sampling_timesteps=a.steps)[0]
    img, cond = synth.inputs(1, a.size, seed=7)
    ref = img.cuda()
    model.diffusion.noise_source = None
    torch.manual_seed(1234)
    model.set_sample_input(sample_img=ref, sample_text=cond.cuda())
    out = {"what": "render of a sampled synthetic video: host path against device path (tools/bench_render.py)",
           "device": torch.cuda.get_device_name(0), "build": _build.source_fingerprint(), "steps": a.steps, "reps": a.reps,
           "host_reps": a.host_reps, "rows": []}
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(sys.stderr):
        for frames in a.frames:
            out["rows"].append(measure(model, ref, frames, a, tmp))
            print(json.dumps(out["rows"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
