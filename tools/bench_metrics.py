#!/usr/bin/env python
"""What one paired comparison of two videos costs, three ways on the same machine, at the headline shape B = 1, T = 40,
128 x 128 frames, 32 x 32 latents.  Needs a GPU.

  (a) ops.video_metrics ("unit" domain) and ops.flow_metrics: the HIP kernels, device events after warm-up, median
  (b) the same numbers written in eager float64 ATen on the GPU (separable conv2d for the window moments), device events, median
  (c) the host path: copy both operands to the host, then numpy / scipy.ndimage in float64, host clock, median

    python tools/bench_metrics.py [--frames 40] [--size 128] [--reps 50] [--out profiles/metrics_c2.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvpr23_lfdm_amd import _build, ops  # noqa: E402

C1, C2 = 0.01 ** 2, 0.03 ** 2


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


def host_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def summary(ts, digits=4):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits), "max": round(max(ts), digits), "n": len(ts)}


def ssim_map(ma, mb, eaa, ebb, eab):
    va, vb, vab = eaa - ma * ma, ebb - mb * mb, eab - ma * mb
    return ((2 * ma * mb + C1) * (2 * vab + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2))


def aten_video(a, b, add, win):
    """[l1, mse, ssim] per frame in eager float64 ATen, "unit" domain."""
    bsz, c, t, h, w = a.shape
    va = (a.double() + add).float().clamp(0, 1).double()
    vb = (b.double() + add).float().clamp(0, 1).double()
    d = va - vb
    blur = lambda v: F.conv2d(F.conv2d(v, win.view(1, 1, 1, 11)), win.view(1, 1, 11, 1))
    xa = va.permute(0, 2, 1, 3, 4).reshape(-1, 1, h, w)
    xb = vb.permute(0, 2, 1, 3, 4).reshape(-1, 1, h, w)
    s = ssim_map(blur(xa), blur(xb), blur(xa * xa), blur(xb * xb), blur(xa * xb))
    return torch.stack((d.abs().mean(dim=(1, 3, 4)), (d * d).mean(dim=(1, 3, 4)), s.mean(dim=(1, 2, 3)).reshape(bsz, t, c).mean(dim=-1)), dim=-1)


def aten_flow(ga, gb, ca, cb):
    d = ga.double() - gb.double()
    return torch.stack((torch.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2).mean(dim=(2, 3)), (ca.double() - cb.double()).abs().mean(dim=(1, 3, 4))), dim=-1)


def host_video(a, b, add):
    from scipy.ndimage import gaussian_filter
    a, b = a.cpu().numpy(), b.cpu().numpy()          # the copy is part of the path
    va = np.clip((a.astype(np.float64) + add).astype(np.float32), 0, 1).astype(np.float64)
    vb = np.clip((b.astype(np.float64) + add).astype(np.float32), 0, 1).astype(np.float64)
    blur = lambda v: gaussian_filter(v, sigma=(0, 0, 0, 1.5, 1.5), truncate=3.5)[..., 5:-5, 5:-5]
    s = ssim_map(blur(va), blur(vb), blur(va * va), blur(vb * vb), blur(va * vb))
    d = va - vb
    return np.stack((np.abs(d).mean(axis=(1, 3, 4)), (d * d).mean(axis=(1, 3, 4)), s.mean(axis=(1, 3, 4))), axis=-1)


def host_flow(ga, gb, ca, cb):
    ga, gb, ca, cb = (v.cpu().numpy().astype(np.float64) for v in (ga, gb, ca, cb))
    d = ga - gb
    return np.stack((np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2).mean(axis=(2, 3)), np.abs(ca - cb).mean(axis=(1, 3, 4))), axis=-1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_metrics.py needs a GPU: nothing here is estimated")
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(1)
    shape, s = (a.batch, 3, a.frames, a.size, a.size), a.size // 4
    va = (torch.randn(shape, generator=g) * 0.3 + 0.5).cuda()
    vb = (va.cpu() + 0.05 * torch.randn(shape, generator=g)).cuda()
    lat_a = torch.randn(a.batch, 3, a.frames, s, s, generator=g).cuda()
    lat_b = (lat_a.cpu() + 0.1 * torch.randn(lat_a.shape, generator=g)).cuda()
    ca, cb = (lat_a[:, 2:3] + 1) * 0.5, (lat_b[:, 2:3] + 1) * 0.5
    mean = (10.0, -7.5, 3.25)
    add_np = (np.array(mean) / 255.0).reshape(1, 3, 1, 1, 1)
    add = torch.from_numpy(add_np).cuda()
    x = torch.arange(11, dtype=torch.float64) - 5
    win = torch.exp(-(x * x) / (2 * 1.5 ** 2))
    win = (win / win.sum()).cuda()

    table = torch.empty(a.batch, a.frames, 3, dtype=torch.float64, device="cuda")
    ftable = torch.empty(a.batch, a.frames, 2, dtype=torch.float64, device="cuda")
    runs = {"video": (lambda: ops.video_metrics(va, vb, mean=mean, domain="unit", out=table), lambda: aten_video(va, vb, add, win),
                      lambda: host_video(va, vb, add_np)),
            "flow": (lambda: ops.flow_metrics(lat_a[:, :2], lat_b[:, :2], ca, cb, out=ftable), lambda: aten_flow(lat_a[:, :2], lat_b[:, :2], ca, cb),
                     lambda: host_flow(lat_a[:, :2], lat_b[:, :2], ca, cb))}
    out = {"what": "paired metrics of two videos: HIP kernels against eager fp64 ATen against copy + numpy (tools/bench_metrics.py)",
           "device": torch.cuda.get_device_name(0), "build": _build.source_fingerprint(), "shape": list(shape), "latent": s, "reps": a.reps,
           "host_reps": a.host_reps, "operand_bytes": int(va.numel() * 4)}
    for name, (hip, aten, host) in runs.items():
        for _ in range(5):
            hip()
            aten()
        got, ref, cpu = hip().cpu(), aten().cpu(), torch.from_numpy(host())
        out[name] = {"a_hip_ms": summary(device_ms(hip, a.reps)), "b_aten_fp64_ms": summary(device_ms(aten, a.reps)),
                     "c_host_ms": summary(host_ms(host, a.host_reps), 2),
                     "max_abs_diff_hip_vs_aten": float((got - ref).abs().max()), "max_abs_diff_hip_vs_host": float((got - cpu).abs().max())}
        print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
