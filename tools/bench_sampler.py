#!/usr/bin/env python
"""lfdm_sampler_step_f32, the DDIM / DDPM update and the multistep one (lfdm_sampler_step_params.multistep), plain, with known frames (8 of
the 40, .known.frame_mask) and with known elements (the same 8 frames as an element mask, and a box of a quarter of every frame;
.known.elem_mask), at the C2 latent (B=1, 3x40x32x32) and two larger shapes: us per step (graph replay), alternating."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvpr23_lfdm_amd import ops  # noqa: E402


def replay_us(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / 100


for b, shape in ((1, (3, 40, 32, 32)), (16, (3, 40, 32, 32)), (4, (3, 40, 64, 64))):
    x, eps, noise, hist = [torch.randn(b, *shape, device="cuda") for _ in range(4)]
    n = x[0].numel()
    table = torch.rand(4, 6, device="cuda")            # every coefficient non-zero: the multistep update reads its history
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = ops.sampler_ws(b, n, "cuda")
    mask = torch.zeros(b, shape[1], dtype=torch.bool, device="cuda")
    mask[:, :8] = True
    kf = dict(known=torch.randn(b, *shape, device="cuda"), known_noise=torch.randn(b, *shape, device="cuda"), frame_mask=mask,
              level=torch.rand(5, 2, device="cuda"), frames=shape[1])
    common = {k: v for k, v in kf.items() if k not in ("frame_mask", "frames")}
    emask = mask[:, None, :, None, None].expand(b, *shape).contiguous()          # the frame mask, one byte per element
    box = torch.zeros(b, *shape, dtype=torch.bool, device="cuda")
    box[..., :shape[2] // 2, :shape[3] // 2] = True                               # a quarter of every frame
    ke, kb = dict(common, elem_mask=emask), dict(common, elem_mask=box)
    fns = {"sampler_step": lambda: ops.sampler_step(x, eps, noise, table, step, ws=ws, advance=False),
           "sampler_step_ms": lambda: ops.sampler_step_ms(x, eps, hist, table, step, ws=ws, advance=False),
           "sampler_step known": lambda: ops.sampler_step(x, eps, noise, table, step, ws=ws, advance=False, **kf),
           "sampler_step_ms known": lambda: ops.sampler_step_ms(x, eps, hist, table, step, ws=ws, advance=False, **kf),
           "sampler_step elem": lambda: ops.sampler_step(x, eps, noise, table, step, ws=ws, advance=False, **ke),
           "sampler_step_ms elem": lambda: ops.sampler_step_ms(x, eps, hist, table, step, ws=ws, advance=False, **ke),
           "sampler_step elem box": lambda: ops.sampler_step(x, eps, noise, table, step, ws=ws, advance=False, **kb),
           "sampler_step_ms elem box": lambda: ops.sampler_step_ms(x, eps, hist, table, step, ws=ws, advance=False, **kb)}
    graphs = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(10):
                fn()
        graphs[name] = g
    torch.cuda.synchronize()
    times = {name: [] for name in graphs}
    for _ in range(5):
        for name, g in graphs.items():
            times[name].append(replay_us(g))
    print("B=%2d n=%7d:\n  %s" % (b, n, "\n  ".join("%s %.1f us per step (min %.1f, max %.1f)" % (k, statistics.median(t), min(t), max(t))
                                                  for k, t in times.items())))
