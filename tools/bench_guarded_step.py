#!/usr/bin/env python
"""Cost of FlatAdam's guarded step (ema_decay / max_grad_norm / skip_nonfinite) inside the DM training step: two models
on one GPU - options off and all three on - driven through FlowDiffusion.optimize_parameters() on bench.py's training inputs, timed in
alternating rounds (events around the whole step and around optimizer_diff.step() alone).  Needs a GPU.

    python tools/bench_guarded_step.py [--batch 8] [--steps 6] [--rounds 3]     # the A/B, one JSON line
    python tools/bench_guarded_step.py --only on --steps 4                      # a few steps of one flavour (for rocprofv3 --kernel-trace)
"""
import argparse
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402
from cvpr23_lfdm_amd import FlowDiffusion  # noqa: E402

OPTIONS = dict(ema_decay=0.9999, ema_start_step=2, max_grad_norm=1.0, skip_nonfinite=True)


def build(dev, batch, frames, image, **options):
    torch.manual_seed(4321)
    with contextlib.redirect_stdout(sys.stderr):
        m = FlowDiffusion(img_size=image // 4, num_frames=frames, sampling_timesteps=1000, null_cond_prob=0.1, is_train=True, lr=1e-4,
                          config_pth=synth.CONFIG, pretrained_pth="", **options)
    m.unet.load_state_dict(synth.unet_state())
    m.generator.load_state_dict(synth.generator_state())
    m.region_predictor.load_state_dict(synth.region_state())
    m.bg_predictor.load_state_dict(synth.bg_state())
    for net in (m.generator, m.region_predictor, m.bg_predictor):
        net.eval()
        m.set_requires_grad(net, False)
    m.to(dev)
    ref_img, real_vid, cond, _, _ = synth.train_inputs(batch, frames, image, seed=100)
    m.set_train_input(ref_img=ref_img.to(dev), real_vid=real_vid.to(dev), ref_text=cond.to(dev))
    # events around the optimizer step alone
    m._opt_events, inner = [], m.optimizer_diff.step

    def timed_step(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = inner(*a, **k)
        e1.record()
        m._opt_events.append((e0, e1))
        return out

    m.optimizer_diff.step = timed_step
    return m


def run(m, steps):
    """-> (ms per training step, ms per optimizer step), device time between events."""
    m._opt_events.clear()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        m.optimize_parameters()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, sum(a.elapsed_time(b) for a, b in m._opt_events) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--image", type=int, default=128)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=("off", "on"), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_guarded_step.py needs a GPU")
    dev = "cuda:0"
    torch.cuda.set_device(0)
    kinds = [a.only] if a.only else ["off", "on"]
    models = {k: build(dev, a.batch, a.frames, a.image, **(OPTIONS if k == "on" else {})) for k in kinds}
    for m in models.values():
        run(m, a.warmup)
    rows = {k: [] for k in kinds}
    for r in range(1 if a.only else a.rounds):
        for k in kinds:
            rows[k].append(run(models[k], a.steps))
            print("round %d %-3s: %.2f ms / training step, %.3f ms / optimizer step" % ((r + 1, k) + rows[k][-1]), file=sys.stderr, flush=True)
    out = {"batch": a.batch, "frames": a.frames, "image": a.image, "steps": a.steps, "rounds": len(rows[kinds[0]]), "options_on": OPTIONS}
    for k in kinds:
        out["step_ms_" + k] = [round(v[0], 2) for v in rows[k]]
        out["optimizer_ms_" + k] = [round(v[1], 3) for v in rows[k]]
    if len(kinds) == 2:
        mean = lambda xs: sum(xs) / len(xs)
        out["step_ms_delta"] = round(mean(out["step_ms_on"]) - mean(out["step_ms_off"]), 2)
        out["optimizer_ms_delta"] = round(mean(out["optimizer_ms_on"]) - mean(out["optimizer_ms_off"]), 3)
    on = models.get("on")
    if on is not None:
        opt = on.optimizer_diff
        out["grad_norm"], out["applied_steps"], out["skipped_steps"] = opt.last_grad_norm(), opt.applied_steps(), opt.skipped_steps()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
