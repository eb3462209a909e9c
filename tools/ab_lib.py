#!/usr/bin/env python
"""A/B of two builds of liblfdm_hip.so (or of two environments) on ONE box: the headline - ms per video in bench.py's own timed region -
alternating base / new for N rounds, so that box-to-box and run-to-run drift cancels.
    tools/ab_lib.py TAG [--base scratch/liblfdm_hip_r6base.so] [--rounds 3] [--new-env K=V ...] [--base-env K=V ...]
--train-steps N / --lfae-train-steps N: the same legs also time bench.py's DM and LFAE training steps (ms per step, beside the headline).
Every leg is a fresh process under a time limit (--leg-timeout); the first leg that fails ends the run.
base leg: LFDM_HIP_LIB = the base library (+ --base-env); new leg: the in-tree library (+ --new-env).  Writes gpurun_out/TAG/ab.txt."""
import argparse
import json
import os
import subprocess
import sys

R = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("tag")
ap.add_argument("--base", default="scratch/liblfdm_hip_r6base.so")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--new-env", nargs="*", default=[])
ap.add_argument("--base-env", nargs="*", default=[])
ap.add_argument("--train-steps", type=int, default=0)
ap.add_argument("--lfae-train-steps", type=int, default=0)
ap.add_argument("--leg-timeout", type=int, default=420)
a = ap.parse_args()
out_dir = os.path.join(R, "gpurun_out", a.tag)
os.makedirs(out_dir, exist_ok=True)
cmd = [sys.executable, os.path.join(R, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", "3", "--no-cpu-baseline", "--no-roofline",
       "--no-gpu-eager-baseline", "--train-steps", str(a.train_steps), "--lfae-train-steps", str(a.lfae_train_steps), "--blocks", "1"]
if a.train_steps or a.lfae_train_steps:
    cmd.append("--full")      # (bench.py times its training legs only in a full run; the other secondary legs stay switched off above)
KEYS = ["video"] + (["train"] if a.train_steps else []) + (["lfae_train"] if a.lfae_train_steps else [])


def leg(extra):
    env = dict(os.environ)
    env.update(dict(kv.split("=", 1) for kv in extra))
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=R, timeout=a.leg_timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        sys.exit("leg failed (exit status %d): %s" % (r.returncode, r.stderr[-400:]))
    j = json.loads(lines[-1])
    return {"video": j["ms_per_step"], "train": j.get("train", {}).get("ms_per_step"), "lfae_train": j.get("lfae_train", {}).get("ms_per_step")}


base_env = (["LFDM_HIP_LIB=" + os.path.join(R, a.base)] if a.base != "none" else []) + a.base_env
rows, log = [], ["# A/B on one box: ms per video (%d timed videos after 3 warm-up).  base: %s   new: in-tree library %s" %
                 (a.steps, " ".join(base_env), " ".join(a.new_env))]
for i in range(a.rounds):
    b = leg(base_env)
    n = leg(a.new_env)
    rows.append((b, n))
    log.append("round %d: " % (i + 1) + "  |  ".join("%s base %s  new %s" % (k, b[k], n[k]) for k in KEYS))
    print(log[-1], flush=True)
for k in KEYS:
    bs, ns = [b[k] for b, _ in rows], [n[k] for _, n in rows]
    mb, mn, spread = sum(bs) / len(bs), sum(ns) / len(ns), max(bs) - min(bs)
    lo, hi = min(bs) - spread, max(bs) + spread
    log.append("%s mean: base %.2f ms  new %.2f ms  -> %+.2f ms (%+.2f %%); base min %.2f max %.2f spread %.2f -> bar [%.2f, %.2f]; every new round inside: %s"
               % (k, mb, mn, mn - mb, 100 * (mn - mb) / mb, min(bs), max(bs), spread, lo, hi, all(lo <= v <= hi for v in ns)))
    print(log[-1])
open(os.path.join(out_dir, "ab.txt"), "w").write("\n".join(log) + "\n")
