#!/usr/bin/env python
"""What preparing one DM training batch costs: the existing host path against ops.video_prep on the same pixels, at
B = 8, T = 40, training size 128, from a store at 128 (k = 1) and at 256 (k = 2), colour jitter on and off.  Needs a GPU.

  host      the arithmetic of data.FrameFolderVideos.__getitem__ behind the decoder (data.color_jitter, float32, io_compat.resize, - mean,
            transpose, / 255) for the 8 videos of a batch, one process, host clock - what a loader worker does per item, decode excluded
  staged    the batch's bytes from a pinned buffer to the device (device events) and the two launches, each alone (device events
            around `--chain` back-to-back launches, divided)
  resident  the launches alone, gathering from a store already on the device
  bytes/s   the main launch against what it must move: B T S S 3 bytes in, B T H H 3 floats out

    python tools/bench_video_prep.py [--reps 30] [--host-reps 1] [--out profiles/<tag>_video_prep.json]

--pairs: the same for one LFAE stage-1 batch (ops.frame_pairs_prep against the arithmetic of lfae_train.FramePairs.__getitem__ behind the
decoder, jitter ranges of the reference's mug128.yaml), B = 32 and 12 pairs, training size 128, frames of store size 128 and 256, half of
the pairs flipped.  --write-store DIR writes a synthetic store (--store-videos x --store-frames frames at --size) for
`tools/train_lfae.py --packed DIR --bench` and exits; that needs no GPU.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvpr23_lfdm_amd import _build, data, io_compat, ops  # noqa: E402

MEAN = (104.5, 117.25, 123.0)
MEAN_C = (ctypes.c_float * 3)(*MEAN)


def summary(ts, digits=3):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits), "max": round(max(ts), digits), "n": len(ts)}


def device_us(fn, reps, chain):
    """Microseconds per call: device events around `chain` back-to-back calls."""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(chain):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / chain)
    return ts


def launch(store, rows, params, shift, ws, result, size, jitter, launches):
    """lfdm_video_prep_u8 on operands checked once outside the timed window (ops.video_prep's host-side range check of the frame table
    and its workspace allocation are not kernel time; the launches of a jitter case share one workspace, so MAIN alone reads the grey
    levels the STATS run before it left there)."""
    lib = ops._lib()
    lib.check(lib.lfdm_video_prep_u8(ops._p(store), store.shape[0], ops._p(rows), ops._p(params), ops._p(shift), None, MEAN_C, ops._p(result),
                                     rows.shape[0], rows.shape[1], store.shape[1], size, int(jitter), launches, ops._p(ws), ws.numel() * 4,
                                     ops._stream(lib)), "lfdm_video_prep_u8")


def host_batch(videos, size, jitter):
    """FrameFolderVideos.__getitem__ behind the decoder, for every video of the batch."""
    mean = np.asarray(MEAN, np.float32)
    out = []
    for frames in videos:
        frames = list(frames)
        if jitter:
            frames = data.color_jitter(frames)
        frames = [io_compat.resize(np.asarray(f, np.float32), size, interpolation=io_compat.INTER_AREA) - mean for f in frames]
        video = np.stack([np.transpose(f, (2, 0, 1)) for f in frames], axis=1)
        out.append(np.array(video / 255.0, dtype=np.float32))
    return np.stack(out)


def frames_like_video(n, s, seed):
    """Smooth moving colour fields plus sensor-like noise: neither flat nor white noise."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:s, 0:s].astype(np.float32) / s
    out = np.empty((n, s, s, 3), np.uint8)
    for i in range(n):
        ph = 0.05 * i
        f = np.stack([np.sin(6.0 * xs + ph) * np.cos(4.0 * ys), np.sin(5.0 * ys - ph), np.cos(3.0 * (xs + ys) + ph)], -1) * 100 + 128
        out[i] = np.clip(f + rng.randn(s, s, 3) * 4, 0, 255).astype(np.uint8)
    return out


MUG_JITTER = dict(bright=0.1, contrast=0.1, sat=0.1, hue=0.1)


def host_pairs(pairs, flips, size, jitter):
    """FramePairs.__getitem__ behind the decoder, for every pair of the batch."""
    src, drv = [], []
    for frames, flip in zip(pairs, flips):
        frames = list(frames)
        if jitter:
            frames = data.color_jitter(frames, **MUG_JITTER)
        frames = [io_compat.resize(np.asarray(f, np.float32), size, interpolation=io_compat.INTER_AREA) / 255.0 for f in frames]
        if flip:
            frames = [f[:, ::-1] for f in frames]
        s_, d_ = (np.ascontiguousarray(np.transpose(f, (2, 0, 1)), dtype=np.float32) for f in frames)
        src.append(s_)
        drv.append(d_)
    return np.stack(src), np.stack(drv)


def write_store(out_dir, videos, frames, size):
    """A synthetic store in video_store's format: `videos` videos of `frames` frames_like_video frames each."""
    from cvpr23_lfdm_amd import video_store
    os.makedirs(out_dir, exist_ok=True)
    mm = np.memmap(os.path.join(out_dir, video_store.FRAMES_FILE), dtype=np.uint8, mode="w+", shape=(videos * frames, size, size, 3))
    entries = []
    for v in range(videos):
        mm[v * frames:(v + 1) * frames] = frames_like_video(frames, size, seed=100 + v)
        entries.append({"label": "synthetic", "video": "v%03d" % v, "first": v * frames, "count": frames, "valid": [0, 0, size, size]})
    mm.flush()
    with open(os.path.join(out_dir, video_store.INDEX_FILE), "w") as f:
        json.dump({"version": video_store.STORE_VERSION, "store_size": size, "frames": videos * frames, "videos": entries}, f)


def bench_pairs(a):
    h = a.size
    lib = ops._lib()
    out = {"what": "one LFAE stage-1 batch: host FramePairs arithmetic against ops.frame_pairs_prep (tools/bench_video_prep.py --pairs)",
           "device": torch.cuda.get_device_name(0), "build": _build.source_fingerprint(), "image_size": h, "reps": a.reps, "chain": a.chain,
           "host_reps": a.host_reps, "host_threads": 1, "cases": {}}
    for b in (32, 12):
        for k in (1, 2):
            s = h * k
            frames = frames_like_video(2 * b, s, seed=k)
            flips = [i % 2 for i in range(b)]
            resident = torch.from_numpy(frames_like_video(4 * b, s, seed=10 + k)).cuda()
            g = torch.Generator().manual_seed(k)
            rows_resident = torch.randint(0, resident.shape[0], (b, 2), generator=g, dtype=torch.int32).cuda()
            rows_staged = torch.arange(2 * b, dtype=torch.int32).view(b, 2).cuda()
            pinned = torch.from_numpy(frames).pin_memory()
            staged = pinned.cuda()
            params = torch.tensor([[1.05, 0.95, 1.1]] * b, dtype=torch.float32).cuda()
            shift = torch.tensor([17] * b, dtype=torch.int32).cuda()
            flip = torch.tensor(flips, dtype=torch.int32).cuda()
            src, drv = torch.empty(b, 3, h, h, device="cuda"), torch.empty(b, 3, h, h, device="cuda")
            ws = torch.empty(lib.lfdm_video_prep_ws_bytes(b, 2) // 4, dtype=torch.int32, device="cuda")
            h2d = device_us(lambda: staged.copy_(pinned, non_blocking=True), a.reps, 1)
            for jitter in (False, True):
                host = []
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    ref = host_pairs(frames.reshape(b, 2, s, s, 3), flips, h, jitter)
                    host.append((time.perf_counter() - t0) * 1e3)
                case = {"batch": b, "store_size": s, "jitter": jitter, "host_ms_per_batch": summary(host, 1), "h2d_bytes": int(pinned.numel()),
                        "h2d_us": summary(h2d, 1)}
                for name, store, rows in (("staged", staged, rows_staged), ("resident", resident, rows_resident)):
                    def run():
                        lib.check(lib.lfdm_frame_pairs_prep_u8(ops._p(store), store.shape[0], ops._p(rows), ops._p(params), ops._p(shift), None,
                                                               ops._p(flip), ops._p(src), ops._p(drv), b, s, h, int(jitter), ops._p(ws),
                                                               ws.numel() * 4, ops._stream(lib)), "lfdm_frame_pairs_prep_u8")
                    for _ in range(3):
                        run()
                    case[name] = {"launches_us": summary(device_us(run, a.reps, a.chain), 2)}
                if not jitter:          # the staged result is the host's, bit for bit (with jitter the host drew its own factors)
                    got = ops.frame_pairs_prep(staged, rows_staged, None, None, flip, h, False)
                    case["equal_to_host"] = bool(torch.equal(got[0].cpu(), torch.from_numpy(ref[0])) and
                                                 torch.equal(got[1].cpu(), torch.from_numpy(ref[1])))
                out["cases"]["batch%d_store%d_jitter_%s" % (b, s, "on" if jitter else "off")] = case
                print(json.dumps(case), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", action="store_true", help="LFAE stage-1 frame pairs (ops.frame_pairs_prep) instead of DM videos")
    ap.add_argument("--write-store", default="", help="write a synthetic store here and exit (no GPU needed)")
    ap.add_argument("--store-videos", type=int, default=16)
    ap.add_argument("--store-frames", type=int, default=24)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.write_store:
        write_store(a.write_store, a.store_videos, a.store_frames, a.size)
        print("%d videos x %d frames at %d x %d in %s" % (a.store_videos, a.store_frames, a.size, a.size, a.write_store))
        return
    if not torch.cuda.is_available():
        sys.exit("tools/bench_video_prep.py needs a GPU: nothing here is estimated")
    torch.cuda.set_device(0)
    if a.pairs:
        torch.set_num_threads(1)
        out = bench_pairs(a)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
        return
    b, t, h = a.batch, a.frames, a.size
    out = {"what": "one DM training batch: host FrameFolderVideos arithmetic against ops.video_prep (tools/bench_video_prep.py)",
           "device": torch.cuda.get_device_name(0), "build": _build.source_fingerprint(), "batch": b, "frames": t, "image_size": h,
           "reps": a.reps, "chain": a.chain, "host_reps": a.host_reps, "host_threads": 1, "cases": {}}
    torch.set_num_threads(1)
    for k in (1, 2):
        s = h * k
        videos = frames_like_video(b * t, s, seed=k).reshape(b, t, s, s, 3)
        resident = torch.from_numpy(frames_like_video(2 * b * t, s, seed=10 + k)).cuda()      # a store 2 batches long, gathered from all over
        g = torch.Generator().manual_seed(k)
        rows_resident = torch.randint(0, resident.shape[0], (b, t), generator=g, dtype=torch.int32).cuda()
        rows_staged = torch.arange(b * t, dtype=torch.int32).view(b, t).cuda()
        pinned = torch.from_numpy(videos.reshape(b * t, s, s, 3)).pin_memory()
        staged = pinned.cuda()
        params = torch.tensor([[1.1, 0.9, 1.2]] * b, dtype=torch.float32).cuda()
        shift = torch.tensor([7] * b, dtype=torch.int32).cuda()
        result = torch.empty(b, 3, t, h, h, device="cuda")
        ws = torch.empty(ops._lib().lfdm_video_prep_ws_bytes(b, t) // 4, dtype=torch.int32, device="cuda")
        h2d = device_us(lambda: staged.copy_(pinned, non_blocking=True), a.reps, 1)
        must_move = b * t * (s * s * 3 + h * h * 3 * 4)
        for jitter in (False, True):
            host = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                ref = host_batch(videos, h, jitter)
                host.append((time.perf_counter() - t0) * 1e3)
            case = {"store_size": s, "jitter": jitter, "host_ms_per_batch": summary(host, 1), "h2d_bytes": int(pinned.numel()),
                    "h2d_us": summary(h2d, 1), "float32_batch_bytes": int(result.numel() * 4), "main_launch_bytes": must_move}
            for name, store, rows in (("staged", staged, rows_staged), ("resident", resident, rows_resident)):
                run = lambda launches: launch(store, rows, params, shift, ws, result, h, jitter, launches)
                for _ in range(3):
                    run(ops.PREP_STATS | ops.PREP_MAIN)
                main_us = device_us(lambda: run(ops.PREP_MAIN), a.reps, a.chain)
                case[name] = {"main_us": summary(main_us, 2), "both_us": summary(device_us(lambda: run(ops.PREP_STATS | ops.PREP_MAIN), a.reps, a.chain), 2),
                              "main_bytes_per_s": round(must_move / (statistics.median(main_us) * 1e-6), 0)}
                if jitter:
                    case[name]["stats_us"] = summary(device_us(lambda: run(ops.PREP_STATS), a.reps, a.chain), 2)
            if not jitter:              # the staged result is the host's, bit for bit (with jitter the host drew its own factors)
                case["equal_to_host"] = bool(torch.equal(ops.video_prep(staged, rows_staged, None, None, MEAN, h, False).cpu(), torch.from_numpy(ref)))
            else:                       # and the launches timed above, from one shared workspace, are what the op computes
                launch(staged, rows_staged, params, shift, ws, result, h, True, ops.PREP_STATS | ops.PREP_MAIN)
                case["equal_to_op"] = bool(torch.equal(result, ops.video_prep(staged, rows_staged, params, shift, MEAN, h, True)))
            out["cases"]["store%d_jitter_%s" % (s, "on" if jitter else "off")] = case
            print(json.dumps({"store": s, "jitter": jitter, **{k_: case[k_] for k_ in ("host_ms_per_batch", "h2d_us", "staged", "resident")}}),
                  file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
