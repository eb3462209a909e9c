#!/usr/bin/env python
"""What decoding a sample at another frame rate costs, at C2 (B = 1, 40 frames, latent 32 x 32, image 128 x 128), all in
one process on one machine.  Needs a GPU: nothing here is estimated.

  kernel   the maps-form launch of lfdm_latent_resample_f32 for T' = 40, 79, 157, 313 output frames (factors 1, 2, 4, 8), both modes:
           the entry point alone on tables and outputs made beforehand (device events around --burst launches, per launch), the whole
           ops.latent_resample_maps call (host tables, two small uploads, two allocations; host clock), the same result from eager torch
           ops (index_select, lerp / weighted sum, clamp, add, cat) on tables made beforehand, and the bytes the launch loads and stores
  decode   FlowDiffusion.decode_at per output frame at those T', beside the unchanged 40-frame _decode_sample per frame and the LFAE
           encode that decode_at repeats (host clock, each call ends in a synchronise)
  sample   wall time of a DDIM sample plus the 4x decode (sample_one_video(frame_times=...)) against the plain sample, alternating

    python tools/bench_resample.py [--steps 100] [--reps 30] [--out profiles/resample_bench.txt]
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
import synth  # noqa: E402
from cvpr23_lfdm_amd import _build, ops  # noqa: E402
from cvpr23_lfdm_amd.retime import frame_times  # noqa: E402

FACTORS = (1, 2, 4, 8)
TAPS = {"linear": 2, "cubic": 4}


def launch_bytes(latent_shape, idx, frac, mode):
    """Bytes the launch loads and stores, from the shapes and the tables: one tap per channel of a selected frame, 2 (linear) or 4 (cubic)
    of an interpolated one, three map channels and conf written; the tables once per workgroup.  The identity tables are not counted."""
    b, c, _, h, w = latent_shape
    plane = h * w * 4
    taps = sum(1 if a == 0 else TAPS[mode] for a in frac.tolist())
    groups = -(-(h * w // 4) // 256)
    return b * (taps * c * plane + len(idx) * (c + 1) * plane) + b * len(idx) * groups * 8


def unique_bytes(latent_shape, n_out):
    b, c, t, h, w = latent_shape
    return b * (c * t + (c + 1) * n_out) * h * w * 4


def eager(latent, tabs, mode, ident, clamp_from=2):
    """The same maps and conf from torch ops on the GPU (tables uploaded beforehand): index_select, lerp or the four-tap sum, clamp, add, cat."""
    t = latent.shape[2]
    i, a = tabs["idx"], tabs["frac"].view(1, 1, -1, 1, 1)
    x1, x2 = latent.index_select(2, i), latent.index_select(2, (i + 1).clamp(max=t - 1))
    if mode == "linear":
        v = torch.lerp(x1, x2, a)
    else:
        x0, x3 = latent.index_select(2, (i - 1).clamp(min=0)), latent.index_select(2, (i + 2).clamp(max=t - 1))
        w = tabs["weights"]
        v = w[0] * x0 + w[1] * x1 + w[2] * x2 + w[3] * x3
    occ = torch.where(a == 0, v[:, clamp_from:], v[:, clamp_from:].clamp(-1, 1))
    maps = torch.cat((v[:, :2] + ident, occ), dim=1)
    return maps, (occ + 1) * 0.5


def device_us(fn, reps, burst):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / burst)
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


def med(ts):
    return statistics.median(ts)


def spread(ts):
    return "%.3f (min %.3f, max %.3f, n %d)" % (med(ts), min(ts), max(ts), len(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20, help="launches between two device events")
    ap.add_argument("--sample-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_resample.py needs a GPU: nothing here is estimated")
    torch.cuda.set_device(0)
    dev = "cuda:0"
    s, nf = a.size // 4, a.frames
    with contextlib.redirect_stdout(sys.stderr):
        model = synth.build_flow_diffusion(dev, img_size=s, num_frames=nf, sampling_timesteps=a.steps)[0]
    img, cond = synth.inputs(1, a.size, seed=7)
    model.diffusion.noise_source = None
    torch.manual_seed(1234)
    model.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
    lines = ["temporal resampling of a sampled latent (tools/bench_resample.py)",
             "device %s, build %s, B = 1, T = %d, latent %d x %d, image %d x %d, DDIM %d steps, %d reps, bursts of %d launches"
             % (torch.cuda.get_device_name(0), _build.source_fingerprint(), nf, s, s, a.size, a.size, a.steps, a.reps, a.burst), ""]

    def say(line=""):
        lines.append(line)
        print(line, file=sys.stderr, flush=True)

    with contextlib.redirect_stdout(sys.stderr):
        model.sample_one_video(cond_scale=1.0)                # warm-up: plans, graphs; leaves a latent
    latent = model.sample_latent.contiguous()
    lib = ops._lib()
    st, p = ops._stream(lib), ops._p
    ident = model.get_grid(1, 1, s, s, normalize=True).to(dev)
    ix, iy = ops._identity_table(s, latent.device), ops._identity_table(s, latent.device)

    # ------------------------------------------------------------------ kernel
    say("kernel: maps form (residual: identity added), occlusion channel clamped; us per call, median of %d" % a.reps)
    say("%-7s %5s %12s %12s %12s %12s %12s %10s" % ("mode", "T'", "launch us", "op call us", "eager us", "loaded+stored", "unique bytes", "GB/s"))
    for mode in ("linear", "cubic"):
        for k in FACTORS:
            times = frame_times(nf, k)
            idx, frac = ops.resample_tables(times, nf)
            n = len(times)
            tabs = {"idx": torch.from_numpy(idx).to(dev).long(), "frac": torch.from_numpy(frac).to(dev)}
            t64 = torch.from_numpy(frac).double()
            tabs["weights"] = [w.float().to(dev).view(1, 1, -1, 1, 1) for w in
                               (((2 - t64) * t64 - 1) * t64 / 2, ((3 * t64 - 5) * t64 * t64 + 2) / 2, ((4 - 3 * t64) * t64 + 1) * t64 / 2,
                                (t64 - 1) * t64 * t64 / 2)]
            idx_d, frac_d = torch.from_numpy(idx).to(dev), torch.from_numpy(frac).to(dev)
            maps = torch.empty(1, 3, n, s, s, device=dev)
            conf = torch.empty(1, 1, n, s, s, device=dev)

            def launch():
                rc = lib.lfdm_latent_resample_f32(p(latent), p(idx_d), p(frac_d), p(ix), p(iy), p(maps), p(conf), 1, 3, nf, n, s, s,
                                                  ops.RESAMPLE_MODES.index(mode), 2, st)
                assert rc == 0

            op = lambda: ops.latent_resample_maps(latent, times, mode, residual=True, clamp_from=2)
            eg = lambda: eager(latent, tabs, mode, ident)
            for fn in (launch, op, eg):
                for _ in range(5):
                    fn()
            got, want = op(), eg()
            worst = max(float((got[0] - want[0]).abs().max()), float((got[1] - want[1]).abs().max()))
            assert worst <= 1e-5 * max(1.0, float(want[0].abs().max())), (mode, k, worst)          # the two make the same thing
            t_launch = device_us(launch, a.reps, a.burst)
            t_eager = device_us(eg, a.reps, max(1, a.burst // 4))
            t_op = [t * 1e3 for t in host_ms(op, a.reps)]
            nbytes = launch_bytes(latent.shape, idx, frac, mode)
            say("%-7s %5d %12.2f %12.1f %12.1f %12d %12d %10.1f" % (mode, n, med(t_launch), med(t_op), med(t_eager), nbytes,
                                                                   unique_bytes(latent.shape, n), nbytes / (med(t_launch) * 1e-6) / 1e9))
    say("(launch: the entry point alone, back to back; op call: ops.latent_resample_maps from Python with its table uploads and allocations,")
    say(" host clock to a synchronise; eager: six to twelve torch launches.  GB/s = loaded + stored bytes over the launch time.)")
    say()

    # ------------------------------------------------------------------ decode
    pic = model.sample_img.float().contiguous()
    with torch.no_grad():
        skips = model.generator.encode(pic)
    plain = lambda: model._decode_sample(pic, skips, latent)
    with torch.no_grad():
        for _ in range(3):
            plain()
        t_plain = host_ms(plain, a.reps)
        t_enc = host_ms(lambda: model.generator.encode(pic), a.reps)
    say("decode: ms per call, host clock to a synchronise, median (min, max, n)")
    say("  unchanged 40-frame _decode_sample     %s   -> %.4f ms per frame" % (spread(t_plain), med(t_plain) / nf))
    say("  LFAE encode (decode_at repeats it)    %s" % spread(t_enc))
    for mode in ("linear", "cubic"):
        for k in FACTORS:
            times = frame_times(nf, k)
            for _ in range(2):
                model.decode_at(times, mode, latent=latent)
            ts = host_ms(lambda: model.decode_at(times, mode, latent=latent), max(5, a.reps // 3))
            say("  decode_at %-6s T' = %3d (%d pieces)   %s   -> %.4f ms per frame, %.4f without the encode"
                % (mode, len(times), -(-len(times) // nf), spread(ts), med(ts) / len(times), (med(ts) - med(t_enc)) / len(times)))
    say()

    # ------------------------------------------------------------------ sample
    times = frame_times(nf, 4)
    with contextlib.redirect_stdout(sys.stderr):
        model.sample_one_video(cond_scale=1.0, frame_times=times)
        t_a, t_b = [], []
        for _ in range(a.sample_reps):          # alternating
            t_a += host_ms(lambda: model.sample_one_video(cond_scale=1.0), 1)
            t_b += host_ms(lambda: model.sample_one_video(cond_scale=1.0, frame_times=times), 1)
    say("sample: wall ms per video, host clock to a synchronise, alternating, median (min, max, n)")
    say("  sample_one_video (40 frames)                         %s" % spread(t_a))
    say("  sample_one_video(frame_times=frame_times(40, 4))     %s   (157 frames: + %.2f ms, + %.2f %%)"
        % (spread(t_b), med(t_b) - med(t_a), 100.0 * (med(t_b) - med(t_a)) / med(t_a)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(a.out)


if __name__ == "__main__":
    main()
