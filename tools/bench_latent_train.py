#!/usr/bin/env python
"""The DM training step from a stored flow latent against the online step, at the shipped training shape (B = 8, 40
frames, 128 x 128, synthetic weights), in ONE process on one box, alternating:
    tools/bench_latent_train.py [--batch 8] [--steps 10] [--rounds 5] [--gather-iters 500] [--skip-step]
1. the gather launch on its own at (B, 3, 40, 32, 32): lfdm_latent_gather_f32 on prepared operands, ops.latent_gather from Python (row
   table checked on the host and uploaded) and the eager index_select + cat that gives the same tensor, for an fp32 and an fp16 store;
   per variant the host time of --gather-iters back-to-back repetitions ending in a synchronise, median over --rounds, alternating;
2. the whole step, batch preparation included - every variant starts from the same collated batch of one packed store (synthetic
   frames, jitter off, uniform sampling; the data set's host work, which DataLoader workers do beside the step, is outside the window):
     online                       DevicePrep -> set_train_input -> optimize_parameters
     online, lazy real decode     the same with lazy_real_decode (LFDM_LAZY_REAL_DECODE=1)
     latent, resident fp32        DeviceLatentPrep -> set_train_latent -> optimize_parameters
     latent, staged fp16          the same, reference frames and latent rows crossing as bytes
   windows of --steps steps ending in a synchronise, median ms per step over --rounds, alternating.  Before timing, one step of the
   latent variant is compared with the online step on the same seeds (loss, pred_x0).
Every comparison is against the online step of this process.  GPU only: nothing here is estimated."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))

FRAMES, LATENT, IMAGE = 40, 32, 128


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def report(name, t, unit="ms"):
    print("%-62s median %9.4f %s, min %9.4f, max %9.4f over %d (%s)" % (name, statistics.median(t), unit, min(t), max(t), len(t),
                                                                       " ".join("%.4f" % v for v in t)), flush=True)
    return statistics.median(t)


def gather(a):
    from cvpr23_lfdm_amd import ops
    lib = ops._lib()
    n = 64 * FRAMES
    g = torch.Generator(device="cuda").manual_seed(1)
    store32 = torch.rand((n, 3, LATENT, LATENT), device="cuda", generator=g)
    rows_host = (torch.arange(a.batch, dtype=torch.int32).view(-1, 1) * 7 * FRAMES + torch.arange(FRAMES, dtype=torch.int32).view(1, -1)) % n
    rows = rows_host.cuda()
    flat = rows.reshape(-1).long()
    ix, iy = ops._identity_table(LATENT, store32.device), ops._identity_table(LATENT, store32.device)
    ident = torch.stack((ix.view(1, -1).expand(LATENT, LATENT), iy.view(-1, 1).expand(LATENT, LATENT))).view(1, 2, 1, LATENT, LATENT)
    out = torch.empty((a.batch, 3, FRAMES, LATENT, LATENT), device="cuda")
    runs = {}
    for tag, store in (("fp32", store32), ("fp16", store32.half())):
        def launch(store=store):
            lib.check(lib.lfdm_latent_gather_f32(ops._p(store), ops.LATENT_DTYPES.index(store.dtype), n, ops._p(rows), ops._p(ix), ops._p(iy),
                                                 ops._p(out), a.batch, FRAMES, LATENT, LATENT, ops._stream(lib)), "lfdm_latent_gather_f32")

        def eager(store=store):
            v = store.index_select(0, flat).float().view(a.batch, FRAMES, 3, LATENT, LATENT).permute(0, 2, 1, 3, 4)
            return torch.cat((v[:, :2] - ident, v[:, 2:3] * 2 - 1), dim=1)

        launch()
        assert torch.equal(out, eager()), "the launch and the eager sequence differ (%s)" % tag
        runs["%s store: the launch alone" % tag] = launch
        runs["%s store: ops.latent_gather (host row table)" % tag] = lambda store=store: ops.latent_gather(store, rows_host, True, out=out)
        runs["%s store: eager index_select + cat" % tag] = eager
    for fn in runs.values():
        timed(fn, 20)
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, fn in runs.items():
            times[name].append(timed(fn, a.gather_iters) * 1e3)
    for name, tt in times.items():
        report("gather (%d, 3, %d, %d, %d), %s" % (a.batch, FRAMES, LATENT, LATENT, name), tt, "us")


def synthetic_store(path, videos):
    """A packed frame store of `videos` videos of FRAMES smooth random frames, written directly (no image files)."""
    from cvpr23_lfdm_amd import video_store
    os.makedirs(path)
    rng = np.random.RandomState(3)
    frames = np.memmap(os.path.join(path, video_store.FRAMES_FILE), dtype=np.uint8, mode="w+", shape=(videos * FRAMES, IMAGE, IMAGE, 3))
    up = lambda x: np.repeat(np.repeat(x, 8, 0), 8, 1)
    entries = []
    for v in range(videos):
        base = up(rng.randint(0, 256, (IMAGE // 8, IMAGE // 8, 3))).astype(np.float32)
        for i in range(FRAMES):
            f = 0.7 * np.roll(base, (2 * i + 1, -i), (0, 1)) + 0.3 * up(rng.randint(0, 256, (IMAGE // 8, IMAGE // 8, 3)))
            frames[v * FRAMES + i] = np.clip(f, 0, 255).astype(np.uint8)
        entries.append({"label": "label%d" % (v % 3), "video": "v%d" % v, "first": v * FRAMES, "count": FRAMES, "valid": [0, 0, IMAGE, IMAGE]})
    frames.flush()
    del frames
    with open(os.path.join(path, video_store.INDEX_FILE), "w") as f:
        json.dump({"version": video_store.STORE_VERSION, "store_size": IMAGE, "frames": videos * FRAMES, "videos": entries}, f)


def step(a, tmp):
    import synth
    from torch.utils.data import default_collate
    from cvpr23_lfdm_amd import FlowDiffusion, video_store
    torch.manual_seed(4321)
    with contextlib.redirect_stdout(sys.stderr):
        m = FlowDiffusion(img_size=LATENT, num_frames=FRAMES, sampling_timesteps=1000, null_cond_prob=0.1, is_train=True, lr=1e-4,
                          config_pth=synth.CONFIG, pretrained_pth="")
    m.unet.load_state_dict(synth.unet_state())
    m.generator.load_state_dict(synth.generator_state())
    m.region_predictor.load_state_dict(synth.region_state())
    m.bg_predictor.load_state_dict(synth.bg_state())
    for net in (m.generator, m.region_predictor, m.bg_predictor):
        net.eval()
        m.set_requires_grad(net, False)
    m.cuda()
    table = {"label%d" % i: torch.randn(768, generator=torch.Generator().manual_seed(i + 1)).cuda() for i in range(3)}
    m.diffusion.text_encoder = lambda texts: torch.stack([table[t] for t in texts])
    stores = {}
    t0 = time.perf_counter()
    for dtype in ("f32", "f16"):
        stores[dtype] = os.path.join(tmp, dtype)
        synthetic_store(stores[dtype], a.batch)
        video_store.pack_latents(m, stores[dtype], dtype=dtype, image_size=IMAGE)
    torch.cuda.synchronize()
    print("writing %d synthetic frames and packing their latents, twice (fp32 and fp16 stores, one LFAE pass per video): %.2f s" % (a.batch * FRAMES, time.perf_counter() - t0))
    kw = dict(image_size=IMAGE, num_frames=FRAMES, sampling="uniform", jitter=False)
    pv = video_store.PackedVideos(stores["f32"], **kw)
    pl32 = video_store.PackedLatents(stores["f32"], resident=True, model=m, **kw)
    pl16 = video_store.PackedLatents(stores["f16"], resident=False, model=m, **kw)
    batches = {id(ds): default_collate([ds[i] for i in range(a.batch)]) for ds in (pv, pl32, pl16)}
    preps = {id(pv): video_store.DevicePrep(pv), id(pl32): video_store.DeviceLatentPrep(pl32), id(pl16): video_store.DeviceLatentPrep(pl16)}

    def online(lazy):
        def run():
            m.lazy_real_decode = lazy
            batch = batches[id(pv)]
            vids = preps[id(pv)](batch)
            m.set_train_input(ref_img=vids[:, :, 0].clone().detach(), real_vid=vids, ref_text=list(batch[3]))
            m.optimize_parameters()
        return run

    def stored(ds):
        def run():
            batch = batches[id(ds)]
            latent, ref = preps[id(ds)](batch)
            m.set_train_latent(ref_img=ref, latent=latent, ref_text=list(batch[5]))
            m.optimize_parameters()
        return run

    # the same step: one step of each on the same seeds, with the learning rate at 0 so that every one starts from the same weights
    group = m.optimizer_diff.param_groups[0]
    lr, group["lr"] = group["lr"], 0.0
    seen = {}
    for name, fn in (("online", online(False)), ("latent, resident fp32", stored(pl32)), ("latent, staged fp16", stored(pl16))):
        torch.manual_seed(7)
        fn()
        seen[name] = (float(m.loss), m.diffusion.pred_x0.clone())
    group["lr"] = lr
    for name in ("latent, resident fp32", "latent, staged fp16"):
        print("one step on the same seeds, %s against online: loss %.9g against %.9g, pred_x0 largest difference %.3g (largest value %.3g)"
              % (name, seen[name][0], seen["online"][0], float((seen[name][1] - seen["online"][1]).abs().max()), float(seen["online"][1].abs().max())))
    modes = {"online": online(False), "online, lazy real decode": online(True), "latent, resident fp32": stored(pl32),
             "latent, staged fp16": stored(pl16)}
    for fn in modes.values():
        timed(fn, 3)
    times = {k: [] for k in modes}
    for _ in range(a.rounds):
        for name, fn in modes.items():
            times[name].append(timed(fn, a.steps))
    med = {name: report("training step B = %d: %s" % (a.batch, name), tt) for name, tt in times.items()}
    for name in list(modes)[1:]:
        print("training step: %s - online = %+.3f ms per step (%.4f of the online step of this process)"
              % (name, med[name] - med["online"], med[name] / med["online"]))
    m.lazy_real_decode = False


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gather-iters", type=int, default=500)
    ap.add_argument("--skip-step", action="store_true", help="the gather alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_latent_train.py needs a GPU: nothing here is estimated")
    gather(a)
    if not a.skip_step:
        with tempfile.TemporaryDirectory() as tmp:
            step(a, tmp)


if __name__ == "__main__":
    main()
