#!/usr/bin/env python
"""Run the frozen LFAE ONCE over a packed frame store and keep its flow latents for `tools/train_dm.py --packed OUT --latents`
(DESIGN.md 4.13).  Needs a GPU.

    python tools/pack_videos.py ROOT OUT --store-size 128
    python tools/pack_latents.py OUT --lfae-ckpt RegionMM.pth --config configs/lfae_128.yaml --size 128 --dtype f32
        # OUT/latents.f32 (or .f16) + OUT/latents.json beside OUT/frames.u8

Every frame's latent is relative to frame 0 of its video, the trainer's reference frame, and is computed from the un-jittered frames.
The store holds the LFAE's raw outputs (grid x, grid y, occlusion): it serves use_residual_flow True and False.  f32 is exact; f16 halves
the store and rounds each value once (at most 2^-12 for |v| < 1, about 0.004 of a latent pixel at 32 x 32).  latents.json carries a
fingerprint of the LFAE's weights and config; the trainer refuses a store computed by another LFAE.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvpr23_lfdm_amd import FlowDiffusion  # noqa: E402
from cvpr23_lfdm_amd.video_store import LATENT_FILES, pack_latents  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", help="a store written by tools/pack_videos.py")
    ap.add_argument("--lfae-ckpt", default="", help="the LFAE checkpoint the DM will train against (empty: the random initialisation, "
                    "as tools/train_dm.py --synthetic)")
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "lfae_128.yaml"))
    ap.add_argument("--size", type=int, default=128, help="the training size (--size of train_dm.py)")
    ap.add_argument("--dtype", choices=tuple(LATENT_FILES), default="f32")
    ap.add_argument("--chunk-frames", type=int, default=64, help="videos of up to this many frames go through one LFAE pass")
    ap.add_argument("--seed", type=int, default=1234, help="with an empty --lfae-ckpt: train_dm.py's --seed, so that both build the same LFAE")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("tools/pack_latents.py needs a GPU: the LFAE pass is liblfdm_hip.so only")
    torch.manual_seed(args.seed)
    model = FlowDiffusion(is_train=False, img_size=args.size // 4, num_frames=2, sampling_timesteps=1, config_pth=args.config,
                          pretrained_pth=args.lfae_ckpt)
    for net in (model.generator, model.region_predictor, model.bg_predictor):
        net.eval()
    model.cuda()
    meta = pack_latents(model, args.out, dtype=args.dtype, image_size=args.size, chunk_frames=args.chunk_frames)
    size = meta["frames"] * 3 * meta["latent_size"] ** 2 * (2 if args.dtype == "f16" else 4)
    print("%d frames, latents of 3 x %d x %d %s: %.1f MB in %s (LFAE %s)" % (meta["frames"], meta["latent_size"], meta["latent_size"],
                                                                          args.dtype, size / 1e6, args.out, meta["fingerprint"][:12]))


if __name__ == "__main__":
    main()
