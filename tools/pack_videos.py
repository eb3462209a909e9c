#!/usr/bin/env python
"""Decode a frame-folder data set ONCE into a packed uint8 store for `tools/train_dm.py --packed`.

    python tools/pack_videos.py ROOT OUT --store-size 128        # ROOT/<label>/<video>/*.jpg|png -> OUT/frames.u8 + OUT/index.json
    python tools/pack_videos.py ROOT OUT --layout any            # every folder of frames at any depth (MUG's <subject>/<expression>/<take>,
                                                                 # MHAD's / NATOPS' flat folders), for `tools/train_lfae.py --packed`

--store-size is 1, 2 or 4 times the training size (--size of train_dm.py) and a multiple of 4.  Equal to the training size, the store
holds exactly the bytes the host loader would feed the colour jitter when the sources are already that size; larger sources are
area-averaged and rounded to a byte once, here.  Without jitter that rounding (at most 0.5 / 255) is the only difference from the host
loader on the original files.  With jitter the augmentation runs on the stored bytes, at store resolution, where the host loader jitters
the full-size frames and shrinks afterwards: the jitter is non-linear, so the two are then not comparable bit for bit or within a bound.
A store larger than the training size keeps the jitter at the finer scale and lets the device do the final shrink.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvpr23_lfdm_amd.video_store import PACK_LAYOUTS, pack_frame_folders  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("root")
    ap.add_argument("out")
    ap.add_argument("--store-size", type=int, default=128)
    ap.add_argument("--layout", choices=PACK_LAYOUTS, default=PACK_LAYOUTS[0], help="label/video: ROOT/<label>/<video>/ as the DM loader "
                    "walks; any: every folder with frames at any depth, in the order lfae_train.FramePairs walks")
    args = ap.parse_args(argv)
    index = pack_frame_folders(args.root, args.out, args.store_size, layout=args.layout)
    size = index["frames"] * index["store_size"] ** 2 * 3
    print("%d videos, %d frames at %d x %d: %.1f MB in %s" % (len(index["videos"]), index["frames"], index["store_size"],
                                                              index["store_size"], size / 1e6, args.out))


if __name__ == "__main__":
    main()
