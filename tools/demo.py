#!/usr/bin/env python
"""The reference's demo flow (demo/demo_mug.py:60-146, demo_mhad.py, demo_natops.py) on this framework: load LFAE + DM
checkpoints, read one reference image, sample a 40-frame video per text prompt and write the five-panel GIF
[source | generated | warped source | flow grid | occlusion].  Needs a GPU (liblfdm_hip.so; there is no CPU path).
--render device renders that strip on the GPU (FlowDiffusion.render_sample; its fourth panel is the colour-coded flow of
misc.flow2fig, not grid2fig's drawing) and --gif indexed writes its palette indices without PIL's per-frame quantisation.

    python tools/demo.py --config configs/lfae_128.yaml --lfae-ckpt RegionMM.pth --dm-ckpt flowdiff.pth \
        --bert /data/bert-base-cased --image face.jpg --text happiness anger --out demo_out
    python tools/demo.py --synthetic --total-frames 112 --overlap 4 --out demo_out      # a long video: three chained 40-frame windows
    python tools/demo.py --synthetic --render device --gif indexed --out demo_out       # strip and palette indices made on the GPU
    python tools/demo.py --synthetic --fps-factor 4 --render device --gif indexed      # 157 frames decoded from the 40 sampled ones
    python tools/demo.py --synthetic --noise counter --video-seeds 7,8,9 --batch 3   # three videos, each a function of its own seed
    python tools/demo.py --synthetic --from-video DIR --strength 0.5 --keep-box 0,0,16,32    # edit a video: keep the upper half of its latent
    python tools/demo.py --synthetic --out demo_out        # random-init weights, random image, fixed embedding:
                                                            # exercises the whole pipeline where no checkpoint exists
"""
import argparse
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvpr23_lfdm_amd import FlowDiffusion, io_compat as C  # noqa: E402


class Explicit(argparse.Action):
    """store, and note in `namespace.explicit` that the option was given: a distilled checkpoint (tools/distill_dm.py) replaces the
    DEFAULTS of --steps / --step-grid / --sampler and is contradicted only by what the command line really asked for."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        namespace.__dict__.setdefault("explicit", set()).add(self.dest)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "lfae_128.yaml"))
    ap.add_argument("--lfae-ckpt", default="", help="RegionMM_*.pth (keys generator / region_predictor / bg_predictor)")
    ap.add_argument("--dm-ckpt", default="", help="flowdiff_*.pth (key 'diffusion')")
    ap.add_argument("--bert", default=os.environ.get("LFDM_BERT_PATH"), help="local bert-base-cased directory")
    ap.add_argument("--image", default="")
    ap.add_argument("--text", nargs="+", default=["happiness"])
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100, action=Explicit, help="sampler steps (sampling_timesteps): DDIM, or --sampler's; default 100 - for a "
                    "checkpoint of tools/distill_dm.py the step count it was distilled to (another value is allowed, with a warning)")
    ap.add_argument("--cond-scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--out", default="demo_out")
    ap.add_argument("--conv-precision", choices=("fp32", "bf16"), default="fp32",
                    help="operands of the UNet's Winograd 3x3 convolutions: bf16 is the faster, lower-precision sampling mode (DESIGN.md)")
    ap.add_argument("--sampler", choices=("reference", "dpmpp_1", "dpmpp_2m"), default="reference", action=Explicit,
                    help="reference (default): DDIM / DDPM as the reference samples; dpmpp_2m: DPM-Solver++(2M), second order, for few --steps "
                         "(DESIGN.md 4.2); a distilled checkpoint is a DDIM model: anything but reference is an error")
    ap.add_argument("--total-frames", type=int, default=0,
                    help="a video of this many frames, longer than --frames, as a chain of overlapping windows conditioned on known frames "
                         "(FlowDiffusion.sample_long_video, DESIGN.md 4.3); 0 (default): off, one window of --frames")
    ap.add_argument("--overlap", type=int, default=8, help="latent frames two consecutive windows of --total-frames share")
    ap.add_argument("--long-method", choices=("chain", "joint"), default="chain",
                    help="how --total-frames is made: chain (default) - window after window, each conditioned on its predecessor's overlap "
                         "frames; joint - one latent of --total-frames frames whose overlapping windows are denoised together, their outputs "
                         "averaged per step (a heuristic; DESIGN.md 4.17)")
    ap.add_argument("--blend", choices=("ramp", "uniform"), default="ramp",
                    help="--long-method joint: the weight of a window's frame in the average - ramp (default): more towards the window's "
                         "middle; uniform")
    ap.add_argument("--window-labels", default="",
                    help="--long-method joint: comma-separated prompts, one per window, in place of --text (cross-faded over the overlaps); "
                         "the number of windows is printed when it does not match")
    ap.add_argument("--known-level", choices=("noised", "clean"), default="noised",
                    help="how known content (--total-frames' overlap frames, --keep-box / --regen-box) is held during sampling: on the step's "
                         "noise level (default), or clean at every step - for a checkpoint trained with tools/train_dm.py --known-prob "
                         "(DESIGN.md 4.12)")
    ap.add_argument("--objective", choices=("pred_noise", "pred_x0", "pred_v"), default=None,
                    help="what the denoiser predicts (tools/train_dm.py --objective, DESIGN.md 4.14); default: the checkpoint's own entry "
                         "(pred_noise where it has none) - a value that contradicts the checkpoint is an error")
    ap.add_argument("--schedule", choices=("cosine", "cosine_zsnr"), default=None,
                    help="the noise schedule the checkpoint was trained on (tools/train_dm.py --schedule, DESIGN.md 4.15); default: the "
                         "checkpoint's own entry (cosine where it has none) - a value that contradicts the checkpoint is an error")
    ap.add_argument("--step-grid", choices=("reference", "trailing"), default="reference", action=Explicit,
                    help="the DDIM / --sampler time grid: the reference's (default), or trailing - it starts at the last timestep and ends on "
                         "the clean latent (Lin et al. 2024, DESIGN.md 4.15); a distilled checkpoint defaults to trailing, at eta 0, and "
                         "reference is then an error (DESIGN.md 4.16)")
    ap.add_argument("--guidance-rescale", type=float, default=0.0,
                    help="phi in [0, 1]: with --cond-scale other than 0 and 1, scale the guided output towards the conditional output's "
                         "standard deviation (Lin et al. 2024, DESIGN.md 4.15); 0 (default): off")
    ap.add_argument("--use-ema", action="store_true",
                    help="sample from the averaged weights: the checkpoint's 'diffusion_ema' entry (tools/train_dm.py --ema-decay, DESIGN.md 4.4)")
    ap.add_argument("--long-attention", action="store_true", help="windows of 65 ... 256 frames (and a mid block of up to 256 pixels per frame) on the streaming attention kernels (FlowDiffusion(long_attention=True), DESIGN.md 4.8)")
    ap.add_argument("--render", choices=("host", "device"), default="host",
                    help="where the panel strip is made: host (default; io_compat.video_strip, per frame with numpy / matplotlib) or device "
                         "(one rendering on the GPU and one copy; the fourth panel is then the colour-coded flow, DESIGN.md 4.5)")
    ap.add_argument("--gif", choices=("rgb", "indexed"), default="rgb",
                    help="rgb (default): RGB frames, PIL quantises each; indexed: the device's 6x6x6-palette indices (ordered dither) written "
                         "as they are - needs --render device")
    ap.add_argument("--fps-factor", type=int, default=1,
                    help="K output frames per sampled interval, decoded from the sampled latent at the times j / K (FlowDiffusion.decode_at, "
                         "DESIGN.md 4.9): (frames - 1) * K + 1 frames for the sampling cost of --frames; 1 (default): off")
    ap.add_argument("--interp", choices=("linear", "cubic"), default="linear", help="how the latent is interpolated between sampled frames")
    ap.add_argument("--noise", choices=("torch", "counter"), default="torch",
                    help="torch (default): sampling noise from torch's generator under --seed; counter: every video has a seed of its own and "
                         "is the same video alone, in any batch and at any place in it (--video-seeds, DESIGN.md 4.10)")
    ap.add_argument("--video-seeds", default="", help="--noise counter: comma-separated integers in [0, 2^64), one per video of --batch "
                                                      "(default: --seed, --seed + 1, ...)")
    ap.add_argument("--save-latents", action="store_true",
                    help="--noise counter: also write every video's sampled latent to OUT/latent_<prompt index>_seed<seed>.npy")
    ap.add_argument("--batch", type=int, default=1, help="videos sampled at once per text prompt (same image and prompt; they differ in their noise)")
    ap.add_argument("--reverse", action="store_true", help="play the sampled motion backwards")
    ap.add_argument("--pingpong", action="store_true", help="forward, then back: a GIF that loops seamlessly")
    ap.add_argument("--from-video", default="",
                    help="edit an existing video (DESIGN.md 4.11): a folder of frames (sorted by name; the first --frames are read, the first "
                         "one is the source image unless --image is given), encoded to a latent by the LFAE (FlowDiffusion.encode_video); "
                         "with --synthetic and no readable folder a synthetic video is used")
    ap.add_argument("--strength", type=float, default=None,
                    help="--from-video: in (0, 1] - how far the video is noised before it is denoised again; the last ceil(strength * steps) "
                         "steps run (1: all of them, only the known box then ties the result to the video)")
    ap.add_argument("--keep-box", default="", help="--from-video: y0,x0,y1,x1 in latent pixels (size / 4) - kept from the encoded video in "
                                                   "every frame, the rest is regenerated")
    ap.add_argument("--regen-box", default="", help="--from-video: y0,x0,y1,x1 in latent pixels - regenerated, everything else is kept")
    return ap


def parse_box(text, size):
    """'y0,x0,y1,x1' -> the four integers, 0 <= y0 < y1 <= size and 0 <= x0 < x1 <= size; ValueError otherwise."""
    try:
        y0, x0, y1, x1 = (int(v) for v in text.split(","))
    except ValueError:
        raise ValueError("a box is four comma-separated integers y0,x0,y1,x1, got %r" % (text,))
    if not (0 <= y0 < y1 <= size and 0 <= x0 < x1 <= size):
        raise ValueError("box %r does not lie inside the %d x %d latent (0 <= y0 < y1 <= %d, 0 <= x0 < x1 <= %d)" % (text, size, size, size, size))
    return y0, x0, y1, x1


def box_mask(shape, box, keep):
    """The (B, 1, T, S, S) bool known-element mask of a latent of `shape`: True inside `box` (keep) or outside it (keep=False), every frame."""
    b, _, t, s, _ = shape
    y0, x0, y1, x1 = box
    mask = torch.zeros((b, 1, t, s, s), dtype=torch.bool)
    mask[:, :, :, y0:y1, x0:x1] = True
    return mask if keep else ~mask


def read_video(args, ref):
    """(B = 1, 3, --frames, size, size) in [0, 1] on the GPU: the frames of --from-video, or the synthetic stand-in (a slow drift of `ref`)."""
    names = sorted(os.listdir(args.from_video)) if os.path.isdir(args.from_video) else []
    if names:
        if len(names) < args.frames:
            sys.exit("--from-video: %s holds %d frames, --frames %d are needed" % (args.from_video, len(names), args.frames))
        frames = [C.resize(C.imread(os.path.join(args.from_video, n))[:, :, :3], args.size, interpolation=C.INTER_AREA) for n in names[:args.frames]]
        vid = torch.from_numpy(np.stack([np.asarray(f, np.float32) / 255.0 for f in frames])).permute(3, 0, 1, 2).unsqueeze(0)
        return vid.cuda().contiguous()
    if not args.synthetic:
        sys.exit("--from-video: %r is no folder of frames" % args.from_video)
    shifts = [int(round(3 * np.sin(2 * np.pi * f / args.frames))) for f in range(args.frames)]
    return torch.stack([torch.roll(ref[0], shifts=(sh, -sh), dims=(1, 2)) for sh in shifts], dim=1).unsqueeze(0).contiguous()


def edit_arguments(args, model, ref):
    """The sample_one_video keywords of --from-video / --strength / --keep-box / --regen-box (empty without --from-video)."""
    if not args.from_video:
        return {}
    latent = model.encode_video(read_video(args, ref), ref)
    latent = latent.expand(args.batch, -1, -1, -1, -1).contiguous()
    kw = dict(start_latent=latent, strength=1.0 if args.strength is None else args.strength)
    box = args.keep_box or args.regen_box
    if box:
        mask = box_mask(tuple(latent.shape), parse_box(box, args.size // 4), keep=bool(args.keep_box))
        kw.update(known_latent=latent, known_mask=mask.cuda(), known_level=args.known_level)
    return kw


def retime(args, frames):
    """The frame times of --fps-factor / --reverse / --pingpong for a sample of `frames` frames, or None when none of them is given."""
    if args.fps_factor == 1 and not args.reverse and not args.pingpong:
        return None
    from cvpr23_lfdm_amd.retime import frame_times
    return frame_times(frames, args.fps_factor, reverse=args.reverse, pingpong=args.pingpong)


def check_args(args):
    if args.fps_factor < 1:
        sys.exit("--fps-factor must be at least 1")
    if args.gif == "indexed" and args.render != "device":
        sys.exit("--gif indexed needs --render device: the palette indices are made by the device rendering")
    if args.use_ema and (args.synthetic or not args.dm_ckpt):
        sys.exit("--use-ema needs --dm-ckpt: a checkpoint with a 'diffusion_ema' entry")
    if args.batch < 1:
        sys.exit("--batch must be at least 1")
    if (args.video_seeds or args.save_latents) and args.noise != "counter":
        sys.exit("--video-seeds / --save-latents need --noise counter")
    if (args.strength is not None or args.keep_box or args.regen_box) and not args.from_video:
        sys.exit("--strength / --keep-box / --regen-box need --from-video")
    if args.known_level == "clean" and not (args.total_frames > 0 or args.keep_box or args.regen_box):
        sys.exit("--known-level clean needs known content: --total-frames, or --from-video with --keep-box / --regen-box")
    if args.keep_box and args.regen_box:
        sys.exit("--keep-box and --regen-box exclude each other (one is the complement of the other)")
    if args.strength is not None and not 0.0 < args.strength <= 1.0:
        sys.exit("--strength must lie in (0, 1]")
    if (args.long_method != "chain" or args.blend != "ramp" or args.window_labels) and args.total_frames <= 0:
        sys.exit("--long-method / --blend / --window-labels need --total-frames")
    if (args.blend != "ramp" or args.window_labels) and args.long_method != "joint":
        sys.exit("--blend / --window-labels need --long-method joint")
    if args.long_method == "joint" and args.known_level == "clean":
        sys.exit("--known-level clean holds the chain's overlap frames: --long-method joint has none")
    if args.from_video and args.total_frames > 0:
        sys.exit("--from-video edits one window of --frames: it does not combine with --total-frames")
    for box in (args.keep_box, args.regen_box):
        if box:
            try:
                parse_box(box, args.size // 4)
            except ValueError as e:
                sys.exit(str(e))


def window_labels(args, windows):
    """--window-labels as a list of `windows` prompts, or None when the option is not given."""
    if not args.window_labels:
        return None
    labels = [v.strip() for v in args.window_labels.split(",")]
    if len(labels) != windows or not all(labels):
        sys.exit("--window-labels: %d frames at overlap %d are %d windows, one prompt each is needed, got %r"
                 % (args.total_frames, args.overlap, windows, args.window_labels))
    return labels


def video_seeds(args):
    """--noise counter: the list of --batch seeds (--video-seeds, or --seed, --seed + 1, ...); None under --noise torch."""
    if args.noise != "counter":
        return None
    if not args.video_seeds:
        return [(args.seed + j) % (1 << 64) for j in range(args.batch)]
    try:
        seeds = [int(v, 0) for v in args.video_seeds.split(",")]
    except ValueError:
        sys.exit("--video-seeds takes comma-separated integers, got %r" % args.video_seeds)
    if len(seeds) != args.batch or not all(0 <= v < (1 << 64) for v in seeds):
        sys.exit("--video-seeds: %d integers in [0, 2^64) are needed (--batch), got %r" % (args.batch, args.video_seeds))
    return seeds


def dm_state(ck, use_ema, path="the checkpoint"):
    """The diffusion state dict to sample from: 'diffusion', or with --use-ema the averaged 'diffusion_ema' - an error when there is none."""
    if not use_ema:
        return ck["diffusion"]
    if "diffusion_ema" not in ck:
        sys.exit("--use-ema: %s has no 'diffusion_ema' entry (keys: %s) - it was trained without --ema-decay; drop --use-ema to "
                 "sample from its raw weights" % (path, ", ".join(sorted(ck))))
    return ck["diffusion_ema"]


def make_model(args, *, steps=None, sampler=None, conv_precision=None, use_ema=None, need_dm=True, explicit=None):
    """The FlowDiffusion of the parsed options with its weights loaded, on the host (demo_mug.py:80-97); tools/eval.py builds its models
    here too.  steps / sampler / conv_precision / use_ema override the options of the same names; need_dm=False accepts a run without
    --dm-ckpt (an LFAE-only evaluation).  explicit: which of "steps" / "sampler" / "step_grid" were asked for rather than defaulted
    (default: what the command line gave, `Explicit`, and the overrides) - a distilled checkpoint's own entry stands in for the others."""
    if explicit is None:
        explicit = set(getattr(args, "explicit", ())) | {k for k, v in (("steps", steps), ("sampler", sampler)) if v is not None}
    steps = args.steps if steps is None else steps
    sampler = args.sampler if sampler is None else sampler
    step_grid = getattr(args, "step_grid", "reference")
    conv_precision = args.conv_precision if conv_precision is None else conv_precision
    use_ema = args.use_ema if use_ema is None else use_ema
    ck = torch.load(args.dm_ckpt, map_location="cpu") if args.dm_ckpt and not args.synthetic else None
    try:
        objective = C.checkpoint_objective(ck, getattr(args, "objective", None), args.dm_ckpt)
        schedule = C.checkpoint_schedule(ck, getattr(args, "schedule", None), args.dm_ckpt)
        # a checkpoint of tools/distill_dm.py says how it is sampled: its step count, the trailing grid, eta 0
        given = lambda name, value: value if name in explicit else None
        distilled = C.distilled_sampling(ck, given("steps", steps), given("step_grid", step_grid), given("sampler", sampler), args.dm_ckpt)
    except ValueError as e:
        sys.exit(str(e))
    eta = distilled[2]
    if eta is not None:
        steps, step_grid, sampler = distilled[0], distilled[1], "reference"
        if distilled[3]:
            print(distilled[3])
    try:
        model = FlowDiffusion(is_train=False, img_size=args.size // 4, num_frames=args.frames, sampling_timesteps=steps,
                              null_cond_prob=0.1, config_pth=args.config, pretrained_pth=args.lfae_ckpt,
                              bert_path=None if args.synthetic else args.bert, conv_precision=conv_precision,
                              sampler=sampler, long_attention=getattr(args, "long_attention", False),
                              noise=getattr(args, "noise", "torch"), objective=objective, schedule=schedule,
                              step_grid=step_grid, guidance_rescale=getattr(args, "guidance_rescale", 0.0),
                              **({} if eta is None else dict(ddim_sampling_eta=eta)))                         # demo_mug.py:80-88
    except ValueError as e:             # (cosine_zsnr with pred_noise, a --guidance-rescale outside [0, 1])
        sys.exit(str(e))
    if args.synthetic:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import synth
        model.unet.load_state_dict(synth.unet_state())
        model.generator.load_state_dict(synth.generator_state())
        emb = {}

        def encode(texts):          # a fixed embedding per prompt, seeded by the prompt
            for t in texts:
                if t not in emb:
                    emb[t] = torch.randn(1, 768, generator=torch.Generator().manual_seed(zlib.crc32(t.encode())))
            return torch.cat([emb[t] for t in texts])
        model.diffusion.text_encoder = encode
    elif args.dm_ckpt:
        model.diffusion.load_state_dict(dm_state(ck, use_ema, args.dm_ckpt))   # demo_mug.py:93-97
    elif need_dm:
        sys.exit("give --dm-ckpt (and --lfae-ckpt), or --synthetic")
    return model


def main():
    args = build_parser().parse_args()
    check_args(args)
    if not torch.cuda.is_available():
        sys.exit("tools/demo.py needs a GPU: the sampling path is liblfdm_hip.so only")
    os.makedirs(args.out, exist_ok=True)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)

    model = make_model(args)
    if args.synthetic and args.from_video:          # the LFAE's two predictors encode the video: synthetic weights for them too
        import synth
        model.region_predictor.load_state_dict(synth.region_state())
        model.bg_predictor.load_state_dict(synth.bg_state())
    model.cuda().eval()

    if args.image:
        img = C.resize(C.imread(args.image)[:, :, :3], args.size, interpolation=C.INTER_AREA)        # demo_mug.py:113-114
    else:
        img = np.random.default_rng(args.seed).integers(0, 256, size=(args.size, args.size, 3), dtype=np.uint8)
    ref = torch.from_numpy(np.asarray(img, np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0).cuda()
    seeds = video_seeds(args)
    skw = {} if seeds is None else dict(seeds=seeds)
    skw.update(edit_arguments(args, model, ref))
    name = os.path.splitext(os.path.basename(args.image))[0] if args.image else "random"
    for i, text in enumerate(args.text):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref_b = ref.expand(args.batch, -1, -1, -1).contiguous()
        model.set_sample_input(sample_img=ref_b, sample_text=[text] * args.batch)
        if args.total_frames > 0 and args.long_method == "joint":
            labels = window_labels(args, len(model.joint_windows(args.total_frames, args.overlap)))
            model.sample_long_video(args.cond_scale, args.total_frames, overlap=args.overlap, method="joint", blend=args.blend,
                                    window_text=None if labels is None else [[label] * args.batch for label in labels],
                                    **({} if seeds is None else dict(seed=seeds)))
        elif args.total_frames > 0:
            model.sample_long_video(args.cond_scale, args.total_frames, overlap=args.overlap, known_level=args.known_level,
                                    **({} if seeds is None else dict(seed=seeds)))
        else:
            model.sample_one_video(cond_scale=args.cond_scale, **skw)
        if seeds is not None:           # a video's identity: its seed, a checksum of its x_T (window 0) and of the latent it gave
            from cvpr23_lfdm_amd import ops
            x_t = ops.philox_normal(torch.empty((len(seeds), 3, args.frames, args.size // 4, args.size // 4), device="cuda"), seeds,
                                    stream=ops.NOISE_STREAM_XT).cpu().numpy()
            for j, sd in enumerate(seeds):
                lat = model.sample_latent[j].float().cpu().numpy()
                print("video seed %d: x_T crc32 %08x, latent crc32 %08x, mean |latent| %.6f"
                      % (sd, zlib.crc32(x_t[j].tobytes()), zlib.crc32(lat.tobytes()), float(np.abs(lat).mean())))
                if args.save_latents:
                    np.save(os.path.join(args.out, "latent_%04d_seed%d.npy" % (i, sd)), lat)
        times = retime(args, args.total_frames if args.total_frames > 0 else args.frames)
        if times is not None:
            model.decode_at(times, args.interp)
        path = os.path.join(args.out, "%04d_%s_%s_%.2f.gif" % (i, text.replace(" ", "_"), name, args.cond_scale))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if args.render == "device":
            frames = C.video_strip_device(model, ref_b, indexed=args.gif == "indexed")
        else:
            frames = C.video_strip(model, ref)
        t2 = time.perf_counter()
        if args.gif == "indexed":
            C.mimsave_indexed(path, frames)
        else:
            C.mimsave(path, frames)
        t3 = time.perf_counter()
        print(path)
        print("%s: sample %.3f s, render (%s) %.3f s, write (%s) %.3f s" % (os.path.basename(path), t1 - t0, args.render, t2 - t1,
                                                                           args.gif, t3 - t2))


if __name__ == "__main__":
    main()
