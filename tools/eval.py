#!/usr/bin/env python
"""Paired, full-reference evaluation of checkpoints on the device (cvpr23_lfdm_amd.evaluate): per-frame L1, MSE / PSNR and
SSIM in image space, end-point and occlusion error in latent-flow space.  Four subcommands share tools/demo.py's model options:

  lfae   the reference's LFAE/test_flowautoenc_*.py loop: every test video reconstructed from its first frame through the frozen LFAE;
         the JSON carries the reference's keys out_loss / warp_loss (same normalisation) plus L1 / PSNR / SSIM of both outputs
  dm     DM/test_video_flow_diffusion_*.py's sampling loop with a measurement: a video sampled from each test video's first frame and
         label, against the real video, against the LFAE's own reconstruction and, in flow space, against the pseudo ground truth
  ab     two sampling configurations on one input, B against A per frame and in summary (what is paired: DESIGN.md 4.6)
  interp what temporal interpolation of the latent costs on real motion: every test video's pseudo-ground-truth latent
         thinned to every --factor-th frame, resampled back (--interp linear | cubic) and decoded, against the full latent's decode

    python tools/eval.py lfae --lfae-ckpt RegionMM.pth --dataset mug --data-dir /data/MUG --out lfae.json
    python tools/eval.py dm --lfae-ckpt RegionMM.pth --dm-ckpt flowdiff.pth --bert /data/bert-base-cased --dataset mug --data-dir /data/MUG
    python tools/eval.py ab --lfae-ckpt RegionMM.pth --dm-ckpt flowdiff.pth --bert /data/bert-base-cased --image face.jpg --text anger \
        --a sampler=reference,steps=100 --b sampler=dpmpp_2m,steps=20,conv_precision=bf16
    python tools/eval.py interp --lfae-ckpt RegionMM.pth --dataset mug --data-dir /data/MUG --factor 2 --interp cubic
    python tools/eval.py ab --synthetic --a steps=10 --b steps=10,conv_precision=bf16      # random-init weights: exercises the path

FVD is not computed: it needs an I3D network this repository does not ship.  Non-finite numbers (the PSNR of equal frames) are written
to the JSON as the strings "inf" / "-inf" / "nan".
"""
import argparse
import importlib.util
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvpr23_lfdm_amd import _native, datasets, evaluate as E, io_compat as C  # noqa: E402

DATASETS = {"mug": datasets.MUG_test, "mhad": datasets.MHAD_test, "natops": datasets.NATOPS_test}
AB_KEYS = {"sampler": str, "steps": int, "conv_precision": str, "use_ema": lambda v: v.lower() in ("1", "true", "yes"), "long_method": str}
HELD_FIXED_COUNTER = ["source image", "text condition", "cond_scale",
                      "the video's seed (--noise counter): the same x_T, the same known-frame noise, and the same step noise at every step index "
                      "both configurations draw at"]
HELD_FIXED = ["source image", "text condition", "cond_scale", "torch.manual_seed before each run: the same x_T (every sampler's first draw)",
              "per-step noise only where both configurations use the reference sampler with equal step counts"]


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="command", required=True)

    def common(p):
        p.add_argument("--config", default=os.path.join(ROOT, "configs", "lfae_128.yaml"))
        p.add_argument("--lfae-ckpt", default="", help="RegionMM_*.pth (keys generator / region_predictor / bg_predictor)")
        p.add_argument("--dm-ckpt", default="", help="flowdiff_*.pth (key 'diffusion')")
        p.add_argument("--bert", default=os.environ.get("LFDM_BERT_PATH"), help="local bert-base-cased directory")
        p.add_argument("--size", type=int, default=128)
        p.add_argument("--frames", type=int, default=40)
        p.add_argument("--synthetic", action="store_true", help="random-init weights and synthetic videos: exercises the path without checkpoints")
        p.add_argument("--sampler", choices=("reference", "dpmpp_1", "dpmpp_2m"), default="reference", action=_demo().Explicit,
                       help="default reference; a distilled checkpoint (tools/distill_dm.py) is a DDIM model: anything else is an error")
        p.add_argument("--steps", type=int, default=100, action=_demo().Explicit, help="default 100; for a distilled checkpoint the step count it was distilled to")
        p.add_argument("--conv-precision", choices=("fp32", "bf16"), default="fp32")
        p.add_argument("--objective", choices=("pred_noise", "pred_x0", "pred_v"), default=None,
                       help="what the denoiser predicts (DESIGN.md 4.14); default: the checkpoint's own entry - a contradiction is an error")
        p.add_argument("--schedule", choices=("cosine", "cosine_zsnr"), default=None,
                       help="the noise schedule the checkpoint was trained on (DESIGN.md 4.15); default: the checkpoint's own entry - a contradiction is an error")
        p.add_argument("--step-grid", choices=("reference", "trailing"), default="reference", action=_demo().Explicit,
                       help="the sampler's time grid: the reference's (default), or trailing - from the last timestep to the clean latent "
                            "(DESIGN.md 4.15); a distilled checkpoint defaults to trailing at eta 0 and refuses reference (DESIGN.md 4.16)")
        p.add_argument("--guidance-rescale", type=float, default=0.0,
                       help="phi in [0, 1]: rescale the guided output (--cond-scale other than 0 and 1) towards the conditional output's standard deviation (DESIGN.md 4.15)")
        p.add_argument("--use-ema", action="store_true", help="sample from the checkpoint's 'diffusion_ema' entry")
        p.add_argument("--long-attention", action="store_true", help="windows of 65 ... 256 frames (and a mid block of up to 256 pixels per frame) on the streaming attention kernels (FlowDiffusion(long_attention=True), DESIGN.md 4.8)")
        p.add_argument("--cond-scale", type=float, default=1.0)
        p.add_argument("--seed", type=int, default=1234)
        p.add_argument("--noise", choices=("torch", "counter"), default="torch",
                       help="counter: sampled videos take their noise from per-video seeds (ab: both sides get --seed as the video's seed)")
        p.add_argument("--domain", choices=("raw", "unit", "uint8"), default="unit", help="value domain of L1 / PSNR / SSIM (out_loss / warp_loss are always raw)")
        p.add_argument("--out", default="", help="JSON file to write (default: eval_<command>.json)")

    def data(p):
        p.add_argument("--dataset", choices=sorted(DATASETS), default="mug")
        p.add_argument("--data-dir", default="")
        p.add_argument("--batch-size", type=int, default=1)
        p.add_argument("--max-videos", type=int, default=0, help="stop after this many test videos (0: all)")
        p.add_argument("--mean", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("R", "G", "B"),
                       help="the data set's mean on the 0 .. 255 scale, subtracted from every frame and added back by the unit / uint8 domains; "
                            "0 0 0 (default) is the MEAN of every reference train / test script - NOT the data-set classes' own default")

    for name in ("lfae", "dm"):
        p = sub.add_parser(name)
        common(p)
        data(p)
    p = sub.add_parser("interp")
    common(p)
    data(p)
    p.add_argument("--factor", type=int, default=2, help="keep every FACTOR-th latent frame and interpolate the others back; of each video the "
                                                          "first 1 + FACTOR * ((frames - 1) // FACTOR) frames are used")
    p.add_argument("--interp", choices=("linear", "cubic"), default="linear")
    p = sub.add_parser("ab")
    common(p)
    p.add_argument("--a", default="", help="configuration A as key=value[,key=value...] over sampler, steps, conv_precision, use_ema")
    p.add_argument("--b", default="", help="configuration B, likewise; unset keys take the shared options")
    p.add_argument("--image", default="")
    p.add_argument("--text", default="happiness")
    p.add_argument("--total-frames", type=int, default=0, help="both sides sample a long video of this many frames "
                                                                "(FlowDiffusion.sample_long_video); 0 (default): one window of --frames")
    p.add_argument("--overlap", type=int, default=8, help="latent frames two consecutive windows of --total-frames share")
    p.add_argument("--long-method", choices=("chain", "joint"), default="chain",
                   help="how --total-frames is made (DESIGN.md 4.3 / 4.17); a side's own long_method=... in --a / --b wins: "
                        "--a long_method=chain --b long_method=joint compares the two")
    p.add_argument("--blend", choices=("ramp", "uniform"), default="ramp", help="the joint method's window profile")
    return ap


def parse_overrides(spec):
    out = {}
    for item in filter(None, (s.strip() for s in spec.split(","))):
        key, sep, value = item.partition("=")
        if not sep or key not in AB_KEYS:
            sys.exit("--a / --b take key=value pairs over %s, got %r" % (", ".join(sorted(AB_KEYS)), item))
        out[key] = AB_KEYS[key](value)
    return out


def device():
    """The product library drives the GPU; the x86 emulation build (tests only) drives CPU tensors."""
    if _native.library().kind == "emu":
        return "cpu"
    if not torch.cuda.is_available():
        sys.exit("tools/eval.py needs a GPU: the models and the metrics run on liblfdm_hip.so only")
    return "cuda"


def _demo():
    """tools/demo.py as a module: the model of the shared options is built by its make_model."""
    if "lfdm_demo_tool" not in sys.modules:
        spec = importlib.util.spec_from_file_location("lfdm_demo_tool", os.path.join(ROOT, "tools", "demo.py"))
        sys.modules["lfdm_demo_tool"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules["lfdm_demo_tool"])
    return sys.modules["lfdm_demo_tool"]


def build_model(args, overrides=None):
    """The model of tools/demo.py (its make_model) for the shared options, with `overrides` (an --a / --b list) on top."""
    cfg = dict(sampler=args.sampler, steps=args.steps, conv_precision=args.conv_precision, use_ema=args.use_ema)
    cfg.update(overrides or {})
    long_method = cfg.pop("long_method", getattr(args, "long_method", "chain"))         # (no option of the model: of how it is sampled)
    if long_method not in ("chain", "joint"):
        sys.exit("long_method is chain or joint, got %r" % (long_method,))
    if cfg["use_ema"] and (args.synthetic or not args.dm_ckpt):
        sys.exit("use_ema needs --dm-ckpt: a checkpoint with a 'diffusion_ema' entry")
    explicit = set(getattr(args, "explicit", ())) | set(overrides or {})       # (asked for on the command line or by an --a / --b list)
    model = _demo().make_model(args, need_dm=args.command not in ("lfae", "interp"), explicit=explicit, **cfg)
    if args.synthetic:          # the frozen-LFAE pass also runs the two predictors, which the demo never does
        import synth
        model.region_predictor.load_state_dict(synth.region_state())
        model.bg_predictor.load_state_dict(synth.bg_state())
    cfg.update(sampler=model.diffusion.sampler, steps=model.diffusion.sampling_timesteps)       # (as resolved: the defaults, a distilled checkpoint's own)
    if getattr(args, "total_frames", 0):
        cfg.update(long_method=long_method)
    return model.to(device()).eval(), cfg


def batches(args):
    """-> (mean, iterator of (real_vid (B, 3, T, H, W), labels, names))"""
    if args.synthetic:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import synth
        vid = synth.train_inputs(2, args.frames, args.size)[1]
        return (0.0, 0.0, 0.0), iter([(vid[i:i + 1], ["happiness"], ["synthetic_%d" % i]) for i in range(2)])
    if not args.data_dir:
        sys.exit("give --data-dir (the %s test set), or --synthetic" % args.dataset)
    mean = tuple(float(m) for m in args.mean)
    # (the reference loops pass mean=MEAN=(0, 0, 0), LFAE/test_flowautoenc_*.py:34,116: the checkpoints were trained on x / 255)
    ds = DATASETS[args.dataset](args.data_dir, num_frames=args.frames, image_size=args.size, mean=mean)
    n = min(len(ds), args.max_videos) if args.max_videos else len(ds)

    def it():
        for i0 in range(0, n, args.batch_size):
            items = [ds[i] for i in range(i0, min(n, i0 + args.batch_size))]
            yield torch.from_numpy(np.stack([v for v, _, _ in items])), [l for _, l, _ in items], [m for _, _, m in items]
    return mean, it()


def jsonable(v):
    if isinstance(v, dict):
        return {k: jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [jsonable(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return str(v)
    return v


def run_lfae(args):
    model, _ = build_model(args)
    mean, it = batches(args)
    acc = {k: E.MetricAccumulator() for k in ("out", "warp", "out_raw", "warp_raw")}
    for real_vid, _, _ in it:
        res = E.lfae_reconstruction(model, real_vid, real_vid[:, :, 0], mean=mean, domain=args.domain)
        for k in acc:
            acc[k].update(res[k]["table"])
    s = {k: a.result() for k, a in acc.items()}
    return {"out_loss": E.reference_loss(s["out_raw"]), "warp_loss": E.reference_loss(s["warp_raw"]), "out": s["out"], "warp": s["warp"],
            "videos": s["out"]["videos"], "frames": s["out"]["frames"], "domain": args.domain, "mean": list(mean)}


def run_dm(args):
    model, cfg = build_model(args)
    mean, it = batches(args)
    acc = {k: E.MetricAccumulator() for k in ("vs_real", "vs_lfae", "lfae")}
    flow = E.FlowAccumulator()
    torch.manual_seed(args.seed)
    for real_vid, labels, _ in it:
        model.set_sample_input(sample_img=real_vid[:, :, 0], sample_text=labels)
        model.sample_one_video(cond_scale=args.cond_scale)
        res = E.sample_against_real(model, real_vid, mean=mean, domain=args.domain)
        for k in acc:
            acc[k].update(res[k]["table"])
        flow.update(res["flow"]["table"])
    out = {k: a.result() for k, a in acc.items()}
    out.update(flow=flow.result(), config=cfg, cond_scale=args.cond_scale, seed=args.seed,
               domain=args.domain, mean=list(mean))
    return out


def run_interp(args):
    if args.factor < 1:
        sys.exit("--factor must be at least 1")
    model, _ = build_model(args)
    mean, it = batches(args)
    names = ("video", "interp_vs_real", "lfae_vs_real")
    acc = {k: E.MetricAccumulator() for k in names}
    held = {k: E.MetricAccumulator() for k in names}
    flow, flow_held = E.FlowAccumulator(), E.FlowAccumulator()
    used = 0
    for real_vid, _, _ in it:
        used = 1 + args.factor * ((real_vid.shape[2] - 1) // args.factor)
        real_vid = real_vid[:, :, :used]
        res = E.interpolation_error(model, real_vid, real_vid[:, :, 0], factor=args.factor, mode=args.interp, mean=mean, domain=args.domain)
        mask = res["held_out"]
        for k in names:
            acc[k].update(res[k]["table"])
            if bool(mask.any()):
                held[k].update(res[k]["table"][:, mask.to(res[k]["table"].device)].contiguous())
        flow.update(res["flow"]["table"])
        if bool(mask.any()):
            flow_held.update(res["flow"]["table"][:, mask.to(res["flow"]["table"].device)].contiguous())
    out = {k: a.result() for k, a in acc.items()}
    out["flow"] = flow.result()
    if flow_held.frames:
        out["held_out"] = dict({k: a.result() for k, a in held.items()}, flow=flow_held.result())
    out.update(factor=args.factor, interp=args.interp, frames_used=used, domain=args.domain, mean=list(mean))
    return out


def run_ab(args):
    model_a, cfg_a = build_model(args, parse_overrides(args.a))
    model_b, cfg_b = build_model(args, parse_overrides(args.b))
    if args.image:
        img = C.resize(C.imread(args.image)[:, :, :3], args.size, interpolation=C.INTER_AREA)
    else:
        img = np.random.default_rng(args.seed).integers(0, 256, size=(args.size, args.size, 3), dtype=np.uint8)
    ref = torch.from_numpy(np.asarray(img, np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    counter = args.noise == "counter"
    if args.total_frames <= 0 and (args.long_method != "chain" or args.blend != "ramp"):
        sys.exit("--long-method / --blend need --total-frames")
    res = E.ab_compare(model_a, model_b, ref, [args.text], cond_scale=args.cond_scale, seed=args.seed, domain=args.domain,
                       seeds=[args.seed % (1 << 64)] if counter else None, total_frames=max(args.total_frames, 0), overlap=args.overlap,
                       methods=(cfg_a.get("long_method", "chain"), cfg_b.get("long_method", "chain")), blend=args.blend)
    video, flow = res["video"]["table"][0].cpu(), res["flow"]["table"][0].cpu()
    psnr = res["video"]["psnr"][0].cpu().tolist()
    print("B against A per frame:  frame        l1       mse      psnr      ssim       epe  occl.err")
    for f in range(video.shape[0]):
        print("                        %5d  %.3e %.3e %9.4f %9.6f %.3e %.3e" % ((f,) + tuple(video[f, :2].tolist()) + (psnr[f], float(video[f, 2]))
                                                                                + tuple(flow[f].tolist())))
    return {"a": cfg_a, "b": cfg_b, "video": res["video"]["summary"], "flow": res["flow"]["summary"],
            "per_frame": dict(l1=video[:, 0].tolist(), mse=video[:, 1].tolist(), psnr=psnr, ssim=video[:, 2].tolist(),
                              epe=flow[:, 0].tolist(), occlusion_error=flow[:, 1].tolist()),
            "held_fixed": HELD_FIXED_COUNTER if counter else HELD_FIXED, "text": args.text, "cond_scale": args.cond_scale, "seed": args.seed, "domain": args.domain}


def main(argv=None):
    args = build_parser().parse_args(argv)
    out = jsonable({"lfae": run_lfae, "dm": run_dm, "ab": run_ab, "interp": run_interp}[args.command](args))
    out["command"] = args.command
    path = args.out or "eval_%s.json" % args.command
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: v for k, v in out.items() if k != "per_frame"}))
    print(path)
    return out


if __name__ == "__main__":
    main()
