#!/usr/bin/env python
"""The reference's DM training driver (DM/train_video_flow_diffusion_{mug,mhad,natops}.py:130-420 and the _multiGPU variant)
on this framework: same loop, checkpoint format ({'example', 'diffusion', 'optimizer_diff'}), MultiStepLR schedule and
restore semantics; one process per GPU under torchrun instead of nn.DataParallel threads.  Needs GPUs.

    python tools/train_dm.py --data DIR --lfae-ckpt RegionMM.pth --bert /data/bert-base-cased --out snapshots
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 tools/train_dm.py --data DIR ...
    python tools/train_dm.py --synthetic --final-step 20          # random videos / random-init LFAE: exercises the loop
    python tools/pack_videos.py DIR PACKED --store-size 128 && python tools/train_dm.py --packed PACKED [--resident] ...
        # frames decoded once into a uint8 store; jitter, shrink and normalisation on the device
    python tools/train_dm.py --data DIR ... --ema-decay 0.9999 --ema-start-step 2000 --max-grad-norm 1.0 --skip-nonfinite
        # averaged weights (checkpoint entry "diffusion_ema", tools/demo.py --use-ema), clipping and the non-finite guard: DESIGN.md 4.4
    python tools/pack_latents.py PACKED --lfae-ckpt RegionMM.pth && python tools/train_dm.py --packed PACKED --latents [--resident] ...
        # the frozen LFAE's flow latents computed once; a step gathers them and launches no LFAE predictor or decoder
"""
import argparse
import contextlib
import math
import os
import sys
import timeit

import numpy as np
import torch
import torch.distributed as dist
from torch.optim.lr_scheduler import MultiStepLR
from torch.utils import data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvpr23_lfdm_amd import FlowDiffusion, io_compat as C  # noqa: E402
from cvpr23_lfdm_amd.data import FrameFolderVideos, SyntheticVideos  # noqa: E402


def build_parser(description=__doc__):
    """The trainer's options (tools/distill_dm.py adds its own to the same parser)."""
    ap = argparse.ArgumentParser(description=description, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", default="")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "lfae_128.yaml"))
    ap.add_argument("--lfae-ckpt", default="")
    ap.add_argument("--bert", default=os.environ.get("LFDM_BERT_PATH"))
    ap.add_argument("--restore-from", default="")
    ap.add_argument("--set-start", action="store_true")
    ap.add_argument("--out", default="snapshots")
    ap.add_argument("--batch-size", type=int, default=8, help="per GPU")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--null-cond-prob", type=float, default=0.1)
    ap.add_argument("--epoch-milestones", type=int, nargs="*", default=[800, 1000])
    ap.add_argument("--final-step", type=int, default=200000)
    ap.add_argument("--save-freq", type=int, default=2000)
    ap.add_argument("--print-freq", type=int, default=10)
    ap.add_argument("--save-img-freq", type=int, default=500)
    ap.add_argument("--num-workers", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--ema-decay", type=float, default=None, help="keep an exponential moving average of the denoiser's weights with this "
                    "decay; checkpoints gain a 'diffusion_ema' entry and previews are sampled from it")
    ap.add_argument("--ema-start-step", type=int, default=0, help="the average tracks the weights exactly through this many applied steps")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="clip the global gradient norm (torch clip_grad_norm_ semantics)")
    ap.add_argument("--skip-nonfinite", action="store_true", help="skip a step whose gradient holds an inf / nan instead of losing the run")
    ap.add_argument("--preview-steps", type=int, default=0, help="> 0: at --save-img-freq also SAMPLE one video with this many DDIM steps "
                    "(from the averaged weights under --ema-decay) and write it as a GIF")
    ap.add_argument("--packed", default="", help="a store written by tools/pack_videos.py (instead of --data): batches cross to the device "
                    "as bytes and colour jitter, area shrink and normalisation run there")
    ap.add_argument("--resident", action="store_true", help="with --packed: upload the whole store once; a batch is then frame numbers")
    ap.add_argument("--latents", action="store_true", help="with --packed: train from the flow-latent store tools/pack_latents.py wrote "
                    "beside the frames - a step gathers the stored latents and runs nothing of the frozen LFAE but the reference frame's "
                    "encoder; the decoded videos and loss_rec / loss_warp are computed at --save-img-freq only (DESIGN.md 4.13)")
    ap.add_argument("--dim-mults", type=int, nargs="+", default=[1, 2, 4, 8], help="the denoiser's channel multipliers (FlowDiffusion(dim_mults=...))")
    ap.add_argument("--long-attention", action="store_true", help="windows of 65 ... 256 frames (and a mid block of up to 256 pixels per frame) on the streaming attention kernels (FlowDiffusion(long_attention=True), DESIGN.md 4.8)")
    ap.add_argument("--known-prob", type=float, default=0.0, help="> 0: random-mask training (FlowDiffusion(known_train=...), DESIGN.md 4.12) - "
                    "with this probability some frames of a training video stay clean and the loss counts the others; sample the "
                    "checkpoint with known_level='clean' (tools/demo.py --known-level clean)")
    ap.add_argument("--known-kinds", nargs="+", choices=("prefix", "ends", "random"), default=["prefix", "ends", "random"],
                    help="--known-prob: the mask kinds drawn from")
    ap.add_argument("--known-max-frames", type=int, default=8, help="--known-prob: at most this many known frames (at most --frames - 1)")
    ap.add_argument("--known-seed", type=int, default=0, help="--known-prob: seed of the mask stream (not stored in checkpoints: a resumed run "
                    "starts the stream again)")
    ap.add_argument("--objective", choices=("pred_noise", "pred_x0", "pred_v"), default="pred_noise",
                    help="what the denoiser predicts (FlowDiffusion(objective=...), DESIGN.md 4.14): the noise (default, the reference's), x0, "
                         "or v = a noise - s x0; stored in the checkpoint, which tools/demo.py and tools/eval.py then sample accordingly")
    ap.add_argument("--schedule", choices=("cosine", "cosine_zsnr"), default="cosine",
                    help="the noise schedule (FlowDiffusion(schedule=...), DESIGN.md 4.15): the reference's cosine (default) or cosine_zsnr, the "
                         "same rescaled to zero terminal SNR (Lin et al. 2024; needs --objective pred_v or pred_x0); stored in the checkpoint, "
                         "which tools/demo.py and tools/eval.py then sample on")
    ap.add_argument("--min-snr-gamma", type=float, default=None,
                    help="min-SNR-gamma loss weights (Hang et al. 2023; 5 is the paper's value); default: every timestep weighs 1")
    ap.add_argument("--log-loss-quartiles", action="store_true",
                    help="at --print-freq also print the mean unweighted per-sample loss by quartile of the timestep (accumulated on the "
                         "device, read back only when printed); needs --objective other than pred_noise or --min-snr-gamma")
    return ap


def parse_args(argv=None):
    return build_parser().parse_args(argv)


class LossQuartiles:
    """--log-loss-quartiles: sums and counts of diffusion.sample_loss by quartile of diffusion.sample_t in one (2, 4) device tensor; `add`
    launches and reads nothing back, `means` (at --print-freq) reads the four means and starts again."""

    def __init__(self, timesteps):
        self.timesteps, self.acc = int(timesteps), None

    def add(self, sample_loss, sample_t):
        if self.acc is None:
            self.acc = torch.zeros(2, 4, dtype=torch.float32, device=sample_loss.device)
        q = (sample_t * 4 // self.timesteps).clamp_(0, 3)
        self.acc[0].index_add_(0, q, sample_loss.detach())
        self.acc[1].index_add_(0, q, torch.ones_like(sample_loss))
        return self

    def means(self):
        if self.acc is None:
            return [float("nan")] * 4
        out = (self.acc[0] / self.acc[1]).tolist()          # (an empty quartile: nan)
        self.acc.zero_()
        return out


def known_train(args):
    """The known_train option of FlowDiffusion for --known-prob / --known-kinds / --known-max-frames / --known-seed (None: off)."""
    if args.known_prob <= 0:
        return None
    return dict(prob=args.known_prob, kinds=tuple(args.known_kinds), max_frames=args.known_max_frames, seed=args.known_seed)


def make_dataset(args, model=None):
    """(dataset, prep): prep is None for the host loaders, whose items are finished videos, a video_store.DevicePrep for --packed and a
    video_store.DeviceLatentPrep for --packed --latents (which needs `model`: the store must be its LFAE's)."""
    if args.latents:
        from cvpr23_lfdm_amd.video_store import DeviceLatentPrep, PackedLatents
        if not args.packed:
            sys.exit("--latents reads the latent store beside a packed frame store: give --packed DIR")
        ds = PackedLatents(args.packed, image_size=args.size, num_frames=args.frames, sampling="random", jitter=True, resident=args.resident,
                           model=model)
        return ds, DeviceLatentPrep(ds)
    if args.packed:
        from cvpr23_lfdm_amd.video_store import DevicePrep, PackedVideos
        ds = PackedVideos(args.packed, image_size=args.size, num_frames=args.frames, sampling="random", jitter=True, resident=args.resident)
        return ds, DevicePrep(ds)
    ds = SyntheticVideos(n=256, image_size=args.size, num_frames=args.frames) if args.synthetic else \
        FrameFolderVideos(args.data, image_size=args.size, num_frames=args.frames, sampling="random", jitter=True)
    return ds, None


def _emulated():
    """True under the test suite's x86 emulation build of the kernels (tests only: the loop then runs on CPU tensors)."""
    from cvpr23_lfdm_amd import _native
    return _native._active is not None and _native._active.kind == "emu"


def build_model(args, cuda=True, **extra):
    """The training model of the options (`extra`: further FlowDiffusion keywords), on the GPU; --synthetic: a text encoder of random
    embeddings and the random-init LFAE frozen."""
    if args.schedule == "cosine_zsnr" and args.objective == "pred_noise":
        sys.exit("--schedule cosine_zsnr needs --objective pred_v or pred_x0: the noise prediction carries no information at SNR 0")
    model = FlowDiffusion(lr=args.lr, is_train=True, img_size=args.size // 4, num_frames=args.frames,
                          null_cond_prob=args.null_cond_prob, sampling_timesteps=args.preview_steps or 1000, config_pth=args.config,
                          pretrained_pth=args.lfae_ckpt, bert_path=None if args.synthetic else args.bert,     # :153-162
                          ema_decay=args.ema_decay, ema_start_step=args.ema_start_step, max_grad_norm=args.max_grad_norm,
                          skip_nonfinite=args.skip_nonfinite, long_attention=args.long_attention, known_train=known_train(args),
                          dim_mults=tuple(args.dim_mults), objective=args.objective, min_snr_gamma=args.min_snr_gamma,
                          schedule=args.schedule, **extra)
    if cuda:
        model.cuda()
    if args.synthetic:
        emb = {}
        model.diffusion.text_encoder = lambda texts: torch.stack(
            [emb.setdefault(t, torch.randn(768, generator=torch.Generator().manual_seed(len(emb) + 1))) for t in texts])
        for net in (model.generator, model.region_predictor, model.bg_predictor):
            net.eval()
            model.set_requires_grad(net, False)
    return model


def feed(model, args, prep, batch):
    """One loader batch as the model's training input; -> (ref_imgs, real_vids | None under --latents, ref_texts, real_names)."""
    if args.latents:                 # the stored latent and the reference frame: no video, no LFAE pass
        (latents, ref_imgs), ref_texts, real_names, real_vids = prep(batch), batch[5], batch[6], None
        model.set_train_latent(ref_img=ref_imgs, latent=latents, ref_text=list(ref_texts))
    else:
        if prep is None:
            real_vids, ref_texts, real_names = batch
            real_vids = real_vids.cuda(non_blocking=True)
        else:
            real_vids, ref_texts, real_names = prep(batch), batch[3], batch[4]
        ref_imgs = real_vids[:, :, 0].clone().detach()                    # first frame = reference frame (:221)
        model.set_train_input(ref_img=ref_imgs, real_vid=real_vids, ref_text=list(ref_texts))
    return ref_imgs, real_vids, ref_texts, real_names


def checkpoint(model, args, step, world, **extra):
    """The checkpoint of a step: the reference's three entries, what the model was trained as, the averaged weights where there are any."""
    ck = {"example": step * args.batch_size * world, "diffusion": model.diffusion.state_dict(),
          "optimizer_diff": model.optimizer_diff.state_dict(), "objective": args.objective, "min_snr_gamma": args.min_snr_gamma,
          "schedule": args.schedule}
    ck.update(extra)
    if args.ema_decay is not None:          # the averaged weights, shaped like "diffusion" (tools/demo.py --use-ema)
        ck["diffusion_ema"] = model.ema_state_dict()
    return ck


def main(argv=None):
    args = parse_args(argv)
    cuda = not _emulated()
    if cuda and not torch.cuda.is_available():
        sys.exit("tools/train_dm.py needs a GPU: the training step is liblfdm_hip.so only")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if cuda:
        torch.cuda.set_device(local % torch.cuda.device_count())
    if world > 1:
        dist.init_process_group("nccl")                      # RCCL
    # every rank must build the SAME initial UNet (parameters are initialised from torch's global generator and the
    # data-parallel step only averages gradients): common seed for construction, per-rank streams afterwards
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    os.makedirs(args.out, exist_ok=True)

    model = build_model(args, cuda)
    quartiles = None
    if args.log_loss_quartiles:
        if args.objective == "pred_noise" and args.min_snr_gamma is None:
            sys.exit("--log-loss-quartiles reads the per-sample losses of the objective loss kernel: give --objective or --min-snr-gamma")
        quartiles = LossQuartiles(model.diffusion.num_timesteps)
    opt = model.optimizer_diff
    start_step = 0
    if args.restore_from:                                                                                     # :169-184
        ck = torch.load(args.restore_from, map_location="cpu")
        try:                                 # a run continues on the objective and the schedule its checkpoint was trained with
            C.checkpoint_objective(ck, args.objective, args.restore_from)
            C.checkpoint_schedule(ck, args.schedule, args.restore_from)
        except ValueError as e:
            sys.exit(str(e))
        if args.set_start:
            start_step = int(math.ceil(ck["example"] / (args.batch_size * world)))
        model.diffusion.load_state_dict(ck["diffusion"])
        if "optimizer_diff" in ck:
            model.optimizer_diff.load_state_dict(ck["optimizer_diff"])
        print("=> loaded checkpoint '%s' (step %d)" % (args.restore_from, start_step))
    if world > 1:
        # bucketed RCCL all-reduce of the flat gradient, overlapped with backward; rank 0's parameters and Adam
        # moments are broadcast once so the replicas start identical whatever happened above (restore on one rank ...)
        model.enable_data_parallel(shard_inputs=False)      # the DistributedSampler below already feeds rank-local batches
    torch.manual_seed(args.seed + 1 + rank)     # per-rank streams for t / noise / null-cond mask / data order
    np.random.seed(args.seed + 1 + rank)

    ds, prep = make_dataset(args, model)
    sampler = data.distributed.DistributedSampler(ds, world, rank, shuffle=True, seed=args.seed) if world > 1 else None
    loader = data.DataLoader(ds, batch_size=args.batch_size, shuffle=sampler is None, sampler=sampler,
                             num_workers=args.num_workers, pin_memory=cuda, drop_last=True)
    per_epoch = max(1, len(loader))
    epoch = start_step // per_epoch
    sched = MultiStepLR(model.optimizer_diff, args.epoch_milestones, gamma=0.1, last_epoch=epoch - 1)         # :210-211
    step, t0 = start_step, timeit.default_timer()
    while step < args.final_step:
        if sampler is not None:
            sampler.set_epoch(epoch)
        for batch in loader:
            ref_imgs, real_vids, ref_texts, real_names = feed(model, args, prep, batch)
            model.optimize_parameters()
            step += 1
            if quartiles is not None:
                quartiles.add(model.diffusion.sample_loss, model.diffusion.sample_t)
            if args.latents and rank == 0 and step % args.save_img_freq == 0:
                real_vids = prep.real_frames(batch)          # the batch's frames from the rows it holds, for the panel and the two logged numbers
                model.decode_step_logs(real_vids)
            if rank == 0 and step % args.print_freq == 0:
                dt = (timeit.default_timer() - t0) / args.print_freq
                t0 = timeit.default_timer()
                guard = ""                       # the device plan is read back HERE only (print frequency), never in the step
                if opt.last_grad_norm() is not None:
                    guard = "  grad_norm %.4g  skipped %d" % (opt.last_grad_norm(), opt.skipped_steps())
                rec = [float("nan") if v is None else float(v) for v in (model.rec_loss, model.rec_warp_loss)]      # (--latents: nan between --save-img-freq hits)
                print("iter %d/%d  loss %.7f  loss_rec %.4f  loss_warp %.4f  lr %.2e  %.1f videos/s%s" % (
                    step, args.final_step, float(model.loss), rec[0], rec[1],
                    opt.param_groups[0]["lr"], args.batch_size * world / dt, guard), flush=True)
                if quartiles is not None:
                    print("    loss by quartile of t (unweighted): %s" % "  ".join("%.5f" % v for v in quartiles.means()), flush=True)
            if rank == 0 and step % args.save_img_freq == 0:                   # the middle-frame panel of :246-275
                mid, s = args.frames // 2, args.size
                panel = np.zeros((2 * s, 4 * s, 3), np.uint8)
                for col, (top, bot) in enumerate([(ref_imgs, real_vids[:, :, mid]), (model.real_out_vid[:, :, mid], model.real_warped_vid[:, :, mid]),
                                                  (model.fake_out_vid[:, :, mid], model.fake_warped_vid[:, :, mid])]):
                    panel[:s, col * s:(col + 1) * s] = C.sample_img(top)
                    panel[s:, col * s:(col + 1) * s] = C.sample_img(bot)
                panel[:s, 3 * s:] = C.grid2fig(model.real_vid_grid[0, :, mid].permute(1, 2, 0).data.cpu().numpy(), grid_size=s // 4, img_size=s)
                panel[s:, 3 * s:] = C.grid2fig(model.fake_vid_grid[0, :, mid].permute(1, 2, 0).data.cpu().numpy(), grid_size=s // 4, img_size=s)
                C.imsave(os.path.join(args.out, "B%04d_S%06d_%s.png" % (args.batch_size, step, real_names[0])), panel)
                if args.preview_steps > 0:                                      # a sampled preview, from the averaged weights when there are any
                    with (model.ema_weights() if args.ema_decay is not None else contextlib.nullcontext()):
                        model.set_sample_input(sample_img=ref_imgs[:1], sample_text=list(ref_texts)[:1])
                        pkw = {}
                        if args.known_prob > 0:         # what the run is learning: the first frames of the video's own latent, held clean
                            with torch.no_grad():
                                latent = model.encode_video(real_vids[:1], ref_imgs[:1])
                            first = torch.zeros((1, args.frames), dtype=torch.bool, device=latent.device)
                            first[:, :max(1, args.known_max_frames // 2)] = True
                            pkw = dict(known_latent=latent, known_mask=first, known_level="clean")
                        model.sample_one_video(cond_scale=1.0, **pkw)
                    C.mimsave(os.path.join(args.out, "B%04d_S%06d_%s%s.gif" % (args.batch_size, step, real_names[0],
                                                                                "_ema" if args.ema_decay is not None else "")),
                              C.video_strip(model, ref_imgs[:1]))
            if rank == 0 and (step % args.save_freq == 0 or step >= args.final_step):                         # :330-340
                torch.save(checkpoint(model, args, step, world),
                           os.path.join(args.out, "flowdiff_%04d_S%06d.pth" % (args.batch_size, step)))
            if step >= args.final_step:
                break
        epoch += 1
        sched.step()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
