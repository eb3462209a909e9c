#!/usr/bin/env python
"""Progressive distillation of a trained DM (Salimans & Ho 2022): rounds --start-steps -> --start-steps / 2 -> ... ->
--end-steps.  In each round the current weights are frozen as the teacher and the student - starting from them - is trained so that ONE
DDIM step on the "trailing" grid lands where TWO steps of the teacher land; the optimizer's moments are reset at each round, as in the
paper.  One checkpoint per round, `distilled_%04d_N%03d.pth`, in tools/train_dm.py's format with "distilled_steps": N beside "objective" and
"schedule": tools/demo.py and tools/eval.py then sample it with N steps on the trailing grid at eta = 0 without further flags.  Data,
optimizer and EMA plumbing are tools/train_dm.py's (its options apply: --packed OUT --latents --resident, --ema-decay, --max-grad-norm ...).

    python tools/distill_dm.py --restore-from flowdiff.pth --packed PACKED --latents --resident --start-steps 64 --end-steps 4 \\
        --iters-per-round 5000 --ema-decay 0.999 [--teacher-cond-scale 2.0 --teacher-guidance-rescale 0.7] [--distill-weight truncated_snr]
    python tools/distill_dm.py --synthetic --size 64 --frames 4 --dim-mults 1 2 --batch-size 2 --start-steps 4 --end-steps 1 \\
        --iters-per-round 2          # random videos, random-init LFAE and teacher: two rounds of the loop, no data

The student is trained on the conditional teacher only (--null-cond-prob defaults to 0 here): its null-condition branch is no longer
trained, so a distilled checkpoint CANNOT be guided at sampling (sample it at cond_scale 1).  Guidance has to be folded in while
distilling: --teacher-cond-scale W makes every teacher output the guided one.  A non-zero --null-cond-prob would train the null branch
towards the conditional teacher and is not what anybody wants.

The checkpoint must be a "pred_v" or "pred_x0" model (the noise objective cannot be distilled: DESIGN.md 4.16).  No checkpoint has been
distilled with this tool yet and the quality of its students is not evaluated.
"""
import os
import sys
import timeit

import numpy as np
import torch
from torch.utils import data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import train_dm as T  # noqa: E402
from cvpr23_lfdm_amd import io_compat as C  # noqa: E402


def parse_args(argv=None):
    ap = T.build_parser(__doc__)
    ap.add_argument("--start-steps", type=int, default=64, help="student steps of the first round (its teacher takes twice as many)")
    ap.add_argument("--end-steps", type=int, default=4, help="student steps of the last round")
    ap.add_argument("--iters-per-round", type=int, default=5000, help="optimizer steps per round")
    ap.add_argument("--teacher-cond-scale", type=float, default=1.0, help="!= 1: the teacher is evaluated under classifier-free guidance "
                    "of this scale (two passes) and the guided model is folded into a student that is sampled at cond_scale 1; with 1 "
                    "(default) the student is the unguided conditional model - either way it can no longer be guided at sampling")
    ap.add_argument("--teacher-guidance-rescale", type=float, default=0.0, help="guidance rescale of the guided teacher (DESIGN.md 4.15)")
    ap.add_argument("--distill-weight", choices=("truncated_snr", "min_snr", "none"), default="truncated_snr",
                    help="loss weight per timestep: max(snr, 1) on the x0 error (default, the paper's), the model's min-SNR weight, or 1")
    # --null-cond-prob defaults to 0 here: the teacher always sees the condition, so a student whose condition is dropped would learn the
    # CONDITIONAL target on its null branch
    ap.set_defaults(objective="pred_v", null_cond_prob=0.0)
    return ap.parse_args(argv)


def round_steps(start, end):
    """[start, start / 2, ..., end]: both powers-of-two multiples of each other."""
    if end < 1 or start < end or (start // end) * end != start or ((start // end) & (start // end - 1)) != 0:
        sys.exit("--start-steps must be --end-steps times a power of two (64 -> 32 -> ... -> 4), got %d and %d" % (start, end))
    steps = [start]
    while steps[-1] > end:
        steps.append(steps[-1] // 2)
    return steps


def main(argv=None):
    args = parse_args(argv)
    cuda = not T._emulated()
    if cuda and not torch.cuda.is_available():
        sys.exit("tools/distill_dm.py needs a GPU: the training step is liblfdm_hip.so only")
    if not args.synthetic and not args.restore_from:
        sys.exit("give --restore-from CHECKPOINT: the model to distil (or --synthetic for a run of the loop on random weights)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit("tools/distill_dm.py runs one process (FlowDiffusion.begin_distill_round itself composes with enable_data_parallel)")
    steps = round_steps(args.start_steps, args.end_steps)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    os.makedirs(args.out, exist_ok=True)
    ck = None
    if args.restore_from:
        ck = torch.load(args.restore_from, map_location="cpu")
        try:                                 # distilled on the objective and the schedule the checkpoint was trained with
            args.objective = C.checkpoint_objective(ck, None, args.restore_from)
            args.schedule = C.checkpoint_schedule(ck, None, args.restore_from)
        except ValueError as e:
            sys.exit(str(e))
        if C.checkpoint_distilled_steps(ck) not in (None, 2 * steps[0]):
            print("warning: %s was distilled to %d steps; the first round's teacher takes %d" % (args.restore_from, ck["distilled_steps"],
                                                                                                2 * steps[0]))
    model = T.build_model(args, cuda, step_grid="trailing")
    if ck is not None:
        model.diffusion.load_state_dict(ck["diffusion_ema" if "diffusion_ema" in ck else "diffusion"])
        print("=> distilling '%s' (%s, %s%s)" % (args.restore_from, args.objective, args.schedule,
                                                 ", its averaged weights" if "diffusion_ema" in ck else ""))
    opt = model.optimizer_diff
    torch.manual_seed(args.seed + 1)
    np.random.seed(args.seed + 1)
    ds, prep = T.make_dataset(args, model)
    loader = data.DataLoader(ds, batch_size=args.batch_size, shuffle=True, num_workers=args.num_workers, pin_memory=cuda, drop_last=True)
    weight = None if args.distill_weight == "none" else args.distill_weight
    done = 0
    for n in steps:
        try:
            model.begin_distill_round(n, teacher_cond_scale=args.teacher_cond_scale, teacher_guidance_rescale=args.teacher_guidance_rescale,
                                      distill_weight=weight)
        except ValueError as e:          # (a "pred_noise" checkpoint, a step count the schedule does not hold: the message names the cure)
            sys.exit(str(e))
        opt.reset_moments()          # (the average, where one is kept, restarts from the round's first weights too)
        step, t0 = 0, timeit.default_timer()
        while step < args.iters_per_round:
            before = step
            for batch in loader:
                T.feed(model, args, prep, batch)
                model.optimize_parameters()
                step += 1
                if step % args.print_freq == 0 or step == args.iters_per_round:
                    dt = (timeit.default_timer() - t0) / max(1, step)
                    guard = "" if opt.last_grad_norm() is None else "  grad_norm %.4g  skipped %d" % (opt.last_grad_norm(), opt.skipped_steps())
                    print("round %d -> %d steps  iter %d/%d  loss %.7f  %.1f videos/s%s" % (2 * n, n, step, args.iters_per_round,
                                                                                           float(model.loss.detach()), args.batch_size / dt, guard), flush=True)
                if step >= args.iters_per_round:
                    break
            if step == before:
                sys.exit("the data set gives no batch of --batch-size %d (%d videos; incomplete batches are dropped)" % (args.batch_size, len(ds)))
        done += step
        path = os.path.join(args.out, "distilled_%04d_N%03d.pth" % (args.batch_size, n))
        torch.save(T.checkpoint(model, args, done, 1, distilled_steps=n, teacher_cond_scale=args.teacher_cond_scale), path)
        print("=> round %d -> %d steps done: %s" % (2 * n, n, path), flush=True)
    model.end_distill()


if __name__ == "__main__":
    main()
