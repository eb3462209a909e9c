"""Optimizer + data-parallel gradient exchange of the DM training step.

`FlatAdam` is a real `torch.optim.Optimizer` (the training scripts call `.state_dict()`, `.load_state_dict()`,
`.param_groups[0]['lr']` and wrap it in `MultiStepLR`: DM/train_video_flow_diffusion_mug.py:181,210-211,367) whose
step is ONE fused HIP launch (lfdm_adam_step_f32) over flat fp32 buffers: parameters, gradients and both moments
live contiguously, each tensor being a view.  The same flat gradient buffer is what `GradAllReduce` hands to RCCL -
bucketed sum all-reduce over xGMI launched from autograd hooks while backward is still running; the 1/world of the
mean is folded into the Adam kernel.  (Reference multi-GPU: nn.DataParallel threads + NCCL reduce to GPU 0,
SURVEY.md 3.4; here: one process per GPU, every rank applies the identical update, no parameter broadcast.)

Opt-in: an exponential moving average of the weights, global-norm gradient clipping and a guard that skips
a step whose gradient is not finite.  With any of them on the step is the GUARDED one - a sum-of-squares pass over the flat
gradient, a one-workgroup plan kernel and a fused Adam + EMA update that reads clip coefficient, skip-or-apply, bias
corrections and EMA decay from device memory - and the authoritative step counter lives on the device: `step()` never
synchronises.
"""
import contextlib

import torch

from ._native import OPTIM_PLAN_BYTES
from .ops import _chk, _lib, _p, _stream
from .params import bump_weights_epoch


class FlatAdam(torch.optim.Optimizer):
    """torch.optim.Adam semantics over flat buffers.  Options (all off by default: the step is then the single
    lfdm_adam_step_f32 launch):
      ema_decay       d in [0, 1): a fifth flat buffer `ema` (same offsets as the parameters, initialised from them) takes
                      ema = d * ema + (1 - d) * p_new in the update pass; every slice is state[p]["ema"], so state_dict() /
                      load_state_dict() carry it (a state without "ema" loads: the average restarts from the parameters).
      ema_start_step  applied steps 1 .. ema_start_step leave ema == p exactly (decay 0).
      max_grad_norm   torch.nn.utils.clip_grad_norm_(params, max_grad_norm) semantics on the averaged gradient, before weight
                      decay.  The flat gradient buffer is NOT modified: p.grad keeps showing the unclipped gradient.
      skip_nonfinite  a step whose gradient norm is inf / nan (one such element anywhere, or a sum of squares beyond fp32)
                      changes nothing: parameters, moments, ema and the step counter stay as they were; skipped_steps() counts it.
    last_grad_norm() / skipped_steps() read the device plan back (a synchronisation: use them at print frequency)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, ema_decay=None, ema_start_step=0,
                 max_grad_norm=None, skip_nonfinite=False):
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError("FlatAdam: ema_decay must lie in [0, 1), got %r" % (ema_decay,))
        if int(ema_start_step) < 0:
            raise ValueError("FlatAdam: ema_start_step must be >= 0, got %r" % (ema_start_step,))
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("FlatAdam: max_grad_norm must be positive, got %r" % (max_grad_norm,))
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._flat = None            # per group: dict(params, offs, p, g, m, v, gviews[, ema, plan, partials])
        self._staged = False         # gradients already gathered into the flat buffer (GradAllReduce.finish)
        self.grad_scale = 1.0        # GradAllReduce sets 1/world
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_start_step = int(ema_start_step)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.ema_decay is not None or self.max_grad_norm is not None or self.skip_nonfinite
        if self.guarded and len(self.param_groups) != 1:
            raise ValueError("FlatAdam: ema_decay / max_grad_norm / skip_nonfinite need ONE parameter group (the norm is global)")
        self._ema_live = False       # inside ema_weights(): the parameters point at the ema slices

    # ------------------------------------------------------------------ flat storage
    def _build(self):
        skipped = 0
        if self.guarded and self._flat is not None:       # a rebuild (parameters moved): the device counters move along
            steps, skipped = self._flat[0]["plan"].view(torch.int64)[4:6].tolist()
            for p in self._flat[0]["params"]:
                self.state[p]["step"] = torch.tensor(float(steps))
        flats = []
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.requires_grad]
            dev, n = ps[0].device, 0
            offs = []
            for p in ps:
                offs.append(n)
                n += (p.numel() + 3) // 4 * 4          # keep every view 16-byte aligned
            fp = torch.zeros(n, dtype=torch.float32, device=dev)
            fg = torch.zeros_like(fp)
            fm = torch.zeros_like(fp)
            fv = torch.zeros_like(fp)
            gviews = []
            for pi, (p, o) in enumerate(zip(ps, offs)):
                k = p.numel()
                fp[o:o + k].copy_(p.data.reshape(-1))
                p.data = fp[o:o + k].view(p.shape)
                gviews.append(fg[o:o + k].view(p.shape))
                # autograd.grad_out: the native backward kernels write the step's first gradient of `p` straight into this slot
                p._lfdm_grad_slot, p._lfdm_grad_slot_busy = gviews[-1], False
                st = self.state[p]
                if "exp_avg" in st:                    # state loaded before the first step
                    if st["exp_avg"].numel() != k or st["exp_avg_sq"].numel() != k:
                        raise ValueError("FlatAdam.load_state_dict: the moment of parameter #%d has %d elements, the parameter %s has %d - "
                                         "the state was saved for a different parameter ORDER (torch indexes optimizer state by "
                                         "position: it must come from a model with the same registration order)"
                                         % (pi, st["exp_avg"].numel(), tuple(p.shape), k))
                    fm[o:o + k].copy_(st["exp_avg"].reshape(-1))
                    fv[o:o + k].copy_(st["exp_avg_sq"].reshape(-1))
                st.setdefault("step", torch.tensor(0.0))
                st["exp_avg"] = fm[o:o + k].view(p.shape)
                st["exp_avg_sq"] = fv[o:o + k].view(p.shape)
            fl = dict(params=ps, offs=offs, p=fp, g=fg, m=fm, v=fv, gviews=gviews)
            if self.guarded:
                self._build_guarded(fl, skipped)
            flats.append(fl)
        self._flat = flats
        self._staged = False

    def _build_guarded(self, fl, skipped=0):
        """The guarded step's device state: the plan (its counter starts at the loaded step), the norm partials, the average."""
        lib = _lib()
        fp, ps, offs = fl["p"], fl["params"], fl["offs"]
        plan = torch.zeros(OPTIM_PLAN_BYTES // 4, dtype=torch.int32, device=fp.device)
        plan.view(torch.int64)[4] = int(self.state[ps[0]]["step"])          # lfdm_optim_plan.applied_steps
        plan.view(torch.int64)[5] = int(skipped)                            # .skipped_steps
        fl["plan"] = plan
        if self.max_grad_norm is not None or self.skip_nonfinite:
            fl["partials"] = torch.zeros(lib.lfdm_grad_sumsq_ws_bytes(fp.numel()) // 4, dtype=torch.float32, device=fp.device)
        if self.ema_decay is None:
            for p in ps:
                self.state[p].pop("ema", None)
            return
        fe = fp.clone()                                                      # no saved average: it starts from the parameters
        for pi, (p, o) in enumerate(zip(ps, offs)):
            k, st = p.numel(), self.state[p]
            if "ema" in st:
                if st["ema"].numel() != k:
                    raise ValueError("FlatAdam.load_state_dict: the average of parameter #%d has %d elements, the parameter %s has %d"
                                     % (pi, st["ema"].numel(), tuple(p.shape), k))
                fe[o:o + k].copy_(st["ema"].reshape(-1))
            st["ema"] = fe[o:o + k].view(p.shape)
        fl["ema"] = fe

    def _valid(self):
        if self._flat is None:
            return False
        if self._ema_live:               # the parameters are deliberately elsewhere (ema_weights); step() refuses to run
            return True
        for fl in self._flat:
            base = fl["p"].data_ptr()
            for p, o in zip(fl["params"], fl["offs"]):
                if p.data_ptr() != base + 4 * o:
                    return False
        return True

    def ensure_flat(self):
        """(Re)build the flat buffers if parameters were moved / replaced (e.g. `.cuda()` after construction)."""
        if not self._valid():
            self._build()
        return self._flat

    def flat_grads(self):
        return [fl["g"] for fl in self.ensure_flat()]

    def zero_grad(self, set_to_none=True):
        """torch semantics.  With set_to_none (the default, what the training scripts get) autograd hands every parameter its
        gradient tensor as is - no `grad += new` kernel per parameter (302 of them per step when the gradients were kept as
        views of the flat buffer) - and `stage_grads` gathers them into the flat buffer with a few multi-tensor copies."""
        self._staged = False
        for fl in self.ensure_flat():
            for p in fl["params"]:
                p._lfdm_grad_slot_busy = False
            if set_to_none:
                for p in fl["params"]:
                    p.grad = None
            else:
                gs = [p.grad for p in fl["params"] if p.grad is not None]
                if gs:
                    torch._foreach_zero_(gs)

    @torch.no_grad()
    def stage_grads(self, fl=None, idxs=None):
        """Gather p.grad of the given parameters (default: all) into their slots of the flat gradient buffer and re-point
        p.grad at the slot (so p.grad shows what the update / the all-reduce sees; a backward without zero_grad then
        accumulates in place).  Parameters without a gradient this step get a zero slot."""
        todo = [(f, range(len(f["params"]))) for f in self.ensure_flat()] if fl is None else [(fl, idxs)]
        for f, ids in todo:
            src, dst = [], []
            for i in ids:
                p, slot = f["params"][i], f["gviews"][i]
                g = p.grad
                if g is None:
                    slot.zero_()
                elif g.data_ptr() != slot.data_ptr():
                    src.append(g if g.shape == slot.shape else g.reshape(slot.shape))
                    dst.append(slot)
                p.grad = slot
                p._lfdm_grad_slot_busy = False
            if dst:
                torch._foreach_copy_(dst, src)
        if fl is None:
            self._staged = True

    def load_state_dict(self, state_dict):
        if self._ema_live:
            raise RuntimeError("FlatAdam.load_state_dict inside ema_weights(): the parameters are the averaged ones")
        super().load_state_dict(state_dict)
        self._flat = None             # loaded moments (and average, and step count) are folded into fresh flat buffers at the next step

    def _plan(self):
        return self.ensure_flat()[0]["plan"]

    def applied_steps(self):
        """Steps applied so far (skipped ones not counted).  Guarded: read back from the device."""
        if self.guarded:
            return int(self._plan().view(torch.int64)[4].item())
        fl = self.ensure_flat()[0]
        return int(self.state[fl["params"][0]]["step"])

    def skipped_steps(self):
        """Steps the non-finite guard dropped since this optimizer's buffers were built (read back from the device)."""
        return int(self._plan().view(torch.int64)[5].item()) if self.guarded else 0

    def last_grad_norm(self):
        """Global norm of the averaged gradient of the latest step, before clipping (read back from the device); None when
        neither clipping nor the guard is on - no norm pass runs then."""
        if self.max_grad_norm is None and not self.skip_nonfinite:
            return None
        return float(self._plan().view(torch.float32)[3].item())

    @torch.no_grad()
    def reset_moments(self):
        """Adam starts again on the current parameters (a new round of progressive distillation): both moments and the step count back
        to zero, the average - where one is kept - restarted from the parameters.  Learning rate, options and skipped_steps() stay."""
        if self._ema_live:
            raise RuntimeError("FlatAdam.reset_moments inside ema_weights(): the parameters are the averaged ones")
        for fl in self.ensure_flat():
            fl["m"].zero_()
            fl["v"].zero_()
            for p in fl["params"]:
                self.state[p]["step"] = torch.tensor(0.0)
            if "ema" in fl:
                fl["ema"].copy_(fl["p"])
            if "plan" in fl:
                fl["plan"].view(torch.int64)[4] = 0          # lfdm_optim_plan.applied_steps

    def state_dict(self):
        if self.guarded and self._flat is not None:      # the device counter is the authoritative one: the only read-back is here
            step = float(self.applied_steps())
            for fl in self._flat:
                for p in fl["params"]:
                    self.state[p]["step"] = torch.tensor(step)
        return super().state_dict()

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside: every parameter's storage is its slice of the averaged buffer (no copy); step() raises.  The caller bumps
        whatever caches depend on the weights (FlowDiffusion.ema_weights does).  Restored on exit, also on an exception."""
        if self.ema_decay is None:
            raise RuntimeError("ema_weights(): this optimizer keeps no average (ema_decay=None)")
        if self._ema_live:
            raise RuntimeError("ema_weights() is not re-entrant")
        fl = self.ensure_flat()[0]
        raw = [p.data for p in fl["params"]]
        self._ema_live = True
        try:
            for p in fl["params"]:
                p.data = self.state[p]["ema"]
            bump_weights_epoch()
            yield self
        finally:
            for p, d in zip(fl["params"], raw):
                p.data = d
            self._ema_live = False
            bump_weights_epoch()

    # ------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._ema_live:
            raise RuntimeError("FlatAdam.step() inside ema_weights(): the parameters are the averaged ones - leave the context first")
        lib = _lib()
        self.ensure_flat()
        if not self._staged:
            self.stage_grads()
        self._staged = False
        if self.guarded:
            self._guarded_step(lib)
            bump_weights_epoch()
            return loss
        for group, fl in zip(self.param_groups, self.ensure_flat()):
            st0 = self.state[fl["params"][0]]
            step = int(st0["step"]) + 1
            for p in fl["params"]:
                self.state[p]["step"] = torch.tensor(float(step))
            _chk(lib, fl["p"], fl["g"], fl["m"], fl["v"])
            b1, b2 = group["betas"]
            lib.check(lib.lfdm_adam_step_f32(_p(fl["p"]), _p(fl["g"]), _p(fl["m"]), _p(fl["v"]), fl["p"].numel(),
                                             float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                             float(group["weight_decay"]), step, float(self.grad_scale), _stream(lib)),
                      "lfdm_adam_step_f32")
        bump_weights_epoch()      # the kernel wrote the parameters behind torch's back: packed weight caches must rebuild
        return loss

    def _guarded_step(self, lib):
        """Norm partials (only with clipping / the guard) -> plan -> fused update, all on the current stream, no read-back."""
        group, fl = self.param_groups[0], self._flat[0]
        n, parts, ema = fl["p"].numel(), fl.get("partials"), fl.get("ema")
        _chk(lib, fl["p"], fl["g"], fl["m"], fl["v"], ema, parts)
        b1, b2 = group["betas"]
        stream = _stream(lib)
        if parts is not None:
            lib.check(lib.lfdm_grad_sumsq_f32(_p(fl["g"]), n, _p(parts), parts.numel() * 4, stream), "lfdm_grad_sumsq_f32")
        lib.check(lib.lfdm_optim_plan_f32(_p(parts), 0 if parts is None else parts.numel(), _p(fl["plan"]), fl["plan"].numel() * 4,
                                          float(self.grad_scale), -1.0 if self.max_grad_norm is None else self.max_grad_norm,
                                          int(self.skip_nonfinite), float(b1), float(b2),
                                          -1.0 if self.ema_decay is None else self.ema_decay, self.ema_start_step, stream),
                  "lfdm_optim_plan_f32")
        lib.check(lib.lfdm_adam_guarded_step_f32(_p(fl["p"]), _p(fl["g"]), _p(fl["m"]), _p(fl["v"]), _p(ema), n, float(group["lr"]),
                                                 float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                                                 float(self.grad_scale), _p(fl["plan"]), stream), "lfdm_adam_guarded_step_f32")


class GradAllReduce:
    """Sum all-reduce of FlatAdam's gradient buffer across ranks (torch.distributed; backend "nccl" = RCCL over xGMI
    on the GPU box, "gloo" in CPU tests).  Buckets are contiguous slices of the flat buffer, walked from the END
    (the last layers finish their gradients first); a bucket becomes READY in the autograd hook of the last of its
    parameters, so the exchange overlaps the remaining backward.  Collectives are issued STRICTLY IN BUCKET-LIST ORDER on
    every rank: a ready bucket is launched only once all buckets before it have been launched (RCCL / gloo match
    collectives by issue order and the buckets differ in size - a rank whose hooks fire in another order, or a rank with
    an empty shard that launches everything from `finish()`, must not permute them).  `finish()` launches what is left
    (parameters without gradient this step, an empty shard) in the same order and waits for all buckets."""

    def __init__(self, optimizer, bucket_bytes=64 << 20, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.opt = optimizer
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        optimizer.grad_scale = 1.0 / self.world
        self.bucket_elems = max(bucket_bytes // 4, 1)
        self._hooks = []
        self._buckets = None
        self._flat_id = None
        self._next = 0
        self.launch_order = []
        # profile = True: finish() brackets its waits with events on the compute stream; exposed_ms() then reports how long the
        # compute stream stood still for the exchange per step (the part of the all-reduce NOT hidden under backward)
        self.profile = False
        self._wait_events = []

    def sync_replicas(self, src=0):
        """Broadcast rank `src`'s flat parameter buffer and Adam moments (one collective each per group) so that the
        replicas start from identical state whatever seeds / restores happened before; afterwards identical averaged
        gradients keep them identical (checked by `replica_checksum`).  The reference's nn.DataParallel re-broadcasts
        the weights from GPU 0 on every forward (DM/train_video_flow_diffusion_mhad_multiGPU.py:207) - here once."""
        if self.world <= 1:
            return
        for group, fl in zip(self.opt.param_groups, self.opt.ensure_flat()):
            for key in ("p", "m", "v") + (("ema",) if "ema" in fl else ()):
                self.dist.broadcast(fl[key], src=src, group=self.group)
            if "plan" in fl:                          # guarded: the device plan carries the counters (applied / skipped steps)
                self.dist.broadcast(fl["plan"], src=src, group=self.group)
            step = torch.tensor([float(self.opt.state[fl["params"][0]]["step"])], device=fl["p"].device)
            self.dist.broadcast(step, src=src, group=self.group)
            for p in fl["params"]:
                self.opt.state[p]["step"] = torch.tensor(float(step.item()))
        bump_weights_epoch()

    def replica_checksum(self):
        """(max - min) over ranks of the fp64 sum of the flat parameter buffer: 0.0 iff the replicas agree.  With an average
        (FlatAdam ema_decay) the same for the `ema` buffer, and the larger of the two is returned."""
        flats = self.opt.ensure_flat()
        tot = [torch.stack([fl["p"].double().sum() for fl in flats]).sum()]
        if all("ema" in fl for fl in flats):
            tot.append(torch.stack([fl["ema"].double().sum() for fl in flats]).sum())
        tot = torch.stack(tot)
        if self.world <= 1:
            return 0.0
        hi, lo = tot.clone(), tot.clone()
        self.dist.all_reduce(hi, op=self.dist.ReduceOp.MAX, group=self.group)
        self.dist.all_reduce(lo, op=self.dist.ReduceOp.MIN, group=self.group)
        return float((hi - lo).max().item())

    def _setup(self):
        flats = self.opt.ensure_flat()
        if self._flat_id == id(flats):
            return
        for h in self._hooks:
            h.remove()
        self._hooks, self._buckets = [], []
        for fl in flats:
            n = fl["p"].numel()
            ends = list(fl["offs"][1:]) + [n]
            # buckets from the end of the buffer
            cur_hi, members = n, []
            items = list(zip(range(len(fl["params"])), fl["params"], fl["offs"], ends))
            idxs = []
            for i, p, lo, hi in reversed(items):
                members.append(p)
                idxs.append(i)
                if cur_hi - lo >= self.bucket_elems or lo == 0:
                    self._buckets.append(dict(view=fl["g"][lo:cur_hi], params=members, fl=fl, idxs=idxs, pending=0, handle=None,
                                              staged=False))
                    cur_hi, members, idxs = lo, [], []
        for bi, b in enumerate(self._buckets):
            for p in b["params"]:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._make_hook(bi)))
        self._flat_id = id(flats)

    def _make_hook(self, bi):
        def hook(_param):
            b = self._buckets[bi]
            b["pending"] -= 1
            if b["pending"] == 0:
                self._stage(b)                    # copy now (overlaps backward) ...
                b["ready"] = True
                self._launch_ready()              # ... launch as soon as every earlier bucket has been launched
        return hook

    def _stage(self, b):
        if not b["staged"]:                       # the bucket's gradients -> its slice of the flat buffer (one multi-tensor copy)
            self.opt.stage_grads(b["fl"], b["idxs"])
            b["staged"] = True

    def _launch_ready(self, force=False):
        """Issue the all-reduces of the leading run of ready buckets (all remaining ones with force=True), in list order."""
        while self._next < len(self._buckets):
            b = self._buckets[self._next]
            if not (b["ready"] or force):
                return
            self._stage(b)
            if self.world > 1 and b["handle"] is None:
                b["handle"] = self.dist.all_reduce(b["view"], op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
            self.launch_order.append(self._next)
            self._next += 1

    def prepare(self):
        """Call before backward (after zero_grad)."""
        self._setup()
        for b in self._buckets:
            b["pending"] = len(b["params"])
            b["handle"] = None
            b["staged"] = False
            b["ready"] = False
        self._next = 0
        self.launch_order = []                    # bucket indices in the order their collectives were issued (tests)

    def finish(self):
        """Call after backward, before optimizer.step()."""
        self._launch_ready(force=True)
        timed = self.profile and self.world > 1 and torch.cuda.is_available() and self._buckets and self._buckets[0]["view"].is_cuda
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        for b in self._buckets:
            if b["handle"] is not None:
                b["handle"].wait()
                b["handle"] = None
        if timed:
            e1.record()
            self._wait_events.append((e0, e1))
        self.opt._staged = True

    def describe(self):
        """Bucket layout of the exchange: count and bytes (after the first prepare())."""
        if not self._buckets:
            return {"buckets": 0, "bytes": []}
        return {"buckets": len(self._buckets), "bytes": [int(b["view"].numel()) * 4 for b in self._buckets]}

    def exposed_ms(self, last=None):
        """Per-step milliseconds the compute stream waited in finish() (profile = True), newest `last` steps."""
        ev = self._wait_events[-last:] if last else self._wait_events
        if not ev:
            return None
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in ev]
