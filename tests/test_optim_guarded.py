"""FlatAdam's opt-in guarded step: EMA of the weights, global-norm gradient clipping and the non-finite guard, decided on
the device by lfdm_grad_sumsq_f32 -> lfdm_optim_plan_f32 -> lfdm_adam_guarded_step_f32.  Every reference is torch itself
(torch.optim.Adam, torch.nn.utils.clip_grad_norm_, a two-line moving average); parameters, moments and the average are held to 1e-6,
the bar tests/test_optim.py holds plain Adam to: a relative error e of the norm moves the clipped gradient by e and Adam's update by at
most lr * e."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from cvpr23_lfdm_amd import _native
from cvpr23_lfdm_amd.optim import FlatAdam
from util import assert_close, rnd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 5), (13,), (4, 3, 3, 3), (1,), (64, 9)]


def _params(dev, seed=0):
    return [torch.nn.Parameter(rnd(*s, seed=seed + i).to(dev)) for i, s in enumerate(SHAPES)]


def _grads(it, dev, scale=1.0):
    return [(rnd(*s, seed=100 * it + i) * scale).to(dev) for i, s in enumerate(SHAPES)]


class TorchRef:
    """torch.optim.Adam + clip_grad_norm_ + `ema.mul_(d).add_(p, alpha=1 - d)` after every applied step (ema = p up to ema_start_step)."""

    def __init__(self, ps, ema_decay=None, ema_start_step=0, max_grad_norm=None, **adam):
        self.ps, self.opt = ps, torch.optim.Adam(ps, **adam)
        self.d, self.start, self.max_norm = ema_decay, ema_start_step, max_grad_norm
        self.ema = [p.detach().clone() for p in ps]
        self.applied, self.norms = 0, []

    def step(self, grads):
        for p, g in zip(self.ps, grads):
            p.grad = g.clone()
        if self.max_norm is not None:
            self.norms.append(float(torch.nn.utils.clip_grad_norm_(self.ps, self.max_norm)))
        else:
            self.norms.append(float(torch.linalg.vector_norm(torch.cat([g.reshape(-1) for g in grads]))))
        self.opt.step()
        self.applied += 1
        if self.d is not None:
            with torch.no_grad():
                for e, p in zip(self.ema, self.ps):
                    if self.applied <= self.start:
                        e.copy_(p)
                    else:
                        e.mul_(self.d).add_(p, alpha=1 - self.d)


def _step(opt, ps, grads):
    opt.zero_grad()
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    opt.step()


def _compare(a, pa, ref, what, ema=True):
    sa, sb = a.state_dict(), ref.opt.state_dict()
    for i, (x, y) in enumerate(zip(pa, ref.ps)):
        assert_close(x, y, 1e-6, what + ": params")
        assert_close(sa["state"][i]["exp_avg"], sb["state"][i]["exp_avg"], 1e-6, what + ": exp_avg")
        assert_close(sa["state"][i]["exp_avg_sq"], sb["state"][i]["exp_avg_sq"], 1e-6, what + ": exp_avg_sq")
        assert float(sa["state"][i]["step"]) == float(sb["state"][i]["step"]) == ref.applied
        if ema:
            assert_close(sa["state"][i]["ema"], ref.ema[i], 1e-6, what + ": ema")
            assert a.state[x]["ema"].shape == x.shape


def test_options_off_is_the_parent(backend):
    """Case 1: with every option at its default the step is the single lfdm_adam_step_f32 launch: bit-identical results."""
    dev = backend
    pa, pb = _params(dev), _params(dev)
    a = FlatAdam(pa, lr=2e-3, betas=(0.9, 0.99), weight_decay=0.01)
    b = FlatAdam(pb, lr=2e-3, betas=(0.9, 0.99), weight_decay=0.01, ema_decay=None, max_grad_norm=None, skip_nonfinite=False)
    assert not a.guarded and not b.guarded
    for it in range(4):
        _step(a, pa, _grads(it, dev))
        _step(b, pb, _grads(it, dev))
    assert "plan" not in b.ensure_flat()[0] and "ema" not in b.ensure_flat()[0]
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
        assert torch.equal(a.state[x]["exp_avg"], b.state[y]["exp_avg"]) and torch.equal(a.state[x]["exp_avg_sq"], b.state[y]["exp_avg_sq"])
        assert "ema" not in b.state[y]
    assert b.last_grad_norm() is None and b.skipped_steps() == 0 and b.applied_steps() == 4


def test_ema_alone(backend):
    """Case 2: six steps, ema_start_step=2 (the average equals the parameters through step 2, then decays)."""
    dev = backend
    pa, pb = _params(dev), _params(dev)
    a = FlatAdam(pa, lr=2e-3, betas=(0.9, 0.99), ema_decay=0.9, ema_start_step=2)
    ref = TorchRef(pb, lr=2e-3, betas=(0.9, 0.99), ema_decay=0.9, ema_start_step=2)
    assert "partials" not in a.ensure_flat()[0]                       # no norm pass when neither clipping nor the guard is on
    for it in range(6):
        g = _grads(it, dev)
        _step(a, pa, g)
        ref.step(g)
        if it == 1:
            for x in pa:
                assert torch.equal(a.state[x]["ema"], x.detach())      # before ema_start_step: exactly the parameters
    _compare(a, pa, ref, "ema alone")
    assert float((a.state[pa[0]]["ema"] - pa[0].detach()).abs().max()) > 1e-4   # ... afterwards a real average
    assert a.last_grad_norm() is None


def test_clipping_alone(backend):
    """Case 3: per-iteration gradient scales such that - by the torch reference's own norms - some iterations clip and some do not; weight
    decay pins the clip-before-decay order; the flat gradient (p.grad) is left unclipped."""
    dev = backend
    max_norm, scales = 20.0, [0.2, 3.0, 0.3, 2.0, 0.5, 4.0]
    pa, pb = _params(dev), _params(dev)
    a = FlatAdam(pa, lr=2e-3, betas=(0.9, 0.99), weight_decay=0.01, max_grad_norm=max_norm)
    ref = TorchRef(pb, lr=2e-3, betas=(0.9, 0.99), weight_decay=0.01, max_grad_norm=max_norm)
    for it, sc in enumerate(scales):
        g = _grads(it, dev, sc)
        _step(a, pa, g)
        ref.step(g)
        got = a.last_grad_norm()
        assert abs(got - ref.norms[-1]) <= 2e-6 * ref.norms[-1], (it, got, ref.norms[-1])
        for p, gi in zip(pa, g):
            assert torch.equal(p.grad, gi)                            # the update never writes the gradient buffer
    assert sum(n > max_norm for n in ref.norms) >= 2 and sum(n < max_norm for n in ref.norms) >= 2, ref.norms
    _compare(a, pa, ref, "clipping alone", ema=False)
    assert a.skipped_steps() == 0


def test_nonfinite_guard(backend):
    """Case 4: an inf at iteration 2 and a nan at iteration 4 (ordinary non-finite DATA) - those steps change nothing, and the run equals a
    torch run that leaves the two iterations out."""
    dev = backend
    pa, pb = _params(dev), _params(dev)
    a = FlatAdam(pa, lr=2e-3, betas=(0.9, 0.99), weight_decay=0.01, ema_decay=0.9, skip_nonfinite=True)
    ref = TorchRef(pb, lr=2e-3, betas=(0.9, 0.99), weight_decay=0.01, ema_decay=0.9)
    for it in range(6):
        g = _grads(it, dev)
        if it in (2, 4):
            g[2].view(-1)[17] = float("inf") if it == 2 else float("nan")
            fl = a.ensure_flat()[0]
            before = {k: fl[k].clone() for k in ("p", "m", "v", "ema")}
            _step(a, pa, g)
            for k, v in before.items():
                assert torch.equal(fl[k], v), k
            assert not math.isfinite(a.last_grad_norm())
        else:
            _step(a, pa, g)
            ref.step(g)
            assert abs(a.last_grad_norm() - ref.norms[-1]) <= 2e-6 * ref.norms[-1]
    assert a.skipped_steps() == 2 and a.applied_steps() == 4
    assert float(a.state_dict()["state"][0]["step"]) == 4.0
    _compare(a, pa, ref, "guard")


def test_guard_off_lets_the_value_through(backend):
    """Without skip_nonfinite the clipped step behaves like the torch calls: the non-finite norm reaches the update."""
    dev = backend
    pa = _params(dev)
    a = FlatAdam(pa, lr=2e-3, max_grad_norm=1.0)
    g = _grads(0, dev)
    g[0].view(-1)[3] = float("nan")
    _step(a, pa, g)
    assert a.skipped_steps() == 0 and a.applied_steps() == 1 and not bool(torch.isfinite(pa[0]).all())


def test_all_options_with_scheduler_and_roundtrip(backend):
    """Case 5: everything on, MultiStepLR, a state_dict -> new FlatAdam -> load_state_dict round trip in the middle (the device step counter
    and the average travel in the ordinary optimizer state); then a state WITHOUT "ema" entries loads and the average restarts."""
    dev = backend
    kw = dict(lr=2e-3, betas=(0.9, 0.99), weight_decay=0.01)
    opts = dict(ema_decay=0.95, ema_start_step=1, max_grad_norm=20.0, skip_nonfinite=True)
    scales = [0.3, 3.0, 0.4, 2.5, 1.0]
    pa, pb = _params(dev), _params(dev)
    a = FlatAdam(pa, **kw, **opts)
    ref = TorchRef(pb, ema_decay=0.95, ema_start_step=1, max_grad_norm=20.0, **kw)
    sched = torch.optim.lr_scheduler.MultiStepLR(a, milestones=[2], gamma=0.1)
    sched_b = torch.optim.lr_scheduler.MultiStepLR(ref.opt, milestones=[2], gamma=0.1)
    for it, sc in enumerate(scales):
        g = _grads(it, dev, sc)
        _step(a, pa, g)
        ref.step(g)
        sched.step()
        sched_b.step()
        if it == 1:
            sd = a.state_dict()
            assert float(sd["state"][0]["step"]) == 2.0 and "ema" in sd["state"][0]
            a2 = FlatAdam(pa, **kw, **opts)
            a2.load_state_dict(sd)
            sched2 = torch.optim.lr_scheduler.MultiStepLR(a2, milestones=[2], gamma=0.1)
            sched2.load_state_dict(sched.state_dict())
            a, sched = a2, sched2
            assert a.applied_steps() == 2
    assert sum(n > 20.0 for n in ref.norms) >= 2 and sum(n < 20.0 for n in ref.norms) >= 2, ref.norms
    assert a.param_groups[0]["lr"] == pytest.approx(ref.opt.param_groups[0]["lr"])
    _compare(a, pa, ref, "all options")
    # a state saved without an average (a reference-saved optimizer, an older checkpoint)
    sd = ref.opt.state_dict()
    assert all("ema" not in st for st in sd["state"].values())
    a3 = FlatAdam(pa, **kw, **opts)
    a3.load_state_dict(sd)
    fl = a3.ensure_flat()[0]
    assert a3.applied_steps() == len(scales) and a3.skipped_steps() == 0
    for i, x in enumerate(pa):
        assert torch.equal(a3.state[x]["ema"], x.detach())
        assert_close(a3.state[x]["exp_avg"], sd["state"][i]["exp_avg"], 0.0, "loaded exp_avg")
    assert torch.equal(fl["ema"], fl["p"])


def test_option_validation():
    ps = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(max_grad_norm=0.0), dict(ema_decay=0.9, ema_start_step=-1)):
        with pytest.raises(ValueError):
            FlatAdam(ps, **bad)
    with pytest.raises(ValueError, match="ONE parameter group"):
        FlatAdam([{"params": ps}, {"params": [torch.nn.Parameter(torch.zeros(2))]}], skip_nonfinite=True)
    with pytest.raises(RuntimeError, match="no average"):
        with FlatAdam(ps, skip_nonfinite=True).ema_weights():
            pass


# ------------------------------------------------------------------------------------------------------------------ the C entry points
GRID_CAP, BLOCK = 4096, 256


def _chain_length(n):
    """L of lfdm_grad_sumsq_f32 (include/lfdm_hip.h): per-accumulator chain of fused multiply-adds for the launch geometry of n."""
    n4 = n // 4
    grid = min(max((n4 + BLOCK - 1) // BLOCK, 1), GRID_CAP)
    return (n4 + BLOCK * grid - 1) // (BLOCK * grid) + (1 if n % 4 else 0), grid


def _norm_via_c(lib, g, stream):
    n = g.numel()
    nparts = lib.lfdm_grad_sumsq_ws_bytes(n) // 4
    parts = torch.full((nparts,), float("nan"), dtype=torch.float32, device=g.device)
    plan = torch.zeros(_native.OPTIM_PLAN_BYTES // 4, dtype=torch.int32, device=g.device)
    P = lambda t: C.c_void_p(t.data_ptr())
    lib.check(lib.lfdm_grad_sumsq_f32(P(g), n, P(parts), nparts * 4, stream), "sumsq")
    lib.check(lib.lfdm_optim_plan_f32(P(parts), nparts, P(plan), plan.numel() * 4, 1.0, -1.0, 1, 0.9, 0.99, -1.0, 0, stream), "plan")
    return parts.cpu(), plan.cpu()


def _norm_sizes(dev):
    # 1, 3 (< one float4), 4, 1023 (partial workgroup, n % 4), one workgroup's worth, a few workgroups + n % 4 == 1, the first n at which
    # the 4096-workgroup cap engages (n / 4 = 4096 * 256 + 1) and that n + 4; on the GPU the UNet's parameter count (n % 4 == 3)
    cap = 4 * (GRID_CAP * BLOCK + 1)
    sizes = [1, 3, 4, 1023, 1024, 70001, cap, cap + 4]
    return sizes + [42731203] if dev == "cuda" else sizes


def test_norm_accuracy_and_dispatch_edges(backend):
    """Case 6.  Bound: relative error of the norm <= (L + 12) * 2^-24 - L roundings of the accumulator chain, 2 for the merge of the four
    accumulators, 6 wave-butterfly + 2 LDS levels, the square root / final rounding to fp32, and slack of 1; the partials are summed in
    fp64.  With the 4096 x 256 cap and four accumulators L = 12 at 42 731 203 elements: bound 1.43e-6.  The largest error the runs reach is
    printed (pytest -s) and recorded in DESIGN.md 4.4."""
    from cvpr23_lfdm_amd import ops
    dev = backend
    lib = ops._lib()
    stream = ops._stream(lib)
    worst = 0.0
    for n in _norm_sizes(dev):
        L, grid = _chain_length(n)
        assert lib.lfdm_grad_sumsq_ws_bytes(n) == 4 * grid
        g = (torch.randn(n, generator=torch.Generator().manual_seed(n % 9973)) * 0.37).to(dev)
        want = math.sqrt(float((g.double() ** 2).sum()))
        parts, plan = _norm_via_c(lib, g, stream)
        parts2, plan2 = _norm_via_c(lib, g, stream)
        assert torch.equal(parts, parts2) and torch.equal(plan, plan2), n            # a fixed function of (g, n, grid)
        got = float(plan.view(torch.float32)[3])
        rel = abs(got - want) / want
        bound = (L + 12) * 2.0 ** -24
        print("grad_sumsq n=%d grid=%d L=%d rel_err=%.3e bound=%.3e" % (n, grid, L, rel, bound))
        worst = max(worst, rel / bound)
        assert rel <= bound, (n, L, rel, bound)
        assert int(plan[0]) == 1 and float(plan.view(torch.float32)[2]) == 1.0 and plan.view(torch.int64)[4:6].tolist() == [1, 0]
    print("grad_sumsq worst fraction of the bound: %.3f" % worst)


def test_guarded_entry_points_validate_arguments(backend):
    from cvpr23_lfdm_amd import ops
    dev = backend
    lib = ops._lib()
    stream = ops._stream(lib)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    g = torch.zeros(4096, device=dev)
    parts = torch.zeros(8, device=dev)
    plan = torch.zeros(16, dtype=torch.int32, device=dev)
    assert lib.lfdm_grad_sumsq_ws_bytes(0) == 0 and lib.lfdm_grad_sumsq_ws_bytes(4096) == 16
    assert lib.lfdm_grad_sumsq_f32(P(g), 4096, P(parts), 12, stream) != 0                 # scratch too small
    assert b"grad_sumsq" in lib.lfdm_last_error()
    assert lib.lfdm_grad_sumsq_f32(P(g, 4), 4092, P(parts), 32, stream) != 0              # misaligned gradient
    assert lib.lfdm_grad_sumsq_f32(P(g), 0, P(parts), 32, stream) != 0                    # n > 0
    assert lib.lfdm_optim_plan_f32(P(parts), 4, P(plan), 32, 1.0, -1.0, 0, 0.9, 0.99, -1.0, 0, stream) != 0      # plan too small
    assert lib.lfdm_optim_plan_f32(None, 0, P(plan), 64, 1.0, 1.0, 0, 0.9, 0.99, -1.0, 0, stream) != 0           # clipping without partials
    assert lib.lfdm_optim_plan_f32(P(parts), 4, P(plan, 4), 64, 1.0, -1.0, 0, 0.9, 0.99, -1.0, 0, stream) != 0   # misaligned plan
    assert lib.lfdm_adam_guarded_step_f32(P(g), P(g), P(g), P(g), None, 0, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1.0, P(plan), stream) != 0
    assert lib.lfdm_adam_guarded_step_f32(P(g), P(g), P(g), P(g), P(g, 4), 4, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1.0, P(plan), stream) != 0
    assert lib.lfdm_adam_guarded_step_f32(P(g), P(g), P(g), P(g), None, 4, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1.0, None, stream) != 0


def test_guarded_step_tail_elements(backend):
    """n % 4 != 0 through the C entry point (FlatAdam's own buffers are multiples of 4): the scalar tail of the update and of the norm."""
    from cvpr23_lfdm_amd import ops
    dev = backend
    lib = ops._lib()
    stream = ops._stream(lib)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    n = 1027
    p0, g = rnd(n, seed=1), rnd(n, seed=2) * 3.0
    ref = TorchRef([torch.nn.Parameter(p0.clone())], lr=1e-2, betas=(0.9, 0.99), weight_decay=0.01, ema_decay=0.5, max_grad_norm=5.0)
    p, m, v, e = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), p0.clone().to(dev)
    gd = g.to(dev)
    parts = torch.zeros(lib.lfdm_grad_sumsq_ws_bytes(n) // 4, device=dev)
    plan = torch.zeros(16, dtype=torch.int32, device=dev)
    for it in range(2):
        ref.step([g])
        lib.check(lib.lfdm_grad_sumsq_f32(P(gd), n, P(parts), parts.numel() * 4, stream), "sumsq")
        lib.check(lib.lfdm_optim_plan_f32(P(parts), parts.numel(), P(plan), 64, 1.0, 5.0, 1, 0.9, 0.99, 0.5, 0, stream), "plan")
        lib.check(lib.lfdm_adam_guarded_step_f32(P(p), P(gd), P(m), P(v), P(e), n, 1e-2, 0.9, 0.99, 1e-8, 0.01, 1.0, P(plan), stream), "step")
    assert ref.norms[0] > 5.0
    assert_close(p, ref.ps[0], 1e-6, "tail: params")
    assert_close(e, ref.ema[0], 1e-6, "tail: ema")
    assert_close(m, ref.opt.state[ref.ps[0]]["exp_avg"], 1e-6, "tail: exp_avg")


# ------------------------------------------------------------------------------------------------------------------ two ranks over gloo
WORKER = r'''
import json, os, sys
sys.path.insert(0, %(repo)r); sys.path.insert(0, os.path.join(%(repo)r, "tests"))
import torch, torch.distributed as dist
from cvpr23_lfdm_amd import _build, _native
_native._set_library_for_tests(_native.NativeLibrary(_build.build_emu(), "emu"))   # CPU test: emulation build
from cvpr23_lfdm_amd.optim import FlatAdam, GradAllReduce
from util import rnd
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
shapes = [(7, 5), (13,), (4, 3, 3, 3), (1,), (64, 9)]
ps = [torch.nn.Parameter(rnd(*s, seed=i + 100 * rank)) for i, s in enumerate(shapes)]   # ranks start DIFFERENT ...
opt = FlatAdam(ps, lr=1e-2, betas=(0.9, 0.99), weight_decay=0.01, ema_decay=0.9, ema_start_step=1, max_grad_norm=%(max_norm)r, skip_nonfinite=True)
if rank == 1:                                      # ... including the average and the device counters
    opt.ensure_flat()[0]["ema"].add_(1.0)
    opt.ensure_flat()[0]["plan"].view(torch.int64)[4] = 7
dp = GradAllReduce(opt, bucket_bytes=256)
drift0 = dp.replica_checksum()
dp.sync_replicas()
assert drift0 > 0 and dp.replica_checksum() == 0.0, (drift0, dp.replica_checksum())
assert opt.applied_steps() == 0
scales = %(scales)r
norms = []
for it, sc in enumerate(scales):
    opt.zero_grad()
    dp.prepare()
    data = [rnd(*p.shape, seed=1000 * it + 10 * rank + i) * sc for i, p in enumerate(ps)]
    if it == %(bad_it)d and rank == 1:             # a non-finite gradient value on ONE rank: after the sum every rank sees it
        data[2].view(-1)[5] = float("inf")
    sum((p * d).sum() for p, d in zip(ps, data)).backward()
    dp.finish()
    opt.step()
    norms.append(opt.last_grad_norm())
assert dp.replica_checksum() == 0.0
out = {"p": [p.detach().reshape(-1).tolist() for p in ps], "ema": [opt.state[p]["ema"].reshape(-1).tolist() for p in ps],
       "skipped": opt.skipped_steps(), "applied": opt.applied_steps(), "norms": [repr(n) for n in norms]}
gathered = [None] * world
dist.all_gather_object(gathered, out)
if rank == 0:
    print(json.dumps({"ranks": gathered}))
dist.destroy_process_group()
'''


def test_guarded_step_two_ranks_gloo(tmp_path):
    """Case 7: two gloo ranks (emulation build), all three options on, ranks starting from different parameters / average / counters; one
    iteration carries an inf on rank 1 only.  Every rank derives the plan from the identical all-reduced buffer, so both skip that
    iteration, take bit-identical updates otherwise (replica_checksum() == 0.0 with `ema` included) and agree with single-process torch."""
    max_norm, scales, bad_it = 10.0, [0.2, 2.0, 1.0, 0.3, 3.0], 2
    script = tmp_path / "dp_guarded_worker.py"
    script.write_text(WORKER % {"repo": REPO, "max_norm": max_norm, "scales": scales, "bad_it": bad_it})
    port = "29591"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", port, str(script)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    r0, r1 = out["ranks"]
    assert r0 == r1                                                                  # identical update, average, counters and norms
    assert r0["skipped"] == 1 and r0["applied"] == len(scales) - 1
    ps = [torch.nn.Parameter(rnd(*s, seed=i)) for i, s in enumerate(SHAPES)]
    ref = TorchRef(ps, lr=1e-2, betas=(0.9, 0.99), weight_decay=0.01, ema_decay=0.9, ema_start_step=1, max_grad_norm=max_norm)
    for it, sc in enumerate(scales):
        if it == bad_it:
            assert not math.isfinite(float(r0["norms"][it]))
            continue
        ref.step([sum(rnd(*s, seed=1000 * it + 10 * rk + i) * sc for rk in range(2)) / 2 for i, s in enumerate(SHAPES)])
        assert abs(float(r0["norms"][it]) - ref.norms[-1]) <= 2e-6 * ref.norms[-1]
    assert sum(n > max_norm for n in ref.norms) >= 2 and sum(n < max_norm for n in ref.norms) >= 2, ref.norms
    for got, ema, p, e in zip(r0["p"], r0["ema"], ref.ps, ref.ema):
        assert_close(torch.tensor(got), p.detach().reshape(-1), 1e-6, "dp guarded params")
        assert_close(torch.tensor(ema), e.reshape(-1), 1e-6, "dp guarded ema")


# ------------------------------------------------------------------------------------------------------------------ full size
@pytest.mark.gpu
def test_guarded_step_full_size_gpu():
    """Case 9: guarded steps over the real 42.7 M-parameter flat buffer (the UNet's parameter shapes) with synthetic gradients - one that
    clips, one that is skipped (an inf), one that does not clip - against torch Adam + clip_grad_norm_ + the moving average on the device.
    No weight decay here (tests of the clip-before-decay order: test_clipping_alone, test_guarded_step_tail_elements): with 42.7 M elements
    some hundred of them have g * clip_coef + weight_decay * p cancel to below eps = 1e-8, where Adam's first step lr * g / (|g| + eps) amplifies
    the one-rounding difference between two correct fp32 evaluations of that sum (7e-12) by lr * eps / (|g| + eps)^2 <= 1e5 - measured
    1.48e-6 on the MI355X with weight_decay=0.01, a property of Adam at a vanishing gradient and not of the guarded step."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvpr23_lfdm_amd import Unet3D
    _native._set_library_for_tests(None)
    dev = "cuda"
    shapes = [tuple(p.shape) for p in Unet3D(dim=64, channels=259, out_grid_dim=2, out_conf_dim=1, use_bert_text_cond=True).parameters()]
    assert sum(math.prod(s) for s in shapes) == 42731203
    gen = torch.Generator(device=dev).manual_seed(3)
    init = [torch.randn(s, generator=gen, device=dev) * 0.05 for s in shapes]
    pa, pb = [torch.nn.Parameter(x.clone()) for x in init], [torch.nn.Parameter(x.clone()) for x in init]
    kw = dict(lr=1e-3, betas=(0.9, 0.99))
    a = FlatAdam(pa, ema_decay=0.999, max_grad_norm=1.0, skip_nonfinite=True, **kw)
    ref = TorchRef(pb, ema_decay=0.999, max_grad_norm=1.0, **kw)
    for it, sc in enumerate((1e-3, 1e-3, 1e-5)):                     # norms ~ 6.5 (clips), -, ~0.065 (does not)
        g = [torch.randn(s, generator=gen, device=dev) * sc for s in shapes]
        if it == 1:
            g[40].view(-1)[0] = float("inf")
            _step(a, pa, g)
            continue
        _step(a, pa, g)
        ref.step(g)
        got = a.last_grad_norm()
        print("full size: norm %.9g reference %.9g" % (got, ref.norms[-1]))
        assert abs(got - ref.norms[-1]) <= 4e-6 * ref.norms[-1]          # (torch's own fp32 norm of 42.7 M elements is the looser side)
    assert ref.norms[0] > 1.0 > ref.norms[1]
    assert a.skipped_steps() == 1 and a.applied_steps() == 2
    _compare(a, pa, ref, "full size")
