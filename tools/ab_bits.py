#!/usr/bin/env python
"""Same bits?  Runs a fixed list of calls on seeded inputs under ONE build of the kernels and writes one line per output tensor -
name, shape, SHA-256 of its bytes - so that two builds (a refactor and its parent commit) can be compared line by line.

    tools/ab_bits.py run OUT.txt [--emu [LIB]] [--set conv|attention|norm|boundary|sampler|glue|train_loss]
                                                         this process, the library LFDM_HIP_LIB names (default: the in-tree one) on the GPU,
                                                         or an emulator library on the CPU (default: the in-tree one)
    tools/ab_bits.py diff A.txt B.txt                    exit status 1 when any line differs or is missing
    tools/ab_bits.py ab BASE_LIB OUT_DIR [--emu] [--new LIB] [--timeout S] [--set conv|attention|norm|boundary|sampler|glue|train_loss]
                                                         `run` under BASE_LIB, then under the in-tree library (or --new), each in a fresh child
                                                         process with its own time limit, one after the other; stops at the first non-zero
                                                         exit status; then `diff`

The calls are the suite's own: the listed tests of tests/ run in-process (their case lists cannot go stale here) with every function of
cvpr23_lfdm_amd.ops / train_ops / lfae_ops wrapped - each tensor a call returns, and the gn_partial buffer it was handed, becomes a line.  The
sampler set also records every tensor ARGUMENT after the call (the step writes x, hist, x0_out and the step counter in place; the workspace is
left out).  `extra` below adds the few cells no test reaches.  Nothing but tensor bytes is looked at."""
import argparse
import hashlib
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (file, -k expression) per --set.  conv: the smallest shapes that reach every epilogue / GroupNorm hand-off of the convolution family;
# norm: the GroupNorm / LayerNorm / BatchNorm kernels forward and backward, the heads kernels and the kernels that share csrc/norm_core.h;
# attention: every entry point that goes through csrc/attn_core.h (the short-sequence core, the fused temporal kernels, the low-resolution
# kernel), the long-sequence kernels beside them, the fast-math cases and the per-tile-order cases; sampler: every form of the sampler step (plain,
# multistep, known frames, known elements, counter noise), the blends and the quantile kernels under them; boundary: the kernels on the way
# into and out of the model (csrc/small.hip, csrc/conv_smalln.hip, the element-wise / layout kernels of csrc/norm.hip) at their launch-plan edges.
SETS = {
    "conv": ([
        ("tests/test_ops_parity.py",
         "test_conv2d or test_deconv_one_launch or test_conv_fused_groupnorm_stats or test_conv_fused_layernorm or test_conv_pointwise or "
         "test_conv_downsample_gather or test_winograd_pooled_epilogue or test_conv_winograd_splitk_reduced_in_launch or "
         "test_conv_winograd_balanced_launch or test_groupnorm_apply_many_partials or test_heads_with_groupnorm_folded"),
        ("tests/test_conv_wino_bf16.py", "test_conv2d_winograd_bf16"),
        ("tests/test_train_ops.py", "test_groupnorm_bwd"),
    ], "not gpu_only and not bigTrue and not random_geometries and not plan and not refuses and not smalln"),
    "attention": ([
        ("tests/test_ops_parity.py",
         "test_attention_temporal or test_attention_spatial or test_temporal_attention_fused or test_attention_lowres or "
         "test_temporal_attention_block_frame_edges or test_temporal_attention_fused_frame_edges or test_attention_frame_edges or "
         "test_spatial_attention_token_edges"),
        ("tests/test_attention_fast_math.py", "attention"),
        ("tests/test_attention_long.py", "test_forward or test_backward"),
        ("tests/test_attend_pipeline.py", "test_block or test_core"),
    ], "not refuses"),
    "norm": ([
        ("tests/test_ops_parity.py",
         "test_groupnorm_silu or test_groupnorm_apply_many_partials or test_conv_fused_groupnorm_stats or "
         "test_conv_pointwise_residual_groupnorm or test_layernorm or test_conv_planar_in_and_heads or test_heads_with_groupnorm_folded"),
        ("tests/test_train_ops.py", "test_groupnorm_bwd or test_layernorm_bwd"),
        ("tests/test_train_edges.py", "test_groupnorm_bwd_edges or test_layernorm_bwd_edges or test_colsum_block_cap"),
        ("tests/test_lfae_ops.py", "test_batchnorm_relu or test_batchnorm_relu_segments or test_batchnorm_fork_and_channel_slices"),
        ("tests/test_norm_edges.py", "test_layernorm or test_groupnorm or test_heads"),
    ], "not gpu_only and not bigTrue and not refuses"),
    "boundary": ([
        ("tests/test_boundary_edges.py",
         "test_stem_conv or test_heads or test_linear_small or test_sinusoidal or test_step_cond or test_conv2d_smalln or test_avgpool2 or "
         "test_transposes or test_affine_act"),
        ("tests/test_ops_parity.py",
         "test_linear_small_and_sinusoidal or test_conv_planar_in_and_heads or test_conv2d_smalln or test_elementwise_and_layout"),
    ], "not gpu_only and not bigTrue and not refusals"),
    "sampler": ([
        ("tests/test_ops_parity.py", "test_sampler_step or test_abs_quantile"),
        ("tests/test_threshold_select.py", "test_threshold_select"),
        ("tests/test_sampler_dpmpp.py", "test_step_ms"),
        ("tests/test_known_frames.py", "test_known_step or test_known_blend"),
        ("tests/test_known_elements.py", "test_known_elements_step or test_known_blend_elem or test_frame_constant_element_mask_is_the_frame_mask"),
        ("tests/test_counter_noise.py", "test_sampler_step_counter_is_the_loading_step"),
    ], "not refuse"),
    # glue: the kernels around the MFMA kernels that share csrc/warp_core.h (the warps forward and backward, grid_sample, the resize
    # adjoint) or end in the workgroup hand-off and the fixed-order folds of csrc/lfdm_device.h (BatchNorm, l1_mean, the fixed-point
    # finalize, the masked loss, the sampler's end of step, the gradient norm, the metrics and the flow colours)
    # The gradients are lines too: the recorder wraps forward and backward of the autograd Functions of the ops modules (dprev, the folded map
    # gradients, the fixed-point source gradient after finalize, dgrid, dx) and FlatAdam.step (every flat buffer after the step).
    "glue": ([
        ("tests/test_lfae_ops.py", "test_apply_optical or test_grid_sample or test_batchnorm or test_l1_mean"),
        ("tests/test_lfae_edges.py",
         "test_warp_ or test_apply_optical_ or test_resize_adjoint_edges or test_grid_sample_edges or test_absmax_exact or "
         "test_fix_finalize_exact or test_batchnorm_ or test_l1_mean_edges or test_region_stats_edges"),
        ("tests/test_ops_parity.py", "test_warp_cl or test_warp_planar"),
        ("tests/test_train_known.py", "test_masked_loss"),
        ("tests/test_optim_guarded.py",
         "test_ema_alone or test_clipping_alone or test_nonfinite_guard or test_guard_off_lets_the_value_through or "
         "test_norm_accuracy_and_dispatch_edges or test_guarded_step_tail_elements"),
        ("tests/test_metrics.py",
         "test_video_metrics_match_both_references or test_uint8_domain_is_the_bytes_of_sample_img or test_identical_operands_are_exact or "
         "test_constant_frames or test_psnr or test_deterministic_and_independent_of_the_batch or test_flow_metrics"),
        ("tests/test_render.py",
         "test_image_panels_are_sample_img or test_conf_panel_is_conf2fig or test_flow_colour or test_flow_panel_is_the_resized_colour_image or "
         "test_strip_panels_land_in_their_columns or test_strip_batch_elements_are_independent"),
    ], "not refusals"),
    # train_loss: the diffusion edge of DM training (csrc/train_diffusion.hip) and the distillation kernels that share csrc/train_elem_core.h,
    # forward, backward and through the autograd Functions.  When the C ABI differs between the two builds, `run` goes once in a checkout of
    # each commit (this file copied into the older one) and `diff` compares the two files.
    "train_loss": ([
        ("tests/test_train_known.py", "test_train_qsample or test_masked_loss"),
        ("tests/test_objective_loss.py", "test_objective_loss_fwd or test_objective_loss_bwd or test_objective_loss_autograd"),
        ("tests/test_distill_ops.py", "test_distill_x0 or test_distill_step"),
    ], "not refusals"),
}
ARGUMENTS_TOO = {"sampler"}      # sets whose calls write their results in place


class Recorder:
    """pytest plugin: wraps the ops layer for the session, names every recorded tensor test-id#call.function#index"""

    def __init__(self, out_path, emu_lib, arguments_too=False):
        self.lines, self.out_path, self.emu_lib, self.test, self.ncall, self.depth = [], out_path, emu_lib, "setup", 0, 0
        self.arguments_too = arguments_too

    def record(self, name, t):
        b = t.detach().cpu().contiguous().view(-1).view(dtype=__import__("torch").uint8).numpy().tobytes()
        self.lines.append("%s %s %s" % (name, "x".join(str(d) for d in t.shape) or "scalar", hashlib.sha256(b).hexdigest()))

    def wrap(self, mod):
        import torch

        def tensors(v):
            if isinstance(v, torch.Tensor):
                yield v
            elif isinstance(v, (tuple, list)):
                for e in v:
                    yield from tensors(e)

        def make(fname, f):
            def g(*a, **kw):
                self.depth += 1
                try:
                    r = f(*a, **kw)
                finally:
                    self.depth -= 1
                if self.depth > 0:      # only what the caller of the ops layer sees
                    return r
                self.ncall += 1
                outs = list(tensors(r)) + ([kw["gn_partial"]] if isinstance(kw.get("gn_partial"), torch.Tensor) else [])
                if self.arguments_too:
                    outs += list(tensors(a)) + [v for k, v in sorted(kw.items()) if isinstance(v, torch.Tensor) and k != "ws"]
                for i, t in enumerate(outs):
                    self.record("%s#%d.%s#%d" % (self.test, self.ncall, fname, i), t)
                return r
            g.__wrapped__ = f
            return g

        for fname, f in list(vars(mod).items()):
            if (callable(f) and not fname.startswith("_") and getattr(f, "__module__", None) == mod.__name__ and not isinstance(f, type)
                    and fname not in ("empty", "conv_params", "sampler_ws")):      # (uninitialised buffers, argument records)
                setattr(mod, fname, make(fname, f))
            elif isinstance(f, type) and issubclass(f, torch.autograd.Function) and f.__module__ == mod.__name__:
                # autograd looks forward / backward up on the class at every call: the gradients a backward returns become lines
                for meth in ("forward", "backward"):
                    setattr(f, meth, staticmethod(make("%s.%s" % (fname, meth), getattr(f, meth))))

    def wrap_optimizer(self, cls):
        """every flat buffer of the optimizer (parameters, moments, average, plan, norm partials) after each step"""
        import torch
        step = cls.step

        def g(opt, *a, **kw):
            r = step(opt, *a, **kw)
            self.ncall += 1
            before = len(self.lines)
            for gi, fl in enumerate(opt._flat or []):
                for key in sorted(k for k, v in fl.items() if isinstance(v, torch.Tensor) and k != "g"):
                    self.record("%s#%d.%s.step#%d.%s" % (self.test, self.ncall, cls.__name__, gi, key), fl[key])
            # (_flat is the optimizer's private layout: if it is renamed, stop here rather than compare nothing)
            assert len(self.lines) - before >= 3, "%s.step: parameters and both moments not found in _flat" % cls.__name__
            return r
        cls.step = g

    def pytest_sessionstart(self, session):
        sys.path.insert(0, R)
        from cvpr23_lfdm_amd import _build, lfae_ops, ops, train_ops
        if self.emu_lib:
            _build.build_emu = lambda force=False: self.emu_lib      # (the suite's `backend` fixture asks the build for the emulator library)
        self.wrap(ops)
        self.wrap(train_ops)
        self.wrap(lfae_ops)
        from cvpr23_lfdm_amd.optim import FlatAdam
        self.wrap_optimizer(FlatAdam)

    def pytest_runtest_setup(self, item):
        self.test, self.ncall = item.nodeid.split("::", 1)[1], 0


def extra(dev, rec):
    """Cells no test reaches.  Same conventions as the suite (tests/util.py layouts, seeded randn)."""
    import math
    import torch
    sys.path.insert(0, os.path.join(R, "tests"))
    from cvpr23_lfdm_amd import ops
    from util import rnd, to_cl

    # 2x2-wave schedule, scalar epilogue WITH statistics: the bias pointer is offset by one float (not 16-byte addressable)
    rec.test, rec.ncall = "extra_igemm_scalar_tail_with_gn_partial", 0
    n, cin, cout, h, w = 2, 32, 64, 8, 8
    x, wt = rnd(n, cin, h, w, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=1.0 / math.sqrt(cin * 9))
    bias = torch.zeros(cout + 1, device=dev)
    bias[1:] = rnd(cout, seed=3).to(dev)
    xs, wd = to_cl(x).to(dev), ops.pack_conv_weight(wt).to(dev)
    pp, _ = ops.conv_params(xs, wd, cout, 3, 3, n, h, w, bias=bias[1:], ksplit=1)
    assert ops.conv_schedule(pp) == 0, "the 2x2-wave schedule was not selected"
    rows, _ = ops.conv_plan(pp)
    partial = torch.zeros(n * (h * w // rows), 16, device=dev)
    ops.conv2d_cl(xs, wd, cout, 3, 3, n, h, w, bias=bias[1:], ksplit=1, gn_partial=partial, gn_groups=8, gn_pixels=h * w)

    # Winograd, a group wider than the workgroup's columns: 512 channels in 8 groups at 4x4 (32-column workgroups: two part slots per group)
    for bn in ("32", "64"):
        rec.test, rec.ncall = "extra_wino_group_spans_column_tiles_bn" + bn, 0
        os.environ.update(LFDM_WINO="1", LFDM_WINO_BN=bn)
        n, cin, cout, h, w = 16, 32, 512, 4, 4
        x, wt = rnd(n, cin, h, w, seed=1), rnd(cout, cin, 3, 3, seed=2, scale=1.0 / math.sqrt(cin * 9))
        xs, wd, ww = to_cl(x).to(dev), ops.pack_conv_weight(wt).to(dev), ops.pack_wino_weight(wt.to(dev))
        kw = dict(bias=rnd(cout, seed=3).to(dev), weight_wino=ww, ksplit=1)
        pp, _ = ops.conv_params(xs, wd, cout, 3, 3, n, h, w, **kw)
        assert ops.conv_schedule(pp) == 2, "the Winograd schedule was not selected"
        pixels = n // 2 * h * w                                            # two samples of 128 pixels = one tile block each
        partial = torch.zeros(2 * (pixels // 128) * 2, 16, device=dev)     # (room for two column parts per group)
        ops.conv2d_cl(xs, wd, cout, 3, 3, n, h, w, gn_partial=partial, gn_groups=8, gn_pixels=pixels, **kw)


def run(out_path, emu, which="conv"):
    import pytest
    tests, deselect = SETS[which]
    emu_lib = None
    if emu is not None:
        emu_lib = os.path.abspath(emu) if emu else os.path.join(R, "tests", "emu", "liblfdm_emu.so")
    rec = Recorder(out_path, emu_lib, which in ARGUMENTS_TOO)
    os.chdir(R)
    # (the F(2x2) Winograd cases run at both workgroup widths: LFDM_WINO_BN is a parameter of the suite's own tests)
    args = ["-q", "-p", "no:cacheprovider", "-x", "-m", "emu" if emu is not None else "gpu"]
    kexpr = "(" + " or ".join("(%s)" % k for _, k in tests) + ") and " + deselect
    rc = pytest.main(args + [f for f, _ in tests] + ["-k", kexpr], plugins=[rec])
    if rc != 0:
        return int(rc)
    # extra cells: drive the same wrapped ops under the same library
    import torch
    from cvpr23_lfdm_amd import _native
    if emu_lib:
        _native._set_library_for_tests(_native.NativeLibrary(emu_lib, "emu"))
    dev = "cpu" if emu_lib else "cuda"
    if which == "conv":
        extra(dev, rec)
    if dev == "cuda":
        torch.cuda.synchronize()
    with open(out_path, "w") as fh:
        fh.write("\n".join(rec.lines) + "\n")
    print("%d tensors -> %s" % (len(rec.lines), out_path))
    return 0


def diff(a, b):
    def load(p):
        d = {}
        for line in open(p):
            if line.strip():
                name, shape, h = line.rsplit(None, 2)
                d[name] = (shape, h)
        return d
    A, B = load(a), load(b)
    bad = 0
    for name in sorted(set(A) | set(B)):
        if A.get(name) != B.get(name):
            bad += 1
            print("DIFFERS %s: %s | %s" % (name, A.get(name, "missing"), B.get(name, "missing")))
    print("%d tensors compared, %d not bit-equal" % (len(set(A) | set(B)), bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run")
    r.add_argument("out")
    r.add_argument("--emu", nargs="?", const="", default=None)
    r.add_argument("--set", choices=sorted(SETS), default="conv")
    d = sub.add_parser("diff")
    d.add_argument("a")
    d.add_argument("b")
    c = sub.add_parser("ab")
    c.add_argument("base")
    c.add_argument("out_dir")
    c.add_argument("--new", default=None)
    c.add_argument("--emu", action="store_true")
    c.add_argument("--timeout", type=int, default=240)
    c.add_argument("--set", choices=sorted(SETS), default="conv")
    a = ap.parse_args()
    if a.mode == "run":
        return run(a.out, a.emu, a.set)
    if a.mode == "diff":
        return diff(a.a, a.b)
    os.makedirs(a.out_dir, exist_ok=True)
    outs = []
    for tag, lib in (("base", os.path.abspath(a.base)), ("new", os.path.abspath(a.new) if a.new else None)):
        out = os.path.join(a.out_dir, "bits_%s%s.txt" % ("emu_" if a.emu else "", tag))
        env = dict(os.environ)
        cmd = [sys.executable, os.path.abspath(__file__), "run", out, "--set", a.set]
        if a.emu:
            cmd += ["--emu"] + ([lib] if lib else [])
        elif lib:
            env["LFDM_HIP_LIB"] = lib
        else:
            env.pop("LFDM_HIP_LIB", None)
        try:
            rc = subprocess.run(cmd, env=env, cwd=R, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            print("%s: time limit of %d s" % (tag, a.timeout))
            return 124
        if rc != 0:
            print("%s: exit status %d" % (tag, rc))
            return rc
        outs.append(out)
    return diff(*outs)


if __name__ == "__main__":
    sys.exit(main())
