"""The oracle against the unmodified reference.  What the reference computes for these checks is stored in
tests/golden/oracle_vs_reference.npz (written by `PYTHONPATH=.:oracle python tests/test_oracle_vs_reference.py` where the reference tree is present),
so every check runs anywhere; where the reference tree is present the checks take the reference live and also pin the stored
values to it.  Only the CPU speed calibration needs the reference itself."""
import json
import os

import numpy as np
import pytest
import torch

import reference_loader

LIVE = reference_loader.reference_available()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_reference.npz")
_stored = None


def _gold(key):
    global _stored
    if _stored is None:
        _stored = dict(np.load(GOLDEN))
    return _stored[key]


def reference_value(key, live_fn):
    """The reference's value for `key`: computed live when the reference tree is present (and then it must equal the stored one),
    the stored one otherwise.  Tensors are stored as arrays, anything else as JSON."""
    if not LIVE:
        v = _gold(key)
        return json.loads(str(v)) if v.dtype.kind == "U" else torch.from_numpy(v)
    v = live_fn()
    if os.path.exists(GOLDEN):
        g = _gold(key)
        if torch.is_tensor(v):
            assert torch.equal(torch.from_numpy(g), v), "stored %s differs from the live reference" % key
        else:
            assert json.loads(str(g)) == json.loads(json.dumps(v)), "stored %s differs from the live reference" % key
    return v


def _live_unet():
    import synth
    ref = reference_loader.load_reference()
    b, t, s = 1, 2, 8
    m = ref.vfdm.FlowDiffusion(img_size=s, num_frames=t, sampling_timesteps=3, is_train=False,
                               config_pth=synth.CONFIG, pretrained_pth="")
    m.unet.load_state_dict(synth.unet_state(seed=99))
    m.generator.load_state_dict(synth.generator_state(seed=98))
    m.eval()
    x, time, cond = synth.unet_inputs(b, t, s, seed=12)
    with torch.no_grad():
        return m.unet(x, time, cond=cond, null_cond_prob=0.)


def test_unet_and_sampler_match_live_reference():
    import lfdm_oracle as O
    import synth
    b, t, s = 1, 2, 8
    want = reference_value("unet", _live_unet)
    dsd = {"denoise_fn." + k: v for k, v in synth.unet_state(seed=99).items()}
    x, time, cond = synth.unet_inputs(b, t, s, seed=12)
    got = O.unet_forward(dsd, x, time, cond)
    assert float((got - want).abs().max()) < 1e-5
    if LIVE:
        # drop-in import path resolves to the reference here (reference root precedes the repo root)
        import DM.modules.video_flow_diffusion_model as mod
        assert mod.__file__.startswith(reference_loader.REFERENCE_ROOT)


def _live_optimizer(learn_null_cond):
    """The reference's parameter order and the param_groups of its optimizer_diff (the state itself is made by the test)."""
    import synth
    ref = reference_loader.load_reference()
    rm = ref.vfdm.FlowDiffusion(img_size=8, num_frames=2, sampling_timesteps=5, is_train=True, config_pth=synth.CONFIG, pretrained_pth="",
                                learn_null_cond=learn_null_cond)
    groups = rm.optimizer_diff.state_dict()["param_groups"]
    return {"names": [k for k, _ in rm.diffusion.named_parameters()], "shapes": [list(p.shape) for p in rm.diffusion.parameters()],
            "param_groups": [dict(g, betas=list(g["betas"])) for g in groups]}


def _reference_optimizer_state(rec):
    """The optimizer_diff state dict the reference's training script would save, with a recognisable moment per parameter."""
    state = {i: {"step": torch.tensor(3.0), "exp_avg": torch.full(shape, float(i + 1)), "exp_avg_sq": torch.full(shape, 0.5 * (i + 1))}
             for i, shape in enumerate(rec["shapes"])}
    return {"state": state, "param_groups": [dict(g, betas=tuple(g["betas"])) for g in rec["param_groups"]]}


@pytest.mark.parametrize("learn_null_cond", [False, True])
def test_optimizer_state_of_the_reference_loads_into_flat_adam(learn_null_cond):
    """torch.optim state dicts index parameters by POSITION: with the reference's registration order mirrored
    (params.unet_spec) an `optimizer_diff` saved by the reference's training script restores into FlatAdam with every
    moment on the right parameter (train_video_flow_diffusion_mug.py:181 `model.optimizer_diff.load_state_dict`)."""
    import synth
    from cvpr23_lfdm_amd import FlowDiffusion
    rec = reference_value("optimizer_%d" % learn_null_cond, lambda: _live_optimizer(learn_null_cond))
    # (learn_null_cond: the root-level null_cond_emb parameter comes FIRST in the reference's named_parameters())
    kw = dict(img_size=8, num_frames=2, sampling_timesteps=5, is_train=True, config_pth=synth.CONFIG, pretrained_pth="",
              learn_null_cond=learn_null_cond)
    om = FlowDiffusion(**kw)
    rnames = rec["names"]
    assert rnames == [k for k, _ in om.diffusion.named_parameters()]
    assert rec["shapes"] == [list(p.shape) for p in om.diffusion.parameters()]
    sd = _reference_optimizer_state(rec)
    om.optimizer_diff.load_state_dict(sd)
    got = om.optimizer_diff.state_dict()
    assert got["param_groups"][0]["betas"] == sd["param_groups"][0]["betas"] and len(got["state"]) == len(rnames)
    for i, p in enumerate(om.diffusion.parameters()):
        st = om.optimizer_diff.state[p]
        assert st["exp_avg"].shape == p.shape and float(st["exp_avg"].flatten()[0]) == float(i + 1) and float(st["step"]) == 3.0
    # the moments are folded into the flat buffers at the first use: every one must have its parameter's size
    om.optimizer_diff.ensure_flat()
    # ... and a state saved for another parameter order is refused with a clear message instead of being mis-assigned
    bad = _reference_optimizer_state(rec)
    bad["state"][0], bad["state"][1] = bad["state"][1], bad["state"][0]
    om2 = FlowDiffusion(**kw)
    om2.optimizer_diff.load_state_dict(bad)
    with pytest.raises(ValueError, match="parameter ORDER"):
        om2.optimizer_diff.ensure_flat()


@pytest.mark.parametrize("bg_type", ["zero", "shift", "affine", "perspective"])
def test_bg_predictor_types_match_live_reference(bg_type):
    """oracle.bg_predictor for every bg_type against LFAE/modules/bg_motion_predictor.py:15-57 itself (eval mode, small encoder)."""
    import lfdm_oracle as O
    sd, src, drv = _bg_case(bg_type)
    if bg_type != "zero":
        assert set(reference_value("bg_%s_keys" % bg_type, lambda: sorted(_live_bg(bg_type)[0].state_dict()))) == set(sd)
    want = reference_value("bg_%s" % bg_type, lambda: _live_bg(bg_type)[1])
    with torch.no_grad():
        got = O.bg_predictor({k: v.float() for k, v in sd.items()}, src, drv, bg_type=bg_type, num_blocks=2)
    assert float((got - want).abs().max()) < 1e-5


def _bg_case(bg_type):
    from cvpr23_lfdm_amd import params as P
    kw = dict(block_expansion=8, max_features=32, num_blocks=2, bg_type=bg_type)
    sd = P.synthetic_state_dict(P.bg_predictor_spec(num_channels=3, **kw), 6262)
    if bg_type != "zero":
        sd["fc.weight"] = sd["fc.weight"] * 0.05
        sd["fc.bias"] = torch.tensor(P.BG_FC_BIAS[bg_type], dtype=torch.float32) + 0.2 * sd["fc.bias"]
    g = torch.Generator().manual_seed(79)
    src, drv = torch.rand(2, 3, 32, 32, generator=g), torch.rand(2, 3, 32, 32, generator=g)
    return sd, src, drv


def _live_bg(bg_type):
    reference_loader.load_reference()
    import LFAE.modules.bg_motion_predictor as bgm
    net = bgm.BGMotionPredictor(num_channels=3, block_expansion=8, max_features=32, num_blocks=2, bg_type=bg_type).eval()
    sd, src, drv = _bg_case(bg_type)
    net.load_state_dict(sd)
    with torch.no_grad():
        return net, net(src, drv)


@pytest.mark.parametrize("estimate_affine", [True, False])
def test_region_predictor_without_pca_matches_live_reference(estimate_affine):
    """oracle.region_predictor(pca_based=False) against LFAE/modules/region_predictor.py:28-117 itself (regression head / centres only)."""
    import lfdm_oracle as O
    from cvpr23_lfdm_amd import params as P
    kw = dict(block_expansion=8, max_features=32, num_blocks=2, temperature=0.1, scale_factor=0.25, pca_based=False, pad=3)
    sd = P.synthetic_state_dict(P.region_predictor_spec(num_regions=4, num_channels=3, estimate_affine=estimate_affine, **kw), 7171)
    from cvpr23_lfdm_amd.flow_diffusion import RegionPredictor
    ours = RegionPredictor(num_regions=4, num_channels=3, estimate_affine=estimate_affine, **kw)
    tag = "region_%d" % estimate_affine
    names = reference_value(tag + "_names", lambda: [k for k, _ in _live_region_net(estimate_affine).named_parameters()])
    assert names == [k for k, _ in ours.named_parameters()]                   # registration order
    if estimate_affine:       # and the regression head's identity initialisation (region_predictor.py:46-47)
        ref_bias = reference_value(tag + "_jacobian_bias", lambda: _live_region_net(True).jacobian.bias.detach().clone())
        assert torch.equal(ours.get("jacobian.bias").detach(), ref_bias) and float(ours.get("jacobian.weight").abs().max()) == 0.0
    assert set(reference_value(tag + "_keys", lambda: sorted(_live_region_net(estimate_affine).state_dict()))) == set(sd)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(80))
    with torch.no_grad():
        got = O.region_predictor({k: v.float() for k, v in sd.items()}, x, pca_based=False, num_blocks=2)
    want_keys = reference_value(tag + "_out_keys", lambda: sorted(_live_region(estimate_affine, sd, x)))
    assert set(got) == set(want_keys)
    for key in want_keys:
        want = reference_value(tag + "_" + key, lambda: _live_region(estimate_affine, sd, x)[key])
        assert float((got[key] - want).abs().max()) < 1e-5, key


def _live_region_net(estimate_affine):
    reference_loader.load_reference()
    import LFAE.modules.region_predictor as rpm
    return rpm.RegionPredictor(num_regions=4, num_channels=3, estimate_affine=estimate_affine, block_expansion=8, max_features=32, num_blocks=2,
                               temperature=0.1, scale_factor=0.25, pca_based=False, pad=3).eval()


def _live_region(estimate_affine, sd, x):
    net = _live_region_net(estimate_affine)
    net.load_state_dict(sd)
    with torch.no_grad():
        return net(x)


@pytest.mark.parametrize("use_deformed_source", [True, False])
def test_pixelwise_flow_predictor_matches_live_reference(use_deformed_source):
    """oracle.pixelwise_flow_predictor against LFAE/modules/pixelwise_flow_predictor.py:17-137 itself on a small hourglass, with and
    without the deformed sources in the hourglass input (:116-119; every LFDM yaml sets use_deformed_source: True)."""
    import lfdm_oracle as O
    k = 4
    gsd, sub, src, drv, sr, bg = _pixelwise_case(use_deformed_source)
    tag = "pixelwise_%d" % use_deformed_source
    assert set(reference_value(tag + "_keys", lambda: sorted(_live_pixelwise_net(use_deformed_source).state_dict()))) == set(sub)
    with torch.no_grad():
        got = O.pixelwise_flow_predictor({key: v.float() for key, v in gsd.items()}, src, drv, sr, bg, num_regions=k,
                                         use_deformed_source=use_deformed_source, num_blocks=2)
    for key in ("optical_flow", "occlusion_map"):
        want = reference_value(tag + "_" + key, lambda: _live_pixelwise(use_deformed_source, sub, src, drv, sr, bg)[key])
        assert float((got[key] - want).abs().max()) < 2e-5, key


def _pixelwise_case(use_deformed_source):
    from cvpr23_lfdm_amd import params as P
    k = 4
    spec = P.generator_spec(num_channels=3, block_expansion=8, max_features=32, num_down_blocks=1, num_bottleneck_blocks=1, num_regions=k,
                            fp_block_expansion=8, fp_max_features=32, fp_num_blocks=2, use_deformed_source=use_deformed_source)
    gsd = P.synthetic_state_dict(spec, 4242)
    pre = "pixelwise_flow_predictor."
    sub = {key[len(pre):]: v for key, v in gsd.items() if key.startswith(pre)}
    g = torch.Generator().manual_seed(81)
    n = 2
    src = torch.rand(n, 3, 64, 64, generator=g)
    mk = lambda: {"shift": torch.rand(n, k, 2, generator=g) * 1.2 - 0.6,
                  "covar": torch.eye(2).view(1, 1, 2, 2) * 0.02 + 0.004 * torch.rand(n, k, 1, 1, generator=g),
                  "affine": torch.eye(2).view(1, 1, 2, 2) * 0.15 + 0.03 * torch.rand(n, k, 2, 2, generator=g)}
    drv, sr = mk(), mk()
    bg = torch.eye(3).view(1, 3, 3).repeat(n, 1, 1) + 0.05 * torch.rand(n, 3, 3, generator=g)
    return gsd, sub, src, drv, sr, bg


def _live_pixelwise_net(use_deformed_source):
    reference_loader.load_reference()
    import LFAE.modules.pixelwise_flow_predictor as pfm
    return pfm.PixelwiseFlowPredictor(block_expansion=8, num_blocks=2, max_features=32, num_regions=4, num_channels=3, estimate_occlusion_map=True,
                                      scale_factor=0.25, use_covar_heatmap=True, use_deformed_source=use_deformed_source, revert_axis_swap=True).eval()


def _live_pixelwise(use_deformed_source, sub, src, drv, sr, bg):
    net = _live_pixelwise_net(use_deformed_source)
    net.load_state_dict(sub)
    with torch.no_grad():
        return net(src, drv, sr, bg_params=bg)


def test_p_losses_tensor_cond_quirk_is_stated(monkeypatch):
    """Bug-compatibility note (reference DM/modules/video_flow_diffusion.py:856-869): the single-GPU
    `GaussianDiffusion.p_losses` binds `none_cond_mask` only when `cond` is a list of strings, so a TENSOR condition raises
    UnboundLocalError in the reference (every reference script passes list[str]).  The drop-in is deliberately MORE permissive:
    a tensor condition trains with `none_cond_mask = None` (cvpr23_lfdm_amd/diffusion.py p_losses) - what the reference's own
    multi-GPU flavour does with a tensor (video_flow_diffusion_multiGPU.py, mask passed by the caller)."""
    import synth
    b, t, s = 1, 2, 8
    x0 = torch.zeros(b, 3, t, s, s)
    fea = torch.zeros(b, 256, t, s, s)
    tt = torch.zeros(b, dtype=torch.long)
    cond = torch.zeros(b, 768)
    if LIVE:            # the reference's own behaviour, where its tree is present
        ref = reference_loader.load_reference()
        rm = ref.vfdm.FlowDiffusion(img_size=s, num_frames=t, sampling_timesteps=3, is_train=True, config_pth=synth.CONFIG, pretrained_pth="")
        with pytest.raises(UnboundLocalError):
            rm.diffusion.p_losses(x0, tt, fea, cond=cond)

    from cvpr23_lfdm_amd import FlowDiffusion
    import cvpr23_lfdm_amd.unet_train as ut
    om = FlowDiffusion(img_size=s, num_frames=t, sampling_timesteps=3, is_train=True, config_pth=synth.CONFIG, pretrained_pth="")
    seen = {}

    def fake_forward(unet, x_noisy, fea2d, tsteps, c, **kw):       # (no kernels here: the test states the host-side contract only)
        seen.update(kw, cond=c)
        return torch.zeros_like(x_noisy, requires_grad=True)

    monkeypatch.setattr(ut, "unet_train_forward", fake_forward)
    om.diffusion.use_dynamic_thres = False
    om.unet.train()
    loss = om.diffusion.p_losses(x0, tt, fea[:, :, 0], cond=cond, clip_denoised=False)
    assert loss.dim() == 0 and seen["none_cond_mask"] is None and seen["cond"] is not None
    seen.clear()
    om.diffusion.text_encoder = lambda texts: cond
    om.diffusion.p_losses(x0, tt, fea[:, :, 0], cond=["None"], clip_denoised=False)
    assert seen["none_cond_mask"] == [True]


_CALIB_SCRIPT = r"""
import json, os, sys, time
import torch
sys.path.insert(0, %(oracle)r); sys.path.insert(0, %(tests)r)
import reference_loader
ref = reference_loader.load_reference()
import lfdm_oracle as O
import synth
b, t, s = 1, 40, 32
m = ref.vfdm.FlowDiffusion(img_size=s, num_frames=t, sampling_timesteps=100, is_train=False, config_pth=synth.CONFIG, pretrained_pth="")
usd = synth.unet_state()
m.unet.load_state_dict(usd)
m.eval()
dsd = {"denoise_fn." + k: v for k, v in usd.items()}
x, tt, cond = synth.unet_inputs(b, t, s, seed=12)
t_ref, t_port = [], []
with torch.no_grad():
    want = m.unet(x, tt, cond=cond, null_cond_prob=0.)            # warm-up of both (thread pools, allocator) = one more parity check
    got = O.unet_forward(dsd, x, tt, cond)
    err = float((got - want).abs().max()) / max(1.0, float(want.abs().max()))
    for _ in range(%(reps)d):
        t0 = time.perf_counter(); m.unet(x, tt, cond=cond, null_cond_prob=0.); t_ref.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); O.unet_forward(dsd, x, tt, cond); t_port.append(time.perf_counter() - t0)
print("CALIB " + json.dumps({"shape": [b, 259, t, s, s], "threads": torch.get_num_threads(), "host_cpus": os.cpu_count(), "rel_err": err,
      "reference_s_per_unet_forward": [round(v, 3) for v in t_ref], "port_s_per_unet_forward": [round(v, 3) for v in t_port],
      "port_over_reference": round(min(t_port) / min(t_ref), 3)}))
"""


@pytest.mark.skipif(not LIVE, reason="times the reference itself: reference tree not present")
def test_port_speed_is_calibrated_against_the_reference():
    """bench.py's `cpu_baseline` times the PORT (oracle/lfdm_oracle.py: /root/reference does not travel to the GPU box).  This pins what that
    number means: the reference's own `Unet3D.forward` and the port's `unet_forward` on the SAME cores, same C2-shape input (B = 1, 259
    channels, 40 frames, 32x32), interleaved, best of five each, in a FRESH interpreter (a process that has run other tests - emulator
    threads, changed thread pools - skews the two differently) - the port must be within +-15 % of the reference (one retry: the container's
    eight cores are shared).  LFDM_WRITE_CALIB=1 writes the pair to profiles/port_vs_reference_cpu.json, which bench.py quotes as
    `cpu_baseline.port_over_reference`."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _CALIB_SCRIPT % {"oracle": os.path.join(root, "oracle"), "tests": os.path.join(root, "tests"), "reps": 5}
    rec = None
    for attempt in range(2):
        r = subprocess.run([sys.executable, "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("CALIB ")][-1][6:])
        assert rec["rel_err"] < 2e-4
        if 0.85 <= rec["port_over_reference"] <= 1.15:
            break
    rec["what"] = ("best-of-5 wall time of ONE UNet forward at the C2 shape: the unmodified reference (DM/modules/video_flow_diffusion.py Unet3D.forward) vs "
                   "oracle/lfdm_oracle.py unet_forward, same fresh process, same torch threads, interleaved (tests/test_oracle_vs_reference.py)")
    print(json.dumps(rec))
    if os.environ.get("LFDM_WRITE_CALIB") == "1":
        with open(os.path.join(root, "profiles", "port_vs_reference_cpu.json"), "w") as f:
            json.dump(rec, f, indent=1)
    assert 0.85 <= rec["port_over_reference"] <= 1.15, rec


def _record():
    """Every reference value the checks above use -> tests/golden/oracle_vs_reference.npz (needs the reference tree)."""
    import lfdm_oracle  # noqa: F401
    from cvpr23_lfdm_amd import params as P
    assert LIVE, "the reference tree is needed to record its values"
    out = {"unet": _live_unet()}
    for lnc in (False, True):
        out["optimizer_%d" % lnc] = _live_optimizer(lnc)
    for bg_type in ("zero", "shift", "affine", "perspective"):
        net, want = _live_bg(bg_type)
        out["bg_%s_keys" % bg_type], out["bg_%s" % bg_type] = sorted(net.state_dict()), want
    kw = dict(block_expansion=8, max_features=32, num_blocks=2, temperature=0.1, scale_factor=0.25, pca_based=False, pad=3)
    for ea in (True, False):
        tag = "region_%d" % ea
        net = _live_region_net(ea)
        out[tag + "_names"], out[tag + "_keys"] = [k for k, _ in net.named_parameters()], sorted(net.state_dict())
        if ea:
            out[tag + "_jacobian_bias"] = net.jacobian.bias.detach().clone()
        sd = P.synthetic_state_dict(P.region_predictor_spec(num_regions=4, num_channels=3, estimate_affine=ea, **kw), 7171)
        want = _live_region(ea, sd, torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(80)))
        out[tag + "_out_keys"] = sorted(want)
        out.update({tag + "_" + key: v for key, v in want.items()})
    for uds in (True, False):
        out["pixelwise_%d_keys" % uds] = sorted(_live_pixelwise_net(uds).state_dict())
        _, sub, src, drv, sr, bg = _pixelwise_case(uds)
        want = _live_pixelwise(uds, sub, src, drv, sr, bg)
        for key in ("optical_flow", "occlusion_map"):
            out["pixelwise_%d_%s" % (uds, key)] = want[key]
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.array(json.dumps(v))) for k, v in out.items()}
    np.savez_compressed(GOLDEN, **arrays)
    print("wrote %s (%d entries)" % (GOLDEN, len(arrays)))


if __name__ == "__main__":
    _record()
