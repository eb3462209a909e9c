"""Training objectives and loss weights: objective_loss_fwd / objective_loss_bwd of csrc/train_diffusion.hip at the edges
of the launch plan, on both backends.  Shapes, masks and fixed timesteps are those of test_train_known.py, for its reasons: 60 floats per
sample (less than a workgroup, ragged), one frame, the shipped shape, and 270 336 floats per sample (the second trip over TD_CAP); mask
forms none / frame / elem with sample 0 all known and sample 1 all unknown; t[0] = 0, t[1] = T - 1; destinations NaN-filled.

Bars.  pred_x0 and inv_count: torch.equal (separately rounded fp32 expressions).  Loss and sample_loss: relative 1e-5 against float64 on
the fp32-rounded target and the fp32 table weight - the bar of test_train_known.py, whose derivation carries over: the weight is applied in
double and every term is non-negative.  Backward: 1e-6 of the largest gradient magnitude - five fp32 roundings in c_b = ((g inv) w) / B
(inv, two products, one quotient) and the l2 product, 5 * 2^-24 = 3e-7; exactly 0.0 at known elements."""
import ctypes
import functools

import pytest
import torch

from cvpr23_lfdm_amd import GaussianDiffusion, ops
from cvpr23_lfdm_amd._native import TrainLossParams, TrainMask
from util import rnd

NAN = float("nan")
TIMESTEPS = 1000
GAMMA = 5.0
SHAPES = [(3, 3, 5, 2, 2), (2, 3, 1, 4, 4), (2, 3, 40, 32, 32), (2, 3, 22, 64, 64)]
FORMS = ["none", "frame", "elem"]
OBJECTIVES = ["pred_noise", "pred_x0", "pred_v"]
TABS = ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")
GOUT = 1.75


def _nan(shape, dev):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device=dev)


@functools.lru_cache(maxsize=None)
def _tables():
    out = {}
    for obj in OBJECTIVES:
        d = GaussianDiffusion(torch.nn.Identity(), image_size=8, num_frames=4, timesteps=TIMESTEPS, sampling_timesteps=10, loss_type="l2",
                              objective=obj, min_snr_gamma=GAMMA)
        out[obj] = d.loss_weight.clone()
    out.update({k: getattr(d, k).clone() for k in TABS})
    return out


@functools.lru_cache(maxsize=None)
def _case(shape, form):
    """Inputs of one (shape, mask form), computed once and shared (never written)."""
    b, c, frames, s, _ = shape
    tab = _tables()
    x0, noise, out = rnd(*shape, seed=1), rnd(*shape, seed=2), rnd(*shape, seed=3)
    g = torch.Generator().manual_seed(4)
    t = torch.randint(0, TIMESTEPS, (b,), generator=g)
    t[0], t[1] = 0, TIMESTEPS - 1
    mask = torch.rand(b, frames, generator=g) < 0.4 if form == "frame" else torch.rand(*shape, generator=g) < 0.4 if form == "elem" else None
    if mask is not None:
        mask[0], mask[1] = True, False
    full = torch.zeros(shape, dtype=torch.bool) if mask is None else mask[:, None, :, None, None].expand(shape) if form == "frame" else mask
    a, sg, r, m = (tab[k][t].reshape(b, 1, 1, 1, 1) for k in TABS)
    x_noisy = torch.where(full, x0, a * x0 + sg * noise)
    target = {"pred_noise": noise, "pred_x0": x0, "pred_v": a * noise - sg * x0}               # fp32: two rounded products, one difference
    pred_x0 = {"pred_noise": r * x_noisy - m * out, "pred_x0": out, "pred_v": a * x_noisy - sg * out}
    pred_x0 = {k: torch.where(full, x_noisy, v) for k, v in pred_x0.items()}
    count = (~full).reshape(b, -1).sum(1).clamp(min=1).double()
    return dict(x0=x0, noise=noise, out=out, t=t, mask=mask, full=full, x_noisy=x_noisy, target=target, pred_x0=pred_x0, count=count,
                inv=(1.0 / count).float())


@functools.lru_cache(maxsize=None)
def _ref(shape, form, objective, loss_type, weighted):
    """float64 on the fp32-rounded target with the fp32 table weight: (loss, per-sample means, d loss / d out)."""
    case = _case(shape, form)
    b = shape[0]
    o64 = case["out"].double().requires_grad_(True)
    d = case["target"][objective].double() - o64
    term = (d.abs() if loss_type == "l1" else d * d) * (~case["full"])
    means = term.reshape(b, -1).sum(1) / case["count"]
    w = _tables()[objective][case["t"]].double() if weighted else torch.ones(b, dtype=torch.float64)
    loss = (w * means).mean()
    loss.backward()
    return float(loss.detach()), means.detach().clone(), o64.grad.clone()


def _operands(case, objective, dev, unused=None):
    """x_start / noise as the objective takes them: None where unused, or `unused` (a tensor) in that place."""
    x0 = case["x0"].to(dev) if objective != "pred_noise" else unused
    noise = case["noise"].to(dev) if objective != "pred_x0" else unused
    return x0, noise


def _mask_kw(case, form, dev):
    return {} if form == "none" else {form + "_mask": case["mask"].to(dev)}


def _fwd(case, form, objective, loss_type, weighted, dev, unused=None):
    tab, shape = _tables(), tuple(case["out"].shape)
    x0, noise = _operands(case, objective, dev, unused)
    return ops.objective_loss_fwd(objective, x0, noise, case["out"].to(dev), case["x_noisy"].to(dev), case["t"].to(dev),
                                  *[tab[k].to(dev) for k in TABS], tab[objective].to(dev) if weighted else None, loss_type=loss_type,
                                  loss=_nan((1,), dev), inv_count=_nan((shape[0],), dev), sample_loss=_nan((shape[0],), dev),
                                  pred_x0=_nan(shape, dev), **_mask_kw(case, form, dev))


def _bwd(case, form, objective, loss_type, weighted, dev, unused=None):
    tab, shape = _tables(), tuple(case["out"].shape)
    x0, noise = _operands(case, objective, dev, unused)
    return ops.objective_loss_bwd(objective, x0, noise, case["out"].to(dev), case["t"].to(dev), tab[TABS[0]].to(dev), tab[TABS[1]].to(dev),
                                  tab[objective].to(dev) if weighted else None, case["inv"].to(dev), torch.tensor([GOUT]).to(dev),
                                  loss_type=loss_type, dout=_nan(shape, dev), **_mask_kw(case, form, dev))


def _params():
    return [pytest.param(shape, form, id="%s-%s" % ("x".join(map(str, shape)), form)) for shape in SHAPES for form in FORMS]


@pytest.mark.parametrize("weighted", [False, True], ids=["w1", "minsnr"])
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("shape,form", _params())
def test_objective_loss_fwd(backend, shape, form, objective, loss_type, weighted):
    dev, case = backend, _case(shape, form)
    want, want_means, _ = _ref(shape, form, objective, loss_type, weighted)
    loss, inv_count, sample_loss, pred_x0 = got = _fwd(case, form, objective, loss_type, weighted, dev)
    rel = abs(float(loss) - want) / max(abs(want), 1e-30)
    mean_err = float(((sample_loss.cpu().double() - want_means).abs() / want_means.abs().clamp(min=1e-30)).max())
    print("objective_loss_fwd %s %s %s %s %s: %.9g against %.9g, relative %.3g; sample_loss relative %.3g"
          % (shape, form, objective, loss_type, weighted, float(loss), want, rel, mean_err))
    assert torch.isfinite(loss).all()
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    assert bool(((sample_loss.cpu().double() - want_means).abs() <= 1e-5 * want_means.abs()).all())
    assert torch.equal(inv_count.cpu(), case["inv"])
    full = case["full"]
    assert torch.equal(pred_x0.cpu()[~full], case["pred_x0"][objective][~full])
    assert torch.equal(pred_x0.cpu()[full], case["x_noisy"][full])
    if objective == "pred_x0":
        assert torch.equal(pred_x0.cpu()[~full], case["out"][~full])
    if form != "none":
        assert float(inv_count[0]) == 1.0 and float(sample_loss[0]) == 0.0           # the all-known sample
    for a, b2 in zip(got, _fwd(case, form, objective, loss_type, weighted, dev)):
        assert torch.equal(a, b2), "two runs on the same inputs differ"
    # an operand the objective does not use is never read: NaN in its place changes no bit
    if objective != "pred_v":
        for a, b2 in zip(got, _fwd(case, form, objective, loss_type, weighted, dev, unused=_nan(shape, dev))):
            assert torch.equal(a, b2), "an unused operand was read"
    # the anchor: the bits of the masked loss.  Both fronts run one kernel, so this pins the masked front's operand mapping (r / m tables in
    # their slots, x_start absent, sample_loss dropped); the bit identity with the two separate kernels this replaced was shown once, by
    # tools/ab_bits.py --set train_loss against the commit before (profiles/train_loss_refactor_ab.txt)
    if objective == "pred_noise" and not weighted:
        tab = _tables()
        anchor = ops.masked_loss_fwd(case["noise"].to(dev), case["out"].to(dev), case["x_noisy"].to(dev), case["t"].to(dev), tab[TABS[2]].to(dev),
                                     tab[TABS[3]].to(dev), loss_type=loss_type, **_mask_kw(case, form, dev))
        for a, b2 in zip((loss, inv_count, pred_x0), anchor):
            assert torch.equal(a, b2)


@pytest.mark.parametrize("weighted", [False, True], ids=["w1", "minsnr"])
@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("shape,form", _params())
def test_objective_loss_bwd(backend, shape, form, objective, loss_type, weighted):
    dev, case = backend, _case(shape, form)
    want = _ref(shape, form, objective, loss_type, weighted)[2] * GOUT
    got = _bwd(case, form, objective, loss_type, weighted, dev)
    bar = 1e-6 * float(want.abs().max())
    err = float((got.cpu().double() - want).abs().max())
    print("objective_loss_bwd %s %s %s %s %s: largest error %.3g, bar %.3g" % (shape, form, objective, loss_type, weighted, err, bar))
    assert not torch.isnan(got).any()
    assert err <= bar
    assert bool((got.cpu()[case["full"]] == 0.0).all())
    if form != "none":
        assert bool((got[0] == 0.0).all())
    assert torch.equal(got, _bwd(case, form, objective, loss_type, weighted, dev)), "two runs on the same inputs differ"
    if objective != "pred_v":
        assert torch.equal(got, _bwd(case, form, objective, loss_type, weighted, dev, unused=_nan(shape, dev))), "an unused operand was read"
    if objective == "pred_noise" and not weighted:          # (the anchor, as in the forward: the masked front's operand mapping, no t)
        anchor = ops.masked_loss_bwd(case["noise"].to(dev), case["out"].to(dev), case["inv"].to(dev), torch.tensor([GOUT]).to(dev),
                                     loss_type=loss_type, **_mask_kw(case, form, dev))
        assert torch.equal(got, anchor)


@pytest.mark.parametrize("objective", OBJECTIVES)
def test_objective_loss_autograd(backend, objective):
    """autograd.ObjectiveDiffusionLoss: the gradient goes to `out` only and is the backward kernel's."""
    from cvpr23_lfdm_amd import autograd as A
    dev, shape, tab = backend, SHAPES[0], _tables()
    case = _case(shape, "frame")
    out = case["out"].clone().to(dev).requires_grad_(True)                # (clones: the case is shared and never written)
    noise = case["noise"].clone().to(dev).requires_grad_(True)
    tabs = [tab[k].to(dev) for k in TABS] + [tab[objective].to(dev)]
    loss, pred_x0, sample_loss = A.objective_diffusion_loss(out, case["x0"].to(dev), noise, case["x_noisy"].to(dev), case["t"].to(dev), tabs,
                                                            case["mask"].to(dev), "l2", objective)
    assert loss.dim() == 0 and not pred_x0.requires_grad and not sample_loss.requires_grad and tuple(sample_loss.shape) == (shape[0],)
    (loss * GOUT).backward()
    assert noise.grad is None
    assert torch.equal(out.grad, _bwd(case, "frame", objective, "l2", True, dev))
    want = _ref(shape, "frame", objective, "l2", True)[2] * GOUT
    assert float((out.grad.cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


def test_objective_loss_refusals(backend):
    dev, tab = backend, _tables()
    a, s, r, m = (tab[k].to(dev) for k in TABS)
    t = torch.zeros(2, dtype=torch.int64, device=dev)
    x = torch.zeros(2, 3, 2, 2, 2, device=dev)
    dest = dict(loss=_nan((1,), dev), inv_count=_nan((2,), dev), sample_loss=_nan((2,), dev), pred_x0=_nan(x.shape, dev))
    with pytest.raises(ValueError, match="objective must be one of"):
        ops.objective_loss_fwd("pred_eps", x, x, x, x, t, a, s, r, m, **dest)
    with pytest.raises(ValueError, match="'pred_v' needs noise"):
        ops.objective_loss_fwd("pred_v", x, None, x, x, t, a, s, r, m, **dest)
    with pytest.raises(ValueError, match="'pred_x0' needs x_start"):
        ops.objective_loss_bwd("pred_x0", None, x, x, t, a, s, None, torch.ones(2, device=dev), torch.ones(1, device=dev))
    with pytest.raises(ValueError, match="loss_type"):
        ops.objective_loss_fwd("pred_v", x, x, x, x, t, a, s, r, m, loss_type="huber", **dest)
    with pytest.raises(ValueError, match="int64"):
        ops.objective_loss_fwd("pred_v", x, x, x, x, t.int(), a, s, r, m, **dest)
    with pytest.raises(ValueError, match="one length"):
        ops.objective_loss_fwd("pred_v", x, x, x, x, t, a, s, r, m, a[:7], **dest)
    with pytest.raises(ValueError, match="exclude each other"):
        ops.objective_loss_fwd("pred_v", x, x, x, x, t, a, s, r, m, frame_mask=torch.zeros(2, 2, dtype=torch.bool, device=dev),
                               elem_mask=torch.zeros_like(x, dtype=torch.bool), **dest)
    odd = torch.zeros(2, 3, 1, 1, 2, device=dev)                                   # n = 6: no multiple of 4
    with pytest.raises(RuntimeError, match="n % 4"):
        ops.objective_loss_fwd("pred_v", odd, odd, odd, odd, t, a, s, r, m, **dict(dest, pred_x0=_nan(odd.shape, dev)))
    assert all(bool(torch.isnan(v).all()) for v in dest.values())                  # a refused call writes nothing
    lib = ops._lib()
    p, n = ops._p, x[0].numel()
    bwd = dict(noise=p(x), out=p(x), t=p(t), a_tab=p(a), s_tab=p(s), t_len=a.numel(), inv_count=p(a), gout=p(a), dout=p(dest["pred_x0"]), batch=2, n=n)
    rc = lib.lfdm_objective_loss_bwd_f32(ctypes.byref(TrainLossParams(objective=7, x_start=p(x), **bwd)), ops._stream(lib))
    assert rc == -1 and b"objective must be" in lib.lfdm_last_error()
    rc = lib.lfdm_objective_loss_bwd_f32(ctypes.byref(TrainLossParams(objective=2, **bwd)), ops._stream(lib))
    assert rc == -1 and b"LFDM_OBJ_V needs x_start, noise, a_tab and s_tab" in lib.lfdm_last_error()
    assert bool(torch.isnan(dest["pred_x0"]).all())


def test_loss_params_refusals(backend):
    """lfdm_train_loss_params straight through ctypes: what the Python layer never lets through.  (2, 3, 2, 2, 2), n = 24: nothing smaller
    satisfies n % 4 == 0 with a two-frame split of 4-element frames.  Each case: the status, a word of the message, nothing written."""
    dev, tab = backend, _tables()
    lib = ops._lib()
    p = ops._p
    a, s, r, m = (tab[k].to(dev) for k in TABS)
    t = torch.zeros(2, dtype=torch.int64, device=dev)
    x = torch.zeros(2, 3, 2, 2, 2, device=dev)
    n = x[0].numel()
    fmask, emask = torch.zeros(2, 2, dtype=torch.uint8, device=dev), torch.zeros(2, n, dtype=torch.uint8, device=dev)
    dest = dict(loss=_nan((1,), dev), inv_count=_nan((2,), dev), sample_loss=_nan((2,), dev), pred_x0=_nan(x.shape, dev), dout=_nan(x.shape, dev))
    nbytes = lib.lfdm_masked_loss_ws_bytes(2, n)
    ws = torch.zeros(nbytes // 8, dtype=torch.int64, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    gout = torch.ones(1, device=dev)
    good = dict(objective=2, loss_type=0, x_start=p(x), noise=p(x), out=p(x), x_noisy=p(x), t=p(t), a_tab=p(a), s_tab=p(s), r_tab=p(r), m_tab=p(m),
                t_len=a.numel(), batch=2, n=n, gout=p(gout), ws=p(ws), ws_bytes=nbytes, ticket=p(ticket), **{k: p(v) for k, v in dest.items()})
    einval, eworkspace = -1, -3                                    # LFDM_EINVAL, LFDM_EWORKSPACE
    cases = [                                                      # (entry, fields changed, status, a word of the message)
        ("fwd", dict(objective=3), einval, b"objective must be"),
        ("bwd", dict(objective=3), einval, b"objective must be"),
        ("fwd", dict(objective=0, noise=None), einval, b"LFDM_OBJ_NOISE needs noise"),
        ("bwd", dict(objective=0, noise=None), einval, b"LFDM_OBJ_NOISE needs noise"),
        ("fwd", dict(objective=1, x_start=None), einval, b"LFDM_OBJ_X0 needs x_start"),
        ("bwd", dict(objective=1, x_start=None), einval, b"LFDM_OBJ_X0 needs x_start"),
        ("fwd", dict(objective=2, a_tab=None), einval, b"a_tab and s_tab"),
        ("bwd", dict(objective=2, a_tab=None), einval, b"a_tab and s_tab"),
        ("fwd", dict(objective=0, r_tab=None), einval, b"r_tab and m_tab"),
        ("fwd", dict(mask=TrainMask(p(fmask), p(emask), 2, 4)), einval, b"exclude each other"),
        ("bwd", dict(mask=TrainMask(p(fmask), p(emask), 2, 4)), einval, b"exclude each other"),
        ("fwd", dict(mask=TrainMask(None, None, 2, 4)), einval, b"needs frame_mask"),
        ("bwd", dict(mask=TrainMask(None, None, 2, 4)), einval, b"needs frame_mask"),
        ("fwd", dict(ws_bytes=nbytes - 1), eworkspace, b"workspace of"),
        ("fwd", dict(ticket=None), einval, b"ticket word"),
        ("bwd", dict(gout=None), einval, b"gout"),
    ]
    for entry, change, status, word in cases:
        fn = lib.lfdm_objective_loss_fwd_f32 if entry == "fwd" else lib.lfdm_objective_loss_bwd_f32
        rc = fn(ctypes.byref(TrainLossParams(**dict(good, **change))), ops._stream(lib))
        msg = lib.lfdm_last_error()
        assert rc == status and word in msg and msg.startswith(b"objective_loss_%s:" % entry.encode()), (entry, change, rc, msg)
        assert all(bool(torch.isnan(v).all()) for v in dest.values()), (entry, change)
    assert int(ticket) == 0
