"""DM training with known frames / elements held clean: the three kernels of csrc/train_diffusion.hip at the edges of
their launch plan, on both backends ("emu": index logic on a GPU-less machine; "hip": the device).

Launch plan (train_diffusion.hip): grid (workgroups of a sample, B), 256 lanes, TD_QUADS = 4 float4 per lane and trip, at most TD_CAP = 64
workgroups per sample - the grid-stride loop takes a second trip above 64 * 4 * 256 float4 = 262 144 floats per sample.  Shapes
(B, 3, T, S, S): 60 floats per sample (less than one workgroup, ragged tail), one frame, the shipped shape (30 workgroups per sample) and
(2, 3, 22, 64, 64) = 270 336 floats per sample, which takes the second trip of that cap.  Every destination is handed over NaN-filled.

Bars.  q_sample and pred_x0: torch.equal (separately rounded products and sum, as torch computes them).  Loss: relative 1e-5 against the
float64 restatement - every term is non-negative, and the only fp32 sums are the 16 terms of one lane's trip (pairwise inside a float4,
a chain over the four: at most 5 roundings on top of the term's own 2), everything above that is double: far inside
(128 + 8) * 2^-24 = 8.1e-6.  Backward: 1e-6 of the largest gradient magnitude (four fp32 roundings: inv_count, g * inv_count, / B, and for
l2 the product with 2 (pred - noise)), exactly 0.0 at every known element."""
import functools

import pytest
import torch

from cvpr23_lfdm_amd import GaussianDiffusion, ops
from util import rnd

NAN = float("nan")
TIMESTEPS = 1000
SHAPES = [(3, 3, 5, 2, 2), (2, 3, 1, 4, 4), (2, 3, 40, 32, 32), (2, 3, 22, 64, 64)]
# mask form x how the batch is filled: "edges" - sample 0 all known, sample 1 all unknown, the others mixed; "mixed" - every sample mixed
CASES = [("none", "edges"), ("frame", "edges"), ("frame", "mixed"), ("elem", "edges"), ("elem", "mixed")]


def _nan(shape, dev):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device=dev)


@functools.lru_cache(maxsize=None)
def _tables():
    d = GaussianDiffusion(torch.nn.Identity(), image_size=8, num_frames=4, timesteps=TIMESTEPS, sampling_timesteps=10, loss_type="l2")
    return {k: getattr(d, k).clone() for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod",
                                               "sqrt_recipm1_alphas_cumprod")}


@functools.lru_cache(maxsize=None)
def _case(shape, form, fill):
    """Inputs and the fp32 / float64 references of one case, computed once and shared (never written)."""
    b, c, frames, s, _ = shape
    tab = _tables()
    x0, noise, pred = rnd(*shape, seed=1), rnd(*shape, seed=2), rnd(*shape, seed=3)
    g = torch.Generator().manual_seed(4)
    t = torch.randint(0, TIMESTEPS, (b,), generator=g)
    t[0], t[1] = 0, TIMESTEPS - 1
    if form == "frame":
        mask = torch.rand(b, frames, generator=g) < 0.4
    elif form == "elem":
        mask = torch.rand(*shape, generator=g) < 0.4
    else:
        mask = None
    if mask is not None and fill == "edges":
        mask[0], mask[1] = True, False
    full = torch.zeros(shape, dtype=torch.bool) if mask is None else mask[:, None, :, None, None].expand(shape) if form == "frame" else mask
    shp = (b, 1, 1, 1, 1)
    x_noisy = torch.where(full, x0, tab["sqrt_alphas_cumprod"][t].reshape(shp) * x0 + tab["sqrt_one_minus_alphas_cumprod"][t].reshape(shp) * noise)
    pred_x0 = torch.where(full, x_noisy, tab["sqrt_recip_alphas_cumprod"][t].reshape(shp) * x_noisy
                          - tab["sqrt_recipm1_alphas_cumprod"][t].reshape(shp) * pred)
    ref = {}
    for loss_type in ("l1", "l2"):
        p64 = pred.double().requires_grad_(True)
        d = noise.double() - p64
        term = (d.abs() if loss_type == "l1" else d * d) * (~full)
        count = (~full).reshape(b, -1).sum(1).clamp(min=1).double()
        loss = (term.reshape(b, -1).sum(1) / count).mean()
        loss.backward()
        ref[loss_type] = (float(loss.detach()), p64.grad.clone(), (1.0 / count).float())
    return dict(x0=x0, noise=noise, pred=pred, t=t, mask=mask, full=full, x_noisy=x_noisy, pred_x0=pred_x0, ref=ref)


def _mask_kw(case, form, dev):
    return {} if form == "none" else {form + "_mask": case["mask"].to(dev)}


def _params():
    return [pytest.param(shape, form, fill, id="%s-%s-%s" % ("x".join(map(str, shape)), form, fill))
            for shape in SHAPES for form, fill in CASES if not (fill == "mixed" and shape[0] > 2)]


@pytest.mark.parametrize("shape,form,fill", _params())
def test_train_qsample(backend, shape, form, fill):
    dev, case, tab = backend, _case(shape, form, fill), _tables()
    out = ops.train_qsample(case["x0"].to(dev), case["noise"].to(dev), case["t"].to(dev), tab["sqrt_alphas_cumprod"].to(dev),
                            tab["sqrt_one_minus_alphas_cumprod"].to(dev), out=_nan(shape, dev), **_mask_kw(case, form, dev))
    assert torch.equal(out.cpu(), case["x_noisy"])
    assert torch.equal(out.cpu()[case["full"]], case["x0"][case["full"]])         # a known element is the bits of x_start


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("shape,form,fill", _params())
def test_masked_loss_fwd(backend, shape, form, fill, loss_type):
    dev, case, tab = backend, _case(shape, form, fill), _tables()
    args = [case[k].to(dev) for k in ("noise", "pred", "x_noisy", "t")] + [tab[k].to(dev) for k in ("sqrt_recip_alphas_cumprod",
                                                                                                  "sqrt_recipm1_alphas_cumprod")]

    def run():
        return ops.masked_loss_fwd(*args, loss_type=loss_type, loss=_nan((1,), dev), inv_count=_nan((shape[0],), dev), pred_x0=_nan(shape, dev),
                                   **_mask_kw(case, form, dev))

    loss, inv_count, pred_x0 = run()
    want, _, want_inv = case["ref"][loss_type]
    got = float(loss)
    print("masked_loss_fwd %s %s %s %s: %.9g against %.9g, relative %.3g" % (shape, form, fill, loss_type, got, want,
                                                                            abs(got - want) / max(abs(want), 1e-30)))
    assert torch.isfinite(loss).all()
    assert abs(got - want) <= 1e-5 * abs(want)
    assert torch.equal(inv_count.cpu(), want_inv)
    if form != "none" and fill == "edges":
        assert float(inv_count[0]) == 1.0                                          # the all-known sample: 1 / max(0, 1)
    full = case["full"]
    assert torch.equal(pred_x0.cpu()[~full], case["pred_x0"][~full])
    assert torch.equal(pred_x0.cpu()[full], case["x_noisy"][full])
    again = run()
    for a, b2 in zip((loss, inv_count, pred_x0), again):
        assert torch.equal(a, b2), "two runs on the same inputs differ"


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("shape,form,fill", _params())
def test_masked_loss_bwd(backend, shape, form, fill, loss_type):
    dev, case = backend, _case(shape, form, fill)
    _, want, inv = case["ref"][loss_type]
    gout = torch.tensor([1.75])
    args = (case["noise"].to(dev), case["pred"].to(dev), inv.to(dev), gout.to(dev))

    def run():
        return ops.masked_loss_bwd(*args, loss_type=loss_type, out=_nan(shape, dev), **_mask_kw(case, form, dev))

    got = run()
    want = want * 1.75
    bar = 1e-6 * float(want.abs().max())
    err = float((got.cpu().double() - want).abs().max())
    print("masked_loss_bwd %s %s %s %s: largest error %.3g, bar %.3g" % (shape, form, fill, loss_type, err, bar))
    assert not torch.isnan(got).any()
    assert err <= bar
    assert bool((got.cpu()[case["full"]] == 0.0).all())
    if form != "none" and fill == "edges":
        assert bool((got[0] == 0.0).all())
    assert torch.equal(got, run()), "two runs on the same inputs differ"


def test_masked_loss_autograd(backend):
    """autograd.MaskedDiffusionLoss: the gradient goes to pred only and is the backward kernel's."""
    from cvpr23_lfdm_amd import autograd as A
    dev, shape, tab = backend, SHAPES[0], _tables()
    case = _case(shape, "frame", "edges")
    pred = case["pred"].to(dev).requires_grad_(True)
    noise = case["noise"].to(dev).requires_grad_(True)
    loss, pred_x0 = A.masked_diffusion_loss(pred, noise, case["x_noisy"].to(dev), case["t"].to(dev), tab["sqrt_recip_alphas_cumprod"].to(dev),
                                            tab["sqrt_recipm1_alphas_cumprod"].to(dev), case["mask"].to(dev), "l2")
    assert loss.dim() == 0 and not pred_x0.requires_grad
    (loss * 1.75).backward()
    want = case["ref"]["l2"][1] * 1.75
    assert noise.grad is None
    assert float((pred.grad.cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


def test_refusals(backend):
    dev, tab = backend, _tables()
    a, s = tab["sqrt_alphas_cumprod"].to(dev), tab["sqrt_one_minus_alphas_cumprod"].to(dev)
    t = torch.zeros(2, dtype=torch.int64, device=dev)
    x = torch.zeros(2, 3, 2, 2, 2, device=dev)
    out = _nan(x.shape, dev)
    with pytest.raises(ValueError, match="exclude each other"):
        ops.train_qsample(x, x, t, a, s, frame_mask=torch.zeros(2, 2, dtype=torch.bool, device=dev), elem_mask=torch.zeros_like(x, dtype=torch.bool), out=out)
    with pytest.raises(ValueError, match="int64"):
        ops.train_qsample(x, x, t.int(), a, s, out=out)
    with pytest.raises(ValueError, match="loss_type"):
        ops.masked_loss_fwd(x, x, x, t, a, s, loss_type="huber")
    odd = torch.zeros(2, 3, 1, 1, 2, device=dev)                                   # n = 6: no multiple of 4
    with pytest.raises(RuntimeError, match="n % 4"):
        ops.train_qsample(odd, odd, t, a, s, out=_nan(odd.shape, dev))
    thin = torch.zeros(2, 2, 2, 1, 2, device=dev)                                  # frames of 2 elements: a float4 would straddle two
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.train_qsample(thin, thin, t, a, s, frame_mask=torch.zeros(2, 2, dtype=torch.bool, device=dev), out=_nan(thin.shape, dev))
    with pytest.raises(RuntimeError, match="table length|needed"):
        ops.train_qsample(x, x, t, a[:0], s[:0], out=out)
    assert bool(torch.isnan(out).all())                                            # a refused call writes nothing
    lib = ops._lib()
    import ctypes
    from cvpr23_lfdm_amd._native import TrainLossParams
    params = TrainLossParams(objective=0, loss_type=7, noise=ops._p(x), out=ops._p(x), inv_count=ops._p(a), gout=ops._p(a), dout=ops._p(out), batch=2,
                             n=x[0].numel())
    rc = lib.lfdm_objective_loss_bwd_f32(ctypes.byref(params), ops._stream(lib))
    assert rc == -1 and b"loss_type" in lib.lfdm_last_error()


# ------------------------------------------------------------------------------------------------------------------------------------
# d. through GaussianDiffusion.p_losses

class _StubDenoiser(torch.nn.Module):
    """A denoiser with Unet3D.forward's call signature and no kernels: p_losses around it is the diffusion edge alone (nothing to train:
    p_losses takes its forward-only branch)."""

    def __init__(self):
        super().__init__()
        self.register_buffer("w", torch.tensor(0.5))

    def forward(self, x, t, cond=None, null_cond_prob=0., none_cond_mask=None):
        return x[:, :3] * self.w + 0.1


def _stub_diffusion(dev, loss_type="l2", **kw):
    d = GaussianDiffusion(_StubDenoiser(), image_size=4, num_frames=5, timesteps=TIMESTEPS, sampling_timesteps=10, loss_type=loss_type,
                          null_cond_prob=0.0, **kw)          # (the stub draws no null-condition mask)
    return d.to(dev)


def _stub_inputs(dev, b=3):
    shape = (b, 3, 5, 4, 4)
    x0, noise = rnd(*shape, seed=21).to(dev), rnd(*shape, seed=22).to(dev)
    fea = rnd(b, 256, 4, 4, seed=23).to(dev)
    t = torch.tensor([0, TIMESTEPS - 1, 500][:b]).to(dev)
    return shape, x0, noise, fea, t


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("form", ["frame", "elem", "elem1"])
def test_p_losses_masked_edge(backend, form, loss_type):
    """p_losses with a mask around a stub denoiser: loss against the float64 restatement, pred_x0, and an all-False mask against the
    unmasked step on the same draws."""
    dev = backend
    d = _stub_diffusion(dev, loss_type)
    shape, x0, noise, fea, t = _stub_inputs(dev)
    g = torch.Generator().manual_seed(5)
    mask = {"frame": torch.rand(3, 5, generator=g) < 0.5, "elem": torch.rand(*shape, generator=g) < 0.5,
            "elem1": torch.rand(3, 1, 5, 4, 4, generator=g) < 0.5}[form]
    mask[0] = True
    full = (mask[:, None, :, None, None] if form == "frame" else mask).expand(shape)
    loss = d.p_losses(x0, t, fea, noise=noise, known_mask=mask.to(dev))
    shp = (3, 1, 1, 1, 1)
    a, s = d.sqrt_alphas_cumprod.cpu()[t.cpu()].reshape(shp), d.sqrt_one_minus_alphas_cumprod.cpu()[t.cpu()].reshape(shp)
    x_noisy = torch.where(full, x0.cpu(), a * x0.cpu() + s * noise.cpu())
    pred = x_noisy * 0.5 + 0.1
    diff = noise.cpu().double() - pred.double()
    term = (diff.abs() if loss_type == "l1" else diff * diff) * (~full)
    want = float((term.reshape(3, -1).sum(1) / (~full).reshape(3, -1).sum(1).clamp(min=1)).mean())
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    r, m = d.sqrt_recip_alphas_cumprod.cpu()[t.cpu()].reshape(shp), d.sqrt_recipm1_alphas_cumprod.cpu()[t.cpu()].reshape(shp)
    px0 = torch.where(full, x_noisy, r * x_noisy - m * pred)
    assert torch.equal(d.pred_x0.cpu(), px0.clamp(-1, 1))
    none = torch.zeros_like(mask).to(dev)
    masked, plain = d.p_losses(x0, t, fea, noise=noise, known_mask=none), d.p_losses(x0, t, fea, noise=noise)
    assert abs(float(masked) - float(plain)) <= 1e-3 * abs(float(plain))            # (the forward bar of test_unet_train)


def test_p_losses_refuses(backend):
    dev = backend
    shape, x0, noise, fea, t = _stub_inputs(dev)
    d = _stub_diffusion(dev, per_element_loss=True)
    with pytest.raises(NotImplementedError, match="per_element_loss"):
        d.p_losses(x0, t, fea, noise=noise, known_mask=torch.zeros(3, 5, dtype=torch.bool, device=dev))
    d = _stub_diffusion(dev)
    for bad in (torch.zeros(3, 4, dtype=torch.bool), torch.zeros(3, 5), torch.zeros(3, 2, 5, 4, 4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="known_mask"):
            d.p_losses(x0, t, fea, noise=noise, known_mask=bad.to(dev))


def test_p_losses_without_a_mask_runs_the_parents_statements(backend, monkeypatch):
    """Option off: none of the new entries is touched, and the loss is the eager expression's bits on the same draws."""
    dev = backend

    def forbidden(*a, **k):
        raise AssertionError("a known-frame training op was called on the unmasked path")

    for name in ("train_qsample", "masked_loss_fwd", "masked_loss_bwd"):
        monkeypatch.setattr(ops, name, forbidden)
    d = _stub_diffusion(dev)
    shape, x0, noise, fea, t = _stub_inputs(dev)
    torch.manual_seed(3)
    loss = d(x0, fea, None)
    torch.manual_seed(3)
    tt = torch.randint(0, TIMESTEPS, (3,), device=dev).long()
    nz = torch.randn_like(x0)
    x_noisy = d.q_sample(x0, tt, nz)
    want = torch.nn.functional.mse_loss(nz, x_noisy * 0.5 + 0.1)
    assert torch.equal(loss.detach(), want)


def _unet_case(dev, form):
    import lfdm_oracle as O
    import synth
    from cvpr23_lfdm_amd import Unet3D
    b, frames, s = (1, 2, 8) if dev == "cpu" else (2, 4, 8)
    usd = synth.unet_state()
    unet = Unet3D(dim=64, channels=259, out_grid_dim=2, out_conf_dim=1, use_bert_text_cond=True)
    unet.load_state_dict(usd)
    unet.to(dev).train()
    d = GaussianDiffusion(unet, image_size=s, num_frames=frames, timesteps=TIMESTEPS, sampling_timesteps=10, loss_type="l2", null_cond_prob=0.0).to(dev)
    x, time, cond = synth.unet_inputs(b, frames, s)
    shape = (b, 3, frames, s, s)
    x0, fea = x[:, :3].contiguous(), x[:, 3:, 0].contiguous()
    noise = synth.NoiseTape(11)(shape)
    g = torch.Generator().manual_seed(6)
    mask = torch.rand(b, frames, generator=g) < 0.5 if form == "frame" else torch.rand(*shape, generator=g) < 0.5
    full = (mask[:, None, :, None, None] if form == "frame" else mask).expand(shape)
    # the composition: x_noisy by torch.where, the oracle's UNet on it (fp32 torch autograd, as in test_unet_train: the oracle casts
    # to float itself), the masked mean on top of it in float64
    sd = {"denoise_fn." + k: v.clone().requires_grad_(v.is_floating_point() and "rotary" not in k) for k, v in usd.items()}
    shp = (b, 1, 1, 1, 1)
    a, sg = d.sqrt_alphas_cumprod.cpu()[time].reshape(shp), d.sqrt_one_minus_alphas_cumprod.cpu()[time].reshape(shp)
    x_noisy = torch.where(full, x0, a * x0 + sg * noise)
    pred = O.unet_forward(sd, torch.cat([x_noisy, x[:, 3:]], dim=1), time, cond)
    diff = noise.double() - pred.double()
    ref = ((diff * diff * (~full)).reshape(b, -1).sum(1) / (~full).reshape(b, -1).sum(1).clamp(min=1)).mean()
    ref.backward()
    unet.zero_grad()
    loss = d.p_losses(x0.to(dev), time.to(dev), fea.to(dev), cond=cond.to(dev), noise=noise.to(dev), known_mask=mask.to(dev))
    loss.backward()
    return unet, sd, loss, ref


@pytest.mark.parametrize("form", ["frame", "elem"])
def test_p_losses_masked_unet_grads(backend, form):
    """Loss and every parameter gradient through the native UNet, at test_unet_train's bars (1e-3 forward, 2e-3 of the largest gradient)."""
    import os
    dev = backend
    if dev == "cpu" and os.environ.get("LFDM_EMU_E2E", "0") != "1":
        pytest.skip("UNet forward+backward under the emulator is opt-in (LFDM_EMU_E2E=1); it runs on the GPU")
    unet, sd, loss, ref = _unet_case(dev, form)
    print("p_losses %s: loss %.9g against %.9g" % (form, float(loss.detach()), float(ref.detach())))
    assert abs(float(loss) - float(ref)) <= 1e-3 * max(1.0, abs(float(ref)))
    worst = ("", 0.0)
    for k, p in unet.named_parameters():
        rg = sd["denoise_fn." + k].grad
        assert p.grad is not None and rg is not None, k
        err = float((p.grad.cpu().double() - rg).abs().max()) / (float(rg.abs().max()) + 1e-12)
        if err > worst[1]:
            worst = (k, err)
    assert worst[1] < 2e-3, "largest relative gradient error %.3e at %s" % (worst[1], worst[0])


# ------------------------------------------------------------------------------------------------------------------------------------
# e. the mask policy (host only)

def _policy(**kw):
    from cvpr23_lfdm_amd.diffusion import KnownMaskPolicy
    return KnownMaskPolicy(40, **kw)


def test_policy_is_reproducible_and_leaves_a_frame_unknown():
    a, b = _policy(seed=7, prob=1.0), _policy(seed=7, prob=1.0)
    ma, mb = a.draw(64), b.draw(64)
    assert torch.equal(ma, mb) and torch.equal(a.draw(64), b.draw(64)) and not torch.equal(ma, a.draw(64))
    assert not torch.equal(ma, _policy(seed=8, prob=1.0).draw(64))
    p = _policy(seed=1, prob=1.0, max_frames=39)
    m = p.draw(2000)
    assert bool((m.sum(1) >= 1).all()) and bool((m.sum(1) <= 39).all())
    assert not bool(_policy(seed=1, prob=0.0).draw(100).any())
    for bad in (dict(max_frames=40), dict(max_frames=0), dict(prob=1.5), dict(kinds=("middle",)), dict(kinds=()), dict(seed=1.5)):
        with pytest.raises(ValueError, match="known_train"):
            _policy(**bad)
    with pytest.raises(TypeError):
        GaussianDiffusion(torch.nn.Identity(), image_size=8, num_frames=4, known_train=dict(chance=0.5))


def test_policy_frequencies():
    """Over 4000 draws: the conditioned share, the kind and k, each within 4 sigma of its binomial expectation.  The kind and k are read
    off the mask: a prefix has frame 0 and is contiguous; "ends" of k >= 2 has frames 0 and T - 1; k = the number of known frames."""
    n, prob, kmax, frames = 4000, 0.5, 8, 40
    m = _policy(seed=3, prob=prob, max_frames=kmax).draw(n)

    def within(count, total, p, what):
        sigma = (total * p * (1 - p)) ** 0.5
        assert abs(count - total * p) <= 4 * sigma, "%s: %d of %d, expected %.1f +- %.1f" % (what, count, total, total * p, sigma)

    k = m.sum(1)
    on = k > 0
    n_on = int(on.sum())
    within(n_on, n, prob, "conditioned videos")
    for v in range(1, kmax + 1):
        within(int((k == v).sum()), n_on, 1.0 / kmax, "k = %d" % v)
    # k >= 3: the three kinds are told apart with certainty up to a random subset that happens to look like one of the others
    sel = m[k >= 3]
    kk = sel.sum(1)
    prefix = torch.tensor([bool(r[:c].all()) for r, c in zip(sel, kk.tolist())])
    ends = torch.tensor([bool(r[:(c + 1) // 2].all() and r[frames - c // 2:].all()) for r, c in zip(sel, kk.tolist())])
    # (a random subset of k >= 3 of 40 frames is a prefix or the ends with probability <= 2 / C(40, 3) = 2e-4: inside the 4 sigma)
    within(int(prefix.sum()), len(sel), 1.0 / 3, "prefix")
    within(int(ends.sum()), len(sel), 1.0 / 3, "ends")
    within(int((~prefix & ~ends).sum()), len(sel), 1.0 / 3, "random")
    only = _policy(seed=3, prob=1.0, kinds=("ends",), max_frames=5).draw(50)
    assert all(bool(r[:(c + 1) // 2].all() and r[frames - c // 2:].all()) for r, c in zip(only, only.sum(1).tolist()))


def test_policy_shards_and_generators(backend, monkeypatch):
    """Two simulated ranks get the halves of the one-process mask; skip_step_draws keeps a rank in step; the default generator's state
    after a step is the same with the policy on and off."""
    dev = backend
    kw = dict(prob=1.0, max_frames=3, seed=11)
    shape, x0, noise, fea, t = _stub_inputs(dev, b=4)
    seen = []
    real = ops.train_qsample
    monkeypatch.setattr(ops, "train_qsample", lambda *a, **k: (seen.append(k["frame_mask"].cpu().clone()), real(*a, **k))[1])

    rng_state = (lambda: torch.cuda.get_rng_state()) if dev == "cuda" else torch.get_rng_state       # the generator the step draws from

    def step(d, lo=0, hi=4):
        d(x0[lo:hi], fea[lo:hi], None)
        return seen.pop()

    torch.manual_seed(1)
    one = _stub_diffusion(dev, known_train=kw)
    whole = [step(one), step(one), step(one)]
    state_on = rng_state()
    ranks = []
    for r in range(2):
        torch.manual_seed(1)
        d = _stub_diffusion(dev, known_train=kw)
        d.rank_shard = (r, 2)
        got = [step(d, 2 * r, 2 * r + 2)]
        d.skip_step_draws(4, shape[1:], dev)                        # (a step this rank sits out)
        got.append(step(d, 2 * r, 2 * r + 2))
        ranks.append(got)
        assert torch.equal(rng_state(), state_on)        # in step on the default generator too
    for r in range(2):
        assert torch.equal(ranks[r][0], whole[0][2 * r:2 * r + 2])
        assert torch.equal(ranks[r][1], whole[2][2 * r:2 * r + 2])
    torch.manual_seed(1)
    off = _stub_diffusion(dev)
    for _ in range(3):
        off(x0, fea, None)
    assert torch.equal(rng_state(), state_on)
    assert "known" not in "".join(one.state_dict())


def test_trainer_flags_parse():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("train_dm", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "train_dm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.known_train(mod.parse_args([])) is None
    args = mod.parse_args(["--known-prob", "0.5", "--known-kinds", "prefix", "ends", "--known-max-frames", "4", "--known-seed", "9"])
    assert mod.known_train(args) == dict(prob=0.5, kinds=("prefix", "ends"), max_frames=4, seed=9)
