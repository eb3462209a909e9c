"""Progressive distillation: `GaussianDiffusion.distill_tables` - host only.  The tables are a pure function of the
registered buffers, in double from their fp32 values and rounded once."""
import math

import pytest
import torch

from cvpr23_lfdm_amd import GaussianDiffusion

T = 1000


def _diffusion(objective="pred_v", schedule="cosine", step_grid="trailing", **kw):
    kw.setdefault("sampling_timesteps", 10)
    return GaussianDiffusion(torch.nn.Identity(), image_size=8, num_frames=4, timesteps=T, loss_type="l2", objective=objective,
                             schedule=schedule, step_grid=step_grid, **kw)


@pytest.mark.parametrize("n", [1, 2, 4, 25, 500])
def test_student_nodes_are_the_even_teacher_nodes(n):
    tabs = _diffusion().distill_tables(n)
    assert tabs["teacher_times"].shape == (2 * n,) and tabs["student_times"].shape == (n,)
    assert tabs["teacher_coef"].shape == (2 * n, 6) and tabs["student_coef"].shape == (n, 6) and tabs["target_coef"].shape == (n, 4)
    assert tabs["weight"].shape == (T,)
    assert torch.equal(tabs["teacher_times"][0::2], tabs["student_times"])
    assert int(tabs["teacher_times"][0]) == T - 1 and tabs["teacher_times"].dtype == torch.int64
    assert all(v.dtype == torch.float32 for k, v in tabs.items() if not k.endswith("_times"))


@pytest.mark.parametrize("objective", ["pred_v", "pred_x0"])
@pytest.mark.parametrize("schedule", ["cosine", "cosine_zsnr"])
def test_rows(schedule, objective):
    d = _diffusion(objective, schedule, ddim_sampling_eta=0.7)          # (eta is not read: column 5 is zero whatever it holds)
    n = 4
    tabs = d.distill_tables(n)
    sc, tc, q, times = tabs["student_coef"], tabs["teacher_coef"], tabs["target_coef"], tabs["student_times"].tolist()
    assert bool((sc[:, 5] == 0).all()) and bool((tc[:, 5] == 0).all()) and bool((sc[:, 3] == 0).all()) and bool((tc[:, 3] == 0).all())
    assert float(q[-1, 0]) == 1.0 and float(q[-1, 1]) == 0.0            # the last student row lands on the clean end: z'' IS x_target
    a_tab, s_tab = d.sqrt_alphas_cumprod.double(), d.sqrt_one_minus_alphas_cumprod.double()
    if schedule == "cosine_zsnr":
        assert times[0] == T - 1 and float(a_tab[times[0]]) == 0.0 and float(q[0, 2]) == 1.0 and float(q[0, 3]) == 0.0
    # the student's rows in double, as distill_tables forms them: k_x0 = a' - s' a / s, k_x = s' / s on (a, s) of the node and (a', s') of the next
    rows64, times64, _ = d._trailing_ddim_rows(d.ddim_times(n), 0.0, {k: v.float() for k, v in d.named_buffers()}, steps=n)
    rows64 = d._objective_rows(times64, torch.stack(rows64), ddim_rows=True, rounded=False)
    assert times64 == times and rows64.dtype == torch.float64
    acp = d.alphas_cumprod.double()
    nxt = times[1:] + [-1]
    for i, (t, tn) in enumerate(zip(times, nxt)):
        a, s = float(a_tab[t]), float(s_tab[t])
        alpha_n = 1.0 if tn < 0 else float(acp[tn])
        a_n, s_n = math.sqrt(alpha_n), math.sqrt(1.0 - alpha_n)
        assert abs(float(rows64[i, 2]) - (a_n - s_n * a / s)) <= 1e-12
        assert abs(float(rows64[i, 4]) - s_n / s) <= 1e-12
        want = torch.tensor([1.0 / float(rows64[i, 2]), -float(rows64[i, 4]) / float(rows64[i, 2]), 1.0 / s, -a / s], dtype=torch.float64).float()
        assert torch.equal(q[i], want)           # rounded once
        assert torch.equal(sc[i, :2], (torch.tensor([a, s]) if objective == "pred_v" else torch.tensor([0.0, -1.0])).float())
    assert torch.equal(sc, rows64.float())
    # the rows the sampler itself makes for an N-step eta-0 model round the DDIM row to fp32 before `_objective_rows`: a last-place difference at most
    s_model = _diffusion(objective, schedule, sampling_timesteps=n, ddim_sampling_eta=0.0)
    times_s, coef_s, _ = s_model._step_tables(True)
    assert times_s == times
    assert bool(((coef_s.double() - sc.double()).abs() <= 2.0 ** -23 * sc.double().abs()).all())


def test_the_call_touches_nothing():
    d = _diffusion(ddim_sampling_eta=0.5)
    sch = d._schedule(True, "reference", torch.device("cpu"))
    keys, steps, eta = dict(d._schedules), d.sampling_timesteps, d.ddim_sampling_eta
    before = {k: v.clone() for k, v in d.named_buffers()}
    a, b = d.distill_tables(8), d.distill_tables(8)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert d._schedules == keys and d._schedule(True, "reference", torch.device("cpu")) is sch
    assert d.sampling_timesteps == steps and d.ddim_sampling_eta == eta
    assert all(torch.equal(v, before[k]) for k, v in d.named_buffers())
    assert len(d.state_dict()) == len([k for k in before if k != "loss_weight"])


def test_refusals():
    with pytest.raises(ValueError, match="pred_x0.*pred_v"):
        _diffusion("pred_noise").distill_tables(4)
    with pytest.raises(ValueError, match="step_grid='trailing'"):
        _diffusion(step_grid="reference").distill_tables(4)
    with pytest.raises(ValueError, match="per_element_loss=False"):
        _diffusion(per_element_loss=True).distill_tables(4)
    with pytest.raises(ValueError, match="known_train=None"):
        _diffusion(known_train=dict(prob=0.5, max_frames=2)).distill_tables(4)
    d = _diffusion()
    for bad in (0, -1, 501, 2.0, True, None):
        with pytest.raises(ValueError, match="student_steps"):
            d.distill_tables(bad)
    with pytest.raises(ValueError, match="distill_weight"):
        d.distill_tables(4, distill_weight="snr")
    small = GaussianDiffusion(torch.nn.Identity(), image_size=8, num_frames=4, timesteps=10, sampling_timesteps=5, loss_type="l2",
                              objective="pred_v", step_grid="trailing")
    small.distill_tables(5)
    with pytest.raises(ValueError, match="student_steps"):
        small.distill_tables(6)
    # set_distill refuses the same, and a teacher that is the student
    net = torch.nn.Linear(1, 1)
    d2 = GaussianDiffusion(net, image_size=8, num_frames=4, timesteps=T, sampling_timesteps=10, loss_type="l2")
    with pytest.raises(ValueError, match="pred_x0.*pred_v"):
        d2.set_distill(torch.nn.Linear(1, 1), 4)
    d3 = GaussianDiffusion(net, image_size=8, num_frames=4, timesteps=T, sampling_timesteps=10, loss_type="l2", objective="pred_v",
                           step_grid="trailing")
    with pytest.raises(ValueError, match="frozen copy"):
        d3.set_distill(net, 4)
    with pytest.raises(ValueError, match="guidance_rescale"):
        d3.set_distill(torch.nn.Linear(1, 1), 4, teacher_guidance_rescale=2.0)
    assert d3._distill is None


@pytest.mark.parametrize("objective", ["pred_v", "pred_x0"])
def test_weights(objective):
    d = _diffusion(objective, "cosine_zsnr", min_snr_gamma=5.0)
    acp = d.alphas_cumprod.double()
    snr = acp / (1.0 - acp)
    w = d.distill_tables(4)["weight"].double()
    at = lambda cond: int(torch.nonzero(cond)[0])
    zero, below, above = T - 1, at((snr > 0) & (snr < 1)), at(snr > 1)
    assert float(snr[zero]) == 0.0 and float(w[zero]) == 1.0            # the zero-SNR node: weight 1, where min-SNR gives 0
    assert float(d.loss_weight[zero]) == 0.0
    for t in (below, above):
        x0_weight = max(float(snr[t]), 1.0)
        want = x0_weight if objective == "pred_x0" else x0_weight / (float(snr[t]) + 1.0)
        assert float(w[t]) == float(torch.tensor(want, dtype=torch.float64).float())
    # snr == 1 exactly: an edited schedule (the tables follow the buffers)
    d.alphas_cumprod[7] = 0.5
    w1 = d.distill_tables(4)["weight"]
    assert float(w1[7]) == (1.0 if objective == "pred_x0" else 0.5)
    assert torch.equal(d.distill_tables(4, distill_weight="min_snr")["weight"], d.loss_weight)
    assert torch.equal(d.distill_tables(4, distill_weight=None)["weight"], torch.ones(T))
