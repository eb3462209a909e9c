"""ops.cfg_combine_rescale (csrc/sampler.hip: cfg_rescale_stats_kernel + cfg_rescale_apply_kernel) against a float64 torch
restatement, on both backends.  out, factor_out and ws are handed over NaN-filled.

Bars, derived (u = 2^-24, the unit roundoff of fp32):
  factor   |factor - factor64| <= 4 u factor64: one rounding of a double result (1 u), and the effect of g's three fp32 roundings on a
           standard deviation over >= 2 elements - the double sums themselves err at 2^-53 per term and do not show.
  output   |out - out64| <= 8 u factor64 (|null| + |scale| |cond - null|), per element: three roundings in g (difference, product, sum -
           each at most u times a term bounded by |null| + |scale| |cond - null|), one in the factor, one in the product, with slack 8 / 5.
Every check prints its fraction of each bar (pytest -s); the largest on the MI355X are in profiles/guidance_margins.txt.

Shapes: launch A runs G = min(ceil(n / 1024), 256) workgroups of 256 threads, four elements per thread and trip.  n = 1023 / 1024 / 1025 sit
either side of one workgroup's full trip; G reaches its cap at n = 262144 = 256 * 1024, which is also the largest n the grid covers in ONE
trip of its grid-stride loop: n = 262143 / 262145 sit either side of both."""
import os

import pytest
import torch

from cvpr23_lfdm_amd import ops

U = 2.0 ** -24
CAP_N = 256 * 1024
SHAPES = [2, 3, 4, 5, 255, 256, 257, 768, 1023, 1024, 1025, 122880, CAP_N - 1, CAP_N, CAP_N + 1]


def _inputs(batch, n, seed=0, offset=0.0, null_sigma=0.6, null_mean=0.3):
    g = torch.Generator().manual_seed(1000 * seed + n % 997 + batch)
    cond = offset + torch.randn(batch, n, generator=g)
    null = offset + null_sigma * torch.randn(batch, n, generator=g) + null_mean
    return cond.float(), null.float()


def reference(cond, null, scale, phi):
    """float64 from the fp32 operands: (out64, factor64, bound of g's terms)."""
    c, a = cond.double(), null.double()
    g = a + (c - a) * scale
    std_c, std_g = c.std(dim=1, unbiased=True), g.std(dim=1, unbiased=True)
    factor = torch.where(std_g == 0, torch.ones_like(std_g), phi * std_c / std_g + (1.0 - phi))
    return g * factor[:, None], factor, a.abs() + abs(scale) * (c - a).abs()


def run(dev, cond, null, scale, phi, out=None, misalign=False):
    """-> (out, factor) on the host; out / factor_out / ws NaN-filled before the call.  misalign: every operand one element off a
    16-byte boundary (the element path)."""
    batch, n = cond.shape
    nan = lambda *size: torch.full(size, float("nan"), device=dev)

    def place(t):
        if not misalign:
            return t.to(dev).contiguous()
        buf = nan(batch * n + 1)
        view = buf[1:].view(batch, n)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4
        return view

    c, a = place(cond), place(null)
    if out is None:
        o = place(torch.full((batch, n), float("nan")))
    else:
        o = {"cond": c, "null": a}[out]
    factor = nan(batch)
    ws = torch.full((ops.cfg_rescale_ws(batch, n, dev).numel(),), float("nan"), dtype=torch.float64, device=dev)
    ops.cfg_combine_rescale(c, a, scale, phi, o, ws=ws, factor_out=factor)
    return o.cpu().clone(), factor.cpu().clone()


def check(what, got, factor, cond, null, scale, phi):
    out64, f64, terms = reference(cond, null, scale, phi)
    assert torch.isfinite(got).all() and torch.isfinite(factor).all(), what
    f_err = (factor.double() - f64).abs() / (4 * U * f64)
    o_bar = 8 * U * f64[:, None] * terms
    o_err = ((got.double() - out64).abs() / o_bar.clamp(min=1e-300)).max()
    print("%s: factor %s (float64 %s), %.3f of the factor bar, %.3f of the output bar" % (what, factor.tolist(), f64.tolist(), float(f_err.max()), float(o_err)))
    assert float(f_err.max()) <= 1.0, "%s: factor %s against %s" % (what, factor.tolist(), f64.tolist())
    assert bool(((got.double() - out64).abs() <= o_bar).all()), "%s: %.3f of the output bar" % (what, float(o_err))


@pytest.mark.parametrize("n", SHAPES)
def test_rescale_against_float64(backend, n):
    dev = backend
    batches = (1, 2, 3) if n <= 1025 else (1,) if n > 122880 else (1, 2)
    combos = [(2.0, 0.25), (7.5, 0.7), (2.0, 1.0), (7.5, 1.0)] if n <= 1025 else [(7.5, 0.7)]
    for batch in batches:
        cond, null = _inputs(batch, n)
        for scale, phi in combos:
            got, factor = run(dev, cond, null, scale, phi)
            check("rescale n=%d batch=%d scale=%g phi=%g" % (n, batch, scale, phi), got, factor, cond, null, scale, phi)


def test_factor_is_far_from_one_at_scale_7p5(backend):
    cond, null = _inputs(1, 122880)
    _, factor = run(backend, cond, null, 7.5, 1.0)
    assert 0.1 < float(factor) < 0.2          # std(cond) / std(g): about 0.15


@pytest.mark.parametrize("n", [5, 768, 1025, 4099])
@pytest.mark.parametrize("batch", [1, 2])
def test_rescale_element_path(backend, n, batch):
    """Bases one element off a 16-byte boundary: the element path, the same bars - and the same bits as the aligned call (a thread adds the
    same elements in the same order on both paths)."""
    cond, null = _inputs(batch, n, seed=2)
    got, factor = run(backend, cond, null, 7.5, 0.7, misalign=True)
    check("element path n=%d batch=%d" % (n, batch), got, factor, cond, null, 7.5, 0.7)
    got0, factor0 = run(backend, cond, null, 7.5, 0.7)
    assert torch.equal(got, got0) and torch.equal(factor, factor0)


@pytest.mark.parametrize("n", [3, 768, 1025, 122880])
def test_phi_zero_is_cfg_combine(backend, n):
    dev = backend
    cond, null = _inputs(2, n, seed=3)
    for scale in (2.0, 7.5):
        got, factor = run(dev, cond, null, scale, 0.0)
        want = ops.cfg_combine(cond.to(dev), null.to(dev), scale, torch.empty(2, n, device=dev)).cpu()
        assert torch.equal(factor, torch.ones(2)) and torch.equal(got, want)


def test_ill_conditioned_mean(backend):
    """cond = 1000 + N(0, 1), null = 1000 + 0.5 N(0, 1), n = 122880: sum x^2 is 1.2e11 against (n - 1) var = 1.2e5, six digits cancel in
    sum x^2 - (sum x)^2 / n, so neither an fp32 accumulation nor an fp32 variance can hold the factor bar of 2.4e-7.  Checked on the CPU
    with fp32 restatements of the kernel's formulas on these inputs (scale 2, phi 0.7: factor64 = 0.639696; scale 7.5, phi 1: 0.122425):
        fp32 sums (torch.sum: a pairwise tree, the best case) and fp32 variance    0.638886 / 0.122291    5310 / 4576 bars
        double sums, the variance formed in fp32                                   0.641565 / 0.122536   12256 / 3803 bars
        sequential fp32 sums (cumsum), the variance formed in double               0.637094 / 0.120511   17062 / 65566 bars"""
    cond, null = _inputs(1, 122880, seed=4, offset=1000.0, null_sigma=0.5, null_mean=0.0)
    for scale, phi in ((2.0, 0.7), (7.5, 1.0)):
        got, factor = run(backend, cond, null, scale, phi)
        check("ill-conditioned n=122880 scale=%g phi=%g" % (scale, phi), got, factor, cond, null, scale, phi)


@pytest.mark.parametrize("n", [2, 1025])
def test_constant_operands(backend, n):
    """cond == null constant: std(g) = 0, the factor is 1, out == g bit for bit, nothing is NaN."""
    dev = backend
    cond = torch.full((2, n), 0.37)
    got, factor = run(dev, cond, cond.clone(), 7.5, 0.7)
    want = ops.cfg_combine(cond.to(dev), cond.to(dev), 7.5, torch.empty(2, n, device=dev)).cpu()
    assert torch.equal(factor, torch.ones(2)) and torch.equal(got, want) and torch.isfinite(got).all()


@pytest.mark.parametrize("n", [5, 1025, 4096])
@pytest.mark.parametrize("alias", ["cond", "null"])
def test_out_may_alias_an_operand(backend, n, alias):
    cond, null = _inputs(2, n, seed=5)
    want, f0 = run(backend, cond, null, 2.0, 0.7)
    got, f1 = run(backend, cond, null, 2.0, 0.7, out=alias)
    assert torch.equal(got, want) and torch.equal(f0, f1)


@pytest.mark.parametrize("n", [5, 768, 4099, 122880])
def test_a_sample_does_not_depend_on_its_batch(backend, n):
    """Sample i of a batch of 3 has the bits of the same sample run alone (n = 5, 4099: samples 1 and 2 of the batch start off a 16-byte
    boundary and take the element path, alone they take the wide one); and two runs give the same bits."""
    cond, null = _inputs(3, n, seed=6)
    got, factor = run(backend, cond, null, 7.5, 0.7)
    again, factor2 = run(backend, cond, null, 7.5, 0.7)
    assert torch.equal(got, again) and torch.equal(factor, factor2)
    for i in range(3):
        alone, f = run(backend, cond[i:i + 1], null[i:i + 1], 7.5, 0.7)
        assert torch.equal(alone[0], got[i]) and torch.equal(f[0], factor[i]), i


def test_refusals_touch_nothing(backend):
    dev = backend
    nan = lambda *size: torch.full(size, float("nan"), device=dev)
    cond, null = (t.to(dev) for t in _inputs(2, 8))
    out, factor = nan(2, 8), nan(2)
    ws = ops.cfg_rescale_ws(2, 8, dev)
    short = torch.empty(ws.numel() * 8 - 1, dtype=torch.uint8, device=dev)
    one, out1 = torch.ones(2, 1, device=dev), nan(2, 1)
    calls = [lambda: ops.cfg_combine_rescale(one, one, 2.0, 0.5, out1, ws=ws, factor_out=factor),           # n = 1
             lambda: ops.cfg_combine_rescale(one, one, 2.0, 0.5, out1, factor_out=factor),                  # ... and no workspace exists for it
             lambda: ops.cfg_combine_rescale(cond, null, 2.0, 0.5, out, ws=short, factor_out=factor),       # one byte short
             lambda: ops.cfg_combine_rescale(cond, null, 2.0, 1.5, out, ws=ws, factor_out=factor),
             lambda: ops.cfg_combine_rescale(cond, null, 2.0, float("nan"), out, ws=ws, factor_out=factor),
             lambda: ops.cfg_combine_rescale(cond, null[:1], 2.0, 0.5, out, ws=ws, factor_out=factor),
             lambda: ops.cfg_combine_rescale(cond[:, ::2], null[:, ::2], 2.0, 0.5, out[:, ::2], ws=ws)]
    for call in calls:
        with pytest.raises((RuntimeError, ValueError)):
            call()
    assert torch.isnan(out).all() and torch.isnan(out1).all() and torch.isnan(factor).all()
    with pytest.raises(RuntimeError, match="cfg_combine_rescale"):
        calls[2]()
    ops.cfg_combine_rescale(cond, null, 2.0, 0.5, out, ws=ws, factor_out=factor)         # and the call itself is fine
    assert torch.isfinite(out).all() and torch.isfinite(factor).all()


def test_header_declares_the_entry_points():
    import re
    from cvpr23_lfdm_amd import _native
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(repo, "include", "lfdm_hip.h")).read()
    assert {"lfdm_cfg_combine_rescale_f32", "lfdm_cfg_rescale_ws_bytes"} <= set(_native.EXPORTED_SYMBOLS)
    decl = re.search(r"/\* Layout:(?:[^*]|\*(?!/))*\*/\s*int lfdm_cfg_combine_rescale_f32\(([^;]*)\)\s*;", header)
    assert decl and "size_t lfdm_cfg_rescale_ws_bytes(int batch, int64_t n);" in header
    from test_operand_layouts import LD_NAMES
    assert not set(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", decl.group(1))) & LD_NAMES
