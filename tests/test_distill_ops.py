"""Progressive distillation: the two kernels of csrc/distill.hip at the edges of their launch plan, on both backends
("emu": index logic on a GPU-less machine; "hip": the device).

Launch plan (train_elem_core.h): grid (workgroups of a sample, B), 256 lanes, 4 float4 per lane and trip, at most 64 workgroups per sample.
The shapes are test_train_known.py's, for its reasons: 60 floats per sample (ragged, under one workgroup), one frame, the shipped shape and
(2, 3, 22, 64, 64) = 270 336 floats per sample, past the workgroup cap into the grid-stride loop.  Rows per sample differ and include row
0 and the last row.  Tables: the "pred_v" and "pred_x0" tables `distill_tables` makes, and a "generic" table with every column non-zero
(k_eps too: the branch the two objectives never take).  Every destination is handed over NaN-filled.

Bars, per element, with E = 2^-24; references are float64 on the fp32-rounded tables and the fp32 thr:
  distill_x0    torch.equal to the eager fp32 expression where both coefficients are non-zero; for "pred_x0" rows the bits of out
  x_next        8 E S,  S = |k_x0| (|c_x x| + |c_eps out|) / s + |k_eps out| + |k_x x|: at most seven roundings, contracted or not
  x_target      8 E (|q0| S + |q0 v| + |q1 x_ref|)
  eps_target    8 E (|q2 x_ref| + |q3| (|xt| + bar of xt)) against q2 x_ref + q3 x_target in float64 ON THE x_target THE KERNEL STORED: the
                two are one pair - eps_target is the noise that this x_target implies - and |xt| + bar of xt bounds that stored value from
                the reference xt.  Against the float64 chain from the inputs the error of x_target comes through times q3 on top of that:
                the second check, at the bar above + |q3| (bar of xt) - where xt cancels it is far above 8 E |q3 xt|."""
import functools

import pytest
import torch

from cvpr23_lfdm_amd import GaussianDiffusion, ops
from util import rnd

NAN = float("nan")
E = 2.0 ** -24
SHAPES = [(3, 3, 5, 2, 2), (2, 3, 1, 4, 4), (2, 3, 40, 32, 32), (2, 3, 22, 64, 64)]
KINDS = ["pred_v", "pred_x0", "generic"]
STEPS = 4           # student steps of the tables: 8 teacher rows, 4 target rows


def _nan(shape, dev):
    return torch.full(tuple(shape), NAN, dtype=torch.float32, device=dev)


@functools.lru_cache(maxsize=None)
def _tables(kind):
    """(coef (8, 6), tcoef (4, 4)) fp32."""
    if kind == "generic":
        g = torch.Generator().manual_seed(9)
        sign = lambda *s: torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)
        return (torch.rand(2 * STEPS, 6, generator=g) + 0.25) * sign(2 * STEPS, 6), (torch.rand(STEPS, 4, generator=g) + 0.25) * sign(STEPS, 4)
    d = GaussianDiffusion(torch.nn.Identity(), image_size=8, num_frames=4, timesteps=1000, sampling_timesteps=10, loss_type="l2",
                          objective=kind, schedule="cosine_zsnr", step_grid="trailing")
    tabs = d.distill_tables(STEPS)
    return tabs["teacher_coef"], tabs["target_coef"]


@functools.lru_cache(maxsize=None)
def _case(shape, kind, with_thr):
    """Inputs and the float64 references with their bars, computed once and shared (never written)."""
    b = shape[0]
    coef, tcoef = _tables(kind)
    x, out, x_ref = rnd(*shape, seed=31) * 1.5, rnd(*shape, seed=32) * 1.5, rnd(*shape, seed=33)
    row = torch.tensor([0, 2 * STEPS - 1, 3][:b])
    trow = torch.tensor([0, STEPS - 1, 1][:b])
    thr = torch.tensor([0.5, 2.25, 1.5][:b]) if with_thr else None           # one below 1 (clamped up to 1) and one above
    shp = (b, 1, 1, 1, 1)
    c = [coef[row][:, j].double().reshape(shp) for j in range(6)]
    q = [tcoef[trow][:, j].double().reshape(shp) for j in range(4)]
    x64, o64, r64 = x.double(), out.double(), x_ref.double()
    s = (thr.double().clamp(min=1.0) if with_thr else torch.ones(b, dtype=torch.float64)).reshape(shp)
    x0 = c[0] * x64 - c[1] * o64
    m = torch.minimum(torch.maximum(x0, -s), s) / s
    v = c[2] * m + c[3] * o64 + c[4] * x64
    big_s = c[2].abs() * ((c[0] * x64).abs() + (c[1] * o64).abs()) / s + (c[3] * o64).abs() + (c[4] * x64).abs()
    xt = q[0] * v + q[1] * r64
    bar_xt = 8 * E * (q[0].abs() * big_s + (q[0] * v).abs() + (q[1] * r64).abs())
    et = q[2] * r64 + q[3] * xt
    bar_et = 8 * E * ((q[2] * r64).abs() + q[3].abs() * (xt.abs() + bar_xt))
    cx, ce = coef[row][:, 0].reshape(shp), coef[row][:, 1].reshape(shp)
    return dict(x=x, out=out, x_ref=x_ref, row=row, trow=trow, thr=thr, coef=coef, tcoef=tcoef, x0_eager=cx * x - ce * out,
                v=v, bar_v=8 * E * big_s, xt=xt, bar_xt=bar_xt, et=et, bar_et=bar_et, q2r=q[2] * r64, q3=q[3])


def _within(got, want, bar, what):
    err = (got.cpu().double() - want).abs()
    worst = float((err / bar.clamp(min=1e-300)).max())
    print("%s: largest error / bar = %.3g" % (what, worst))
    assert not torch.isnan(got).any(), what
    assert bool((err <= bar).all()), "%s: largest error / bar = %.3g" % (what, worst)


def _params():
    return [pytest.param(shape, kind, id="%s-%s" % ("x".join(map(str, shape)), kind)) for shape in SHAPES for kind in KINDS]


@pytest.mark.parametrize("shape,kind", _params())
def test_distill_x0(backend, shape, kind):
    dev, case = backend, _case(shape, kind, False)
    args = [case[k].to(dev) for k in ("out", "coef", "row")]
    got = ops.distill_x0(case["x"].to(dev), *args, x0=_nan(shape, dev))
    if kind == "pred_x0":           # rows {0, -1}: the bits of out, and x is never read
        assert torch.equal(got.cpu(), case["out"])
        assert torch.equal(ops.distill_x0(_nan(shape, dev), *args, x0=_nan(shape, dev)), got)
    else:
        both = (case["coef"][case["row"]][:, :2] != 0).all(dim=1)
        assert int(both.sum()) >= 1         # ("pred_v" on the zero-SNR node, sample 0: c_x = a = 0 - with a finite x the eager bits all the same)
        assert torch.equal(got.cpu(), case["x0_eager"])
        if not bool(both[0]):
            poisoned = case["x"].clone()
            poisoned[0] = NAN
            assert torch.equal(ops.distill_x0(poisoned.to(dev), *args), got)
    assert torch.equal(got, ops.distill_x0(case["x"].to(dev), *args)), "two runs on the same inputs differ"


@pytest.mark.parametrize("with_thr", [False, True], ids=["static", "thr"])
@pytest.mark.parametrize("shape,kind", _params())
def test_distill_step(backend, shape, kind, with_thr):
    dev, case = backend, _case(shape, kind, with_thr)
    x, out, coef, row = (case[k].to(dev) for k in ("x", "out", "coef", "row"))
    thr = None if case["thr"] is None else case["thr"].to(dev)
    tkw = dict(x_ref=case["x_ref"].to(dev), tcoef=case["tcoef"].to(dev), trow=case["trow"].to(dev))
    plain = ops.distill_step(x, out, coef, row, thr, _nan(shape, dev))
    _within(plain, case["v"], case["bar_v"], "x_next")

    def run(with_next):
        return ops.distill_step(x, out, coef, row, thr, _nan(shape, dev) if with_next else None, x_target=_nan(shape, dev),
                                eps_target=_nan(shape, dev), **tkw)

    x_next, x_target, eps_target = run(True)
    assert torch.equal(x_next, plain)
    _within(x_target, case["xt"], case["bar_xt"], "x_target")
    _within(eps_target, case["q2r"] + case["q3"] * x_target.cpu().double(), case["bar_et"], "eps_target of the stored x_target")
    _within(eps_target, case["et"], case["bar_et"] + case["q3"].abs() * case["bar_xt"], "eps_target of the inputs")
    again = run(True)
    assert all(torch.equal(a, b) for a, b in zip((x_next, x_target, eps_target), again)), "two runs on the same inputs differ"
    none, xt2, et2 = run(False)             # v never stored: the same targets
    assert none is None and torch.equal(xt2, x_target) and torch.equal(et2, eps_target)
    if kind == "pred_x0" and shape == SHAPES[0]:        # the last row has k_x = 0 next to c_x = 0: sample 1 never reads x
        poisoned = x.clone()
        poisoned[1] = NAN
        assert torch.equal(ops.distill_step(poisoned, out, coef, row, thr)[1], plain[1])


@pytest.mark.parametrize("kind", KINDS)
def test_distill_step_in_place(backend, kind):
    """x_next is x, without a target: accepted and the bits of the out-of-place call."""
    dev, shape = backend, SHAPES[0]
    case = _case(shape, kind, True)
    x, out, coef, row, thr = (case[k].to(dev) for k in ("x", "out", "coef", "row", "thr"))
    want = ops.distill_step(x, out, coef, row, thr)
    work = x.clone()
    assert ops.distill_step(work, out, coef, row, thr, work) is work
    assert torch.equal(work, want)
    _within(work, case["v"], case["bar_v"], "x_next in place")


@pytest.mark.parametrize("kind", ["pred_v", "generic"])
def test_row_out_of_range_is_clamped(backend, kind):
    """The tables sit between NaN rows (tests/layout.py's guard rows): a row index outside the table is clamped, not followed."""
    dev, shape = backend, SHAPES[0]
    case = _case(shape, kind, False)

    def guarded(tab):
        wide = _nan((tab.shape[0] + 2, tab.shape[1]), dev)
        wide[1:-1] = tab.to(dev)
        return wide[1:-1]

    coef, tcoef = guarded(case["coef"]), guarded(case["tcoef"])
    assert coef.is_contiguous() and tcoef.is_contiguous()
    x, out, x_ref = (case[k].to(dev) for k in ("x", "out", "x_ref"))
    wild = torch.tensor([-5, 2 * STEPS, 1 << 40], device=dev)
    edge = torch.tensor([0, 2 * STEPS - 1, 2 * STEPS - 1], device=dev)
    twild, tedge = torch.tensor([-1, STEPS, 1 << 33], device=dev), torch.tensor([0, STEPS - 1, STEPS - 1], device=dev)
    got_x0, want_x0 = ops.distill_x0(x, out, coef, wild), ops.distill_x0(x, out, coef, edge)
    assert torch.isfinite(got_x0).all() and torch.equal(got_x0, want_x0)
    got = ops.distill_step(x, out, coef, wild, None, _nan(shape, dev), x_ref=x_ref, tcoef=tcoef, trow=twild)
    want = ops.distill_step(x, out, coef, edge, None, _nan(shape, dev), x_ref=x_ref, tcoef=tcoef, trow=tedge)
    for a, b in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_refusals(backend):
    """Python-side refusals raise ValueError; the C entry points refuse with LFDM_EINVAL (-1) for themselves; nothing is written."""
    dev, shape = backend, SHAPES[0]
    case = _case(shape, "pred_v", True)
    x, out, x_ref, coef, tcoef, row, trow, thr = (case[k].to(dev) for k in ("x", "out", "x_ref", "coef", "tcoef", "row", "trow", "thr"))
    dst = [_nan(shape, dev) for _ in range(3)]
    with pytest.raises(ValueError, match="go together"):
        ops.distill_step(x, out, coef, row, thr, dst[0], x_ref=x_ref, tcoef=tcoef)
    with pytest.raises(ValueError, match="go together"):
        ops.distill_step(x, out, coef, row, thr, dst[0], x_target=dst[1])
    with pytest.raises(ValueError, match="int64"):
        ops.distill_step(x, out, coef, row.int(), thr, dst[0])
    with pytest.raises(ValueError, match="int64"):
        ops.distill_x0(x, out, coef, row[:2], dst[0])
    with pytest.raises(ValueError, match="table"):
        ops.distill_x0(x, out, coef[:, :4].contiguous(), row, dst[0])
    with pytest.raises(ValueError, match="thr"):
        ops.distill_step(x, out, coef, row, thr[:2], dst[0])
    with pytest.raises(ValueError, match="shape"):
        ops.distill_step(x, out[:2], coef, row, thr, dst[0])
    with pytest.raises(RuntimeError, match="x_ref must not alias"):
        ops.distill_step(x, out, coef, row, thr, dst[0], x_ref=dst[1], tcoef=tcoef, trow=trow, x_target=dst[1], eps_target=dst[2])
    with pytest.raises(RuntimeError, match="x_ref must not alias"):
        ops.distill_step(x, out, coef, row, thr, dst[0], x_ref=dst[0], tcoef=tcoef, trow=trow, x_target=dst[1], eps_target=dst[2])
    with pytest.raises(RuntimeError, match="must not alias each other"):
        ops.distill_step(x, out, coef, row, thr, dst[0], x_ref=x_ref, tcoef=tcoef, trow=trow, x_target=dst[1], eps_target=dst[1])
    with pytest.raises(RuntimeError, match="x_next must not alias out"):
        ops.distill_step(x, out, coef, row, thr, out)
    odd = torch.zeros(3, 3, 1, 1, 2, device=dev)                                   # n = 6: no multiple of 4
    with pytest.raises(RuntimeError, match="n % 4"):
        ops.distill_x0(odd, odd, coef, row, _nan(odd.shape, dev))
    with pytest.raises(RuntimeError, match="n % 4"):
        ops.distill_step(odd, odd, coef, row, None, _nan(odd.shape, dev))
    lib = ops._lib()
    p, n, st = ops._p, x[0].numel(), ops._stream(lib)
    shifted = torch.zeros(x.numel() + 4, device=dev)[1:1 + x.numel()]              # 4 bytes off a 16-byte boundary
    assert shifted.data_ptr() % 16 != 0
    bad_step = [
        (None, p(out), p(coef), p(row), 8, None, p(dst[0]), None, None, None, 0, None, None, 3, n),                        # null x
        (p(x), p(out), p(coef), p(row), 8, None, None, None, None, None, 0, None, None, 3, n),                             # no output at all
        (p(shifted), p(out), p(coef), p(row), 8, None, p(dst[0]), None, None, None, 0, None, None, 3, n),                  # misaligned x
        (p(x), p(out), p(coef), p(row), 8, None, p(dst[0]), p(x_ref), p(tcoef), p(trow), 4, p(dst[1]), None, 3, n),        # partial target set
        (p(x), p(out), p(coef), p(row), 8, None, p(dst[0]), None, None, None, 4, None, None, 3, n),                        # trows without target
        (p(x), p(out), p(coef), p(row), 8, None, p(dst[0]), p(x_ref), p(tcoef), p(trow), 0, p(dst[1]), p(dst[2]), 3, n),   # target without trows
        (p(x), p(out), p(coef), p(row), 0, None, p(dst[0]), None, None, None, 0, None, None, 3, n),                        # rows = 0
        (p(x), p(out), p(coef), p(row), 8, None, p(dst[0]), None, None, None, 0, None, None, 0, n),                        # batch = 0
        (p(x), p(out), p(coef), p(row), 8, None, p(dst[0]), None, None, None, 0, None, None, 3, 1 << 24),                  # n = 2^24
        (p(x), p(out), p(coef), p(row), 8, None, p(dst[0]), None, None, None, 0, None, None, 3, 0),                        # n = 0
    ]
    for args in bad_step:
        assert lib.lfdm_distill_step_f32(*args, st) == -1 and b"distill_step" in lib.lfdm_last_error(), args
    bad_x0 = [
        (p(x), None, p(coef), p(row), 8, p(dst[0]), 3, n),
        (p(x), p(out), p(coef), p(row), 8, p(shifted), 3, n),
        (p(x), p(out), p(coef), p(row), 8, p(out), 3, n),
        (p(x), p(out), p(coef), p(row), -1, p(dst[0]), 3, n),
        (p(x), p(out), p(coef), p(row), 8, p(dst[0]), 70000, n),
        (p(x), p(out), p(coef), p(row), 8, p(dst[0]), 3, n + 2),
    ]
    for args in bad_x0:
        assert lib.lfdm_distill_x0_f32(*args, st) == -1 and b"distill_x0" in lib.lfdm_last_error(), args
    if dev == "cuda":
        torch.cuda.synchronize()
    assert all(bool(torch.isnan(d).all()) for d in dst)                            # a refused call writes nothing
    assert bool((shifted == 0).all()) and torch.equal(out, case["out"].to(dev))
