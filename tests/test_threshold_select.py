"""The dynamic threshold s = max(1, quantile_q(|x0|)) of csrc/sampler.hip (three-pass radix select + ATen's lerp) against
torch.quantile(x.abs(), q, dim=-1) on the CPU, bit for bit (torch.equal, no tolerance: exactness is the project's own contract).

The select's control flow depends on the VALUES of a row - which 2048-bin histogram the two ranks fall in at each of the three levels,
whether they share it, what fraction lies between them - so the rows here are chosen by value:
  1. every rank class: each n = 1 .. 130 (all ten fractions 0.9 (n - 1) mod 1, the whole rank, lo == hi) and the sizes around one thread
     row, one workgroup and the step from one workgroup to two; other q at a few sizes; the largest accepted n on the GPU;
  2. neighbouring order statistics built from bit patterns, so that they differ across a level-0 bin, a level-1 bin, or inside one;
  3. ties at the rank;
  4. one workspace shared by abs_quantile and the sampler step;
  5. the threshold as every step entry point of ops uses it, with x0 = x bit for bit.
Every test first asserts that the oracle's abs_quantile equals torch.quantile on the same rows: a change on torch's side shows up as such.

Scope: rows hold finite values, except where +inf is placed strictly above the upper rank floor(q (n - 1)) + 1.  Rows with NaN, and
rows where one of the two order statistics (ranks floor(q (n - 1)) and the one above it) is itself infinite, are not tested: ATen
returns NaN there and the kernel does not."""
import numpy as np
import pytest
import torch

import lfdm_oracle as O
from util import rnd

Q = 0.9
INF_BITS = 0x7F800000


def ranks(n, q=Q):
    """(lo, lo + 1 clamped, fraction) of torch.quantile's position q (n - 1), evaluated in fp32 as ATen does."""
    pos = torch.tensor(q, dtype=torch.float32) * (n - 1)
    lo = int(pos.floor())
    return lo, min(lo + 1, n - 1), float(pos - pos.floor())


def check_rows(ops, dev, x, q=Q, what=""):
    """ops.abs_quantile(x) == torch.quantile(|x|) on every row; -> the reference."""
    ref = torch.quantile(x.abs(), q, dim=-1)
    assert torch.equal(O.abs_quantile(x, q), ref), "oracle quantile must equal torch.quantile bit for bit"
    out = ops.abs_quantile(x.to(dev).contiguous(), q).cpu()
    bad = (out != ref).nonzero().flatten().tolist()
    n = x.shape[1]
    assert torch.equal(out, ref), "%s n=%d q=%g (lo, hi, frac)=%s: rows %s differ, kernel %s, torch %s" % (
        what, n, q, ranks(n, q), bad, [out[i].item().hex() for i in bad[:4]], [ref[i].item().hex() for i in bad[:4]])
    return ref


# ------------------------------------------------------------------------------------------ 1. every rank class
def rank_class_rows(n):
    """16 rows: randn * 1.7; row 1 scaled by 1e-3, row 2 by 1e3, a third of row 3 set to 0.25, row 4 of two distinct values."""
    x = rnd(16, n, seed=1000 + n) * 1.7
    x[1] *= 1e-3
    x[2] *= 1e3
    x[3, : (n + 2) // 3] = 0.25
    x[4] = torch.where(x[4] > 0.3, torch.tensor(1.9), torch.tensor(-0.3))
    return x


SWEEP = list(range(1, 131)) + [255, 256, 257, 2047, 2048, 2049, 4096, 4097]


@pytest.mark.parametrize("n", SWEEP)
def test_every_rank_class(backend, n):
    """n = 255 / 256 / 257: one row of threads; 2047 / 2048 / 2049: eight elements per thread, then a second workgroup; 4096 / 4097: a third."""
    from cvpr23_lfdm_amd import ops
    check_rows(ops, backend, rank_class_rows(n), Q, "rank class")


@pytest.mark.parametrize("n", [1, 2, 7, 97, 2049])
@pytest.mark.parametrize("q", [0.0, 0.5, 0.995, 1.0])
def test_other_quantiles(backend, q, n):
    """The C entry point takes any q in [0, 1]; q = 1 reaches the clamp of the upper rank to n - 1."""
    from cvpr23_lfdm_amd import ops
    check_rows(ops, backend, rank_class_rows(n), q, "other q")


@pytest.mark.gpu
def test_largest_accepted_size():
    """n = 2^24 - 1, one row: half random, half one repeated value (one bin of every histogram holds eight million elements)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvpr23_lfdm_amd import _native, ops
    _native._set_library_for_tests(None)
    n = (1 << 24) - 1
    x = rnd(1, n, seed=24) * 1.7
    x[0, ::2] = -0.8125
    check_rows(ops, "cuda", x, Q, "largest size")


# ------------------------------------------------------------------------------------------ 2. constructed neighbours
PAIRS = {   # (bits at rank lo, bits at rank lo + 1 and above, [bits above rank lo + 1])
    "level0_bins_at_1": (0x3F7FFFFF, 0x3F800000),          # bits [31:21] differ
    "level0_bins_at_2": (0x3FFFFFFF, 0x40000000),
    "level1_bins": (0x3F8003FF, 0x3F800400),               # bits [31:21] equal, bits [20:10] differ
    "one_level1_bin_first": (0x3F800000, 0x3F800001),      # bits [31:10] equal
    "one_level1_bin_last": (0x3F8003FE, 0x3F8003FF),
    "equal": (0x3F800000, 0x3F800000),
    "zeros_of_both_signs": (0, 0),
    "denormals": (1, 2),
    "denormal_and_smallest_normal": (0x007FFFFF, 0x00800000),
    "largest_finite": (0x7F7FFFFE, 0x7F7FFFFF),
    "infinity_above": (0x3F8003FF, 0x3F800400, INF_BITS),
}


def row_from_sorted_bits(bits, seed):
    """The sorted magnitudes `bits` (uint32 patterns of non-negative floats) permuted, with random signs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bits = rng.permutation(np.asarray(bits, dtype=np.uint32))
    bits = bits | (rng.integers(0, 2, size=bits.shape, dtype=np.uint32) << np.uint32(31))
    return torch.from_numpy(bits.view(np.float32).copy())


def neighbour_row(n, lo_bits, hi_bits, top_bits, seed):
    lo, hi, _ = ranks(n)
    rng = np.random.Generator(np.random.PCG64(seed))
    bits = np.empty(n, dtype=np.uint32)
    bits[:lo] = np.sort(rng.integers(0, lo_bits, size=lo)) if lo_bits > 0 else 0      # non-negative floats order like their bit patterns
    bits[lo] = lo_bits
    bits[hi:] = hi_bits
    if top_bits is not None:
        bits[hi + 1:] = top_bits
    assert np.all(np.diff(bits.astype(np.int64)) >= 0) and (hi == lo or bits[hi] == hi_bits)
    return row_from_sorted_bits(bits, seed + 1)


@pytest.mark.parametrize("n", [11, 97, 192])
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_constructed_neighbours(backend, pair, n):
    """n = 11: whole rank (fraction 0), 97: fraction .4, 192: fraction .9.  Three permutations of each row."""
    from cvpr23_lfdm_amd import ops
    lo_bits, hi_bits = PAIRS[pair][:2]
    top_bits = PAIRS[pair][2] if len(PAIRS[pair]) > 2 else None
    x = torch.stack([neighbour_row(n, lo_bits, hi_bits, top_bits, seed) for seed in (n, n + 100, n + 200)])
    ref = check_rows(ops, backend, x, Q, pair)
    assert torch.isfinite(ref).all()


# ------------------------------------------------------------------------------------------ 3. ties at the rank
@pytest.mark.parametrize("n", [97, 192])
def test_ties_at_the_rank(backend, n):
    """Rows of one value; rows of two runs A < B whose boundary lies between the two ranks, one position below, one above."""
    from cvpr23_lfdm_amd import ops
    lo, hi, _ = ranks(n)
    rows = [torch.full((n,), v) for v in (0.0, -0.0, 0.25, 1.0)]
    a, b = np.float32(0.7).view(np.uint32), np.float32(1.9).view(np.uint32)
    for count_a in (hi, hi - 1, hi + 1):                                  # = lo + 1: A at lo, B at hi; both B; both A
        bits = np.full(n, b, dtype=np.uint32)
        bits[:count_a] = a
        rows.append(row_from_sorted_bits(bits, count_a))
    ref = check_rows(ops, backend, torch.stack(rows), Q, "ties")
    assert ref[:4].tolist() == [0.0, 0.0, 0.25, 1.0] and ref[5].item() == np.float32(1.9) and ref[6].item() == np.float32(0.7)
    assert np.float32(0.7) < ref[4].item() < np.float32(1.9)


# ------------------------------------------------------------------------------------------ 4. workspace reuse
DDIM_ROW = [1.0, 0.0, 0.8, 0.3, 0.0, 0.4]        # {c_x, c_eps, k_x0, k_eps, k_x, k_noise}: c_x = 1, c_eps = 0 make x0 = x bit for bit
DDPM_ROW = [1.0, 0.0, 0.6, 0.0, 0.5, 0.2]
MS_ROW = [1.0, 0.0, 0.8125, 0.37, 0.0, 0.0]      # {c_x, c_eps, k_x, k_m, k_prev, -}: a first-order step, the history is not read


def table_of(row):
    return torch.tensor([[9.0] * 6, row, [9.0] * 6])


@pytest.mark.parametrize("batch", [2, 3])
def test_workspace_reuse(backend, batch):
    """abs_quantile, a sampler step, abs_quantile, a step - on ONE workspace, every call on other data - equal the same calls on a fresh
    workspace each.  batch 2: the update kernel clears the histograms itself; batch 3: the clearing launch stays."""
    from cvpr23_lfdm_amd import ops
    dev, n = backend, 192
    data = [rnd(batch, n, seed=40 + i) * (0.6 + 0.5 * i) for i in range(4)]
    eps, noise = rnd(batch, n, seed=50), rnd(batch, n, seed=51)
    table = table_of(DDIM_ROW).to(dev)

    def run(shared):
        ws = ops.sampler_ws(batch, n, dev) if shared else None
        outs = []
        for i, x in enumerate(data):
            if i % 2 == 0:
                outs.append(ops.abs_quantile(x.to(dev), Q, ws=ws).cpu())
            else:
                xd, x0_out, step = x.clone().to(dev), torch.empty(batch, n).to(dev), torch.tensor([1], dtype=torch.int32).to(dev)
                ops.sampler_step(xd, eps.to(dev), noise.to(dev), table, step, quantile=Q, x0_out=x0_out, ws=ws)
                outs += [x0_out.cpu(), xd.cpu()]
        return outs

    shared, fresh = run(True), run(False)
    for i, (a, b) in enumerate(zip(shared, fresh)):
        assert torch.equal(a, b), "call result %d on the shared workspace differs from the fresh one" % i
    assert torch.equal(shared[0], torch.quantile(data[0].abs(), Q, dim=-1)) and torch.equal(shared[3], torch.quantile(data[2].abs(), Q, dim=-1))
    assert torch.equal(shared[1], O.dynamic_threshold(data[1])) and torch.equal(shared[4], O.dynamic_threshold(data[3]))


# ------------------------------------------------------------------------------------------ 5. the threshold inside the step kernels
KINDS = ("below_floor", "exactly_one", "above_tied", "above_lerp")


def threshold_row(kind, n, seed):
    """One row and the indices whose value is exactly +-s, s = max(1, quantile) of the finished row.
    No element can equal a threshold that lies strictly between two neighbouring order statistics, so elements are forced to +-s where
    that leaves s what it was: the floor s = 1 above a quantile < 1 (below_floor: elements above the upper rank become +-1), and rows
    whose two order statistics coincide (exactly_one at 1.0; above_tied at the threshold torch computes for the unforced row, which
    lies between them).  above_lerp rows are left alone: there the interpolation decides s."""
    lo, hi, _ = ranks(n)
    g = torch.Generator().manual_seed(seed)
    mags = (torch.randn(n, generator=g).abs() * (0.2 if kind == "below_floor" else 1.7)).sort().values
    if kind == "below_floor":
        mags.clamp_(max=0.96875)
        mags[hi + 1:] = 1.0
        forced = range(hi + 1, n)
    elif kind == "exactly_one":
        mags[:lo] = mags[:lo].clamp(max=0.96875)
        mags[lo:hi + 1] = 1.0
        mags[hi + 1:] += 1.0
        forced = range(lo, hi + 1)
    else:
        mags[lo:] += 1.0                                           # s > 1 whatever the draw
        forced = range(0)
        if kind == "above_tied":
            s = torch.quantile(mags, Q)
            assert mags[lo] <= s <= mags[hi]
            mags[lo:min(hi + 3, n)] = s                            # the two ranks and up to two elements above them
            forced = range(lo, min(hi + 3, n))
    perm = torch.randperm(n, generator=g)
    sign = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    row = torch.empty(n)
    row[perm] = mags
    row *= sign
    s = torch.quantile(row.abs(), Q).clamp_min(1.0)
    assert {"below_floor": s == 1.0 and mags[hi] < 1.0, "exactly_one": s == 1.0 and mags[hi] == 1.0}.get(kind, s > 1.0), (kind, n, s)
    idx = perm[list(forced)]
    assert bool((row[idx].abs() == s).all())
    return row, idx


KNOWN_SHAPE = {2: (2, 1), 7: (7, 1), 192: (12, 16), 3072: (12, 256)}     # (C * T, hw) with C * T a multiple of the four / two / seven frames
KNOWN_FRAMES = {2: 2, 7: 7, 192: 4, 3072: 4}


@pytest.mark.parametrize("n", [2, 7, 192, 3072])
@pytest.mark.parametrize("batch", [1, 2, 3])
@pytest.mark.parametrize("entry", ["ddim", "ddpm", "ms", "known", "counter"])
def test_threshold_in_the_step(backend, entry, batch, n):
    """x0_out of every step entry point == O.dynamic_threshold(x) bit for bit (c_x = 1, c_eps = 0: x0 is x), elements at +-s come out as
    +-1 exactly, the updated x within 1e-5 of a double model (its multiply-adds may be contracted).  Row b of rotation r is of kind
    (b + r) mod 4, so every batch size sees every kind at every row.  n = 3072: the single-frame latent 3 x 1 x 32 x 32."""
    from cvpr23_lfdm_amd import ops
    dev = backend
    eps, noise = rnd(batch, n, seed=61), rnd(batch, n, seed=62)
    for rot in range(4):
        built = [threshold_row(KINDS[(b + rot) % 4], n, 1000 * n + 10 * rot + b) for b in range(batch)]
        x = torch.stack([r for r, _ in built])
        m = O.dynamic_threshold(x)
        s_ref = torch.quantile(x.abs(), Q, dim=-1).clamp_min(1.0)
        assert torch.equal(O.abs_quantile(x, Q).clamp_min(1.0), s_ref), "oracle quantile must equal torch.quantile bit for bit"
        shape = (batch,) + KNOWN_SHAPE[n] if entry == "known" else (batch, n)
        xd, x0_out = x.clone().view(shape).to(dev), torch.full(shape, float("nan")).to(dev)
        step = torch.tensor([1], dtype=torch.int32).to(dev)
        x64, m64 = x.double(), m.double()
        if entry == "ms":
            hist = torch.full(shape, float("nan")).to(dev)
            ops.sampler_step_ms(xd, eps.to(dev), hist, table_of(MS_ROW).to(dev), step, quantile=Q, x0_out=x0_out)
            assert torch.equal(hist.cpu(), m), "history != thresholded x0"
            ref = MS_ROW[2] * x64 + MS_ROW[3] * m64
        elif entry == "counter":
            seeds, window = [7, (1 << 63) + 5, 11][:batch], 2
            z = ops.philox_normal(torch.empty(batch, n).to(dev), seeds, stream=ops.NOISE_STREAM_STEP, step=1, window=window).cpu()
            ops.sampler_step(xd, eps.to(dev), None, table_of(DDIM_ROW).to(dev), step, quantile=Q, x0_out=x0_out,
                             seeds=ops.seeds_tensor(seeds, dev), window=torch.tensor([window], dtype=torch.int32).to(dev))
            ref = DDIM_ROW[2] * m64 + DDIM_ROW[3] * eps.double() + DDIM_ROW[5] * z.double()
        else:
            row = DDPM_ROW if entry == "ddpm" else DDIM_ROW
            kf = {}
            ref = row[2] * m64 + row[3] * eps.double() + row[4] * x64 + row[5] * noise.double()
            if entry == "known":
                frames = KNOWN_FRAMES[n]
                mask = torch.zeros(batch, frames, dtype=torch.bool)
                mask[0, 0] = mask[batch - 1, frames - 1] = True
                known, known_noise = rnd(*shape, seed=63), rnd(*shape, seed=64)
                level = torch.tensor([[9.0, 9.0], [9.0, 9.0], [0.8125, 0.59]])
                kf = dict(known=known.to(dev), known_noise=known_noise.to(dev), frame_mask=mask.to(dev), level=level.to(dev), frames=frames)
                blend = (0.8125 * known.double() + 0.59 * known_noise.double()).view(batch, -1, frames, shape[2])
                ref = torch.where(mask.view(batch, 1, frames, 1), blend, ref.view(blend.shape)).reshape(batch, n)
            ops.sampler_step(xd, eps.view(shape).to(dev), noise.view(shape).to(dev), table_of(row).to(dev), step, quantile=Q, x0_out=x0_out, **kf)
        what = "%s B=%d n=%d kinds %s" % (entry, batch, n, [KINDS[(b + rot) % 4] for b in range(batch)])
        got = x0_out.cpu().view(batch, n)
        assert int(step.cpu()[0]) == 2, what
        assert torch.equal(got, m), "%s: x0_out differs from clamp(x, -s, s) / s in rows %s" % (what, (got != m).any(dim=1).nonzero().flatten().tolist())
        for b, (_, idx) in enumerate(built):
            assert bool((got[b, idx].abs() == 1.0).all()) and torch.equal(got[b, idx].sign(), x[b, idx].sign()), what
        err = float((xd.cpu().view(batch, n).double() - ref).abs().max())
        assert err <= 1e-5, "%s: updated x, max abs err %.3e" % (what, err)
