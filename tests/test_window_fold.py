"""ops.window_gather / ops.window_fold (csrc/window_fold.hip) and the host tables of ops.joint_windows, on both backends.
Every output is handed over NaN-filled.  The window starts, profiles and weights are written out here from the formulas of the design,
not taken from ops.

Gather: torch.equal to the slicing expression.

Fold bar, derived (u = 2^-24, the unit roundoff of fp32), per element of a frame with K contributors, against float64 formed from the
fp32 operands and the fp32 weights the kernel reads:
    |out - out64| <= (K + 1) u sum_j wgt_j |e_j|
K products each err by at most u |w_j e_j|; K - 1 additions each err by at most u times a partial sum bounded by sum_j |w_j e_j|; one
unit of slack.  Every check prints its largest fraction of the bar (pytest -s); the MI355X values are in profiles/joint_margins.txt.

Launch plan of both kernels: items = floats / V (V = 4 on the 16-byte path: frame_elems % 4 == 0 and 16-byte bases; V = 1 on the element
path), 256 threads, one item per thread and trip, G = min(ceil(items / 256), 1024) workgroups in a grid-stride loop.  Edges:
    255 / 256 / 257 items              either side of one workgroup's full trip
    262143 / 262144 / 262145 items     G reaches its cap at 262144 = 1024 * 256, which is also the most one trip of the grid covers
each on both paths (frame_elems = 4 and frame_elems = 1, the item count set by the channel count)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cvpr23_lfdm_amd import ops

U = 2.0 ** -24
KMAX = 8
CAP = 1024 * 256
EDGES = [255, 256, 257, CAP - 1, CAP, CAP + 1]
GEOMETRIES = [(4, 4, [0]), (7, 4, [0, 2, 3]), (20, 8, [0, 5, 10, 12])]          # (F, T, starts)
ELEMS = [1, 3, 4, 5, 64, 71, 1024]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def design_starts(total, frames, overlap):
    """0, s, 2s, ... with s = frames - overlap while start + frames < total, then one last window at total - frames."""
    total = max(total, frames)
    starts, s = [], 0
    while s + frames < total:
        starts.append(s)
        s += frames - overlap
    if not starts or starts[-1] + frames != total:
        starts.append(total - frames)
    return starts


def design_table(total, frames, starts, blend="ramp"):
    """count, win, loc and the float64 weights p / sum p over every frame's contributors in ascending window order."""
    p = (lambda t: min(t + 1, frames - t)) if blend == "ramp" else (lambda t: 1)
    count = np.zeros(total, dtype=np.int32)
    win, loc = np.zeros((total, KMAX), dtype=np.int32), np.zeros((total, KMAX), dtype=np.int32)
    w64 = np.zeros((total, KMAX), dtype=np.float64)
    for f in range(total):
        who = [(w, f - s) for w, s in enumerate(starts) if 0 <= f - s < frames]
        norm = sum(p(t) for _, t in who)
        count[f] = len(who)
        for j, (w, t) in enumerate(who):
            win[f, j], loc[f, j], w64[f, j] = w, t, p(t) / norm
    return {"count": count, "win": win, "loc": loc, "wgt": w64.astype(np.float32)}, w64


def nan_like(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def place(dev, t, misalign=False):
    """t on the device, contiguous; misalign: one element off a 16-byte boundary."""
    if not misalign:
        return t.to(dev).contiguous()
    buf = torch.full((t.numel() + 1,), float("nan"), device=dev)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def rand5(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def gather_ref(x, starts, frames):
    b = x.shape[0]
    return torch.stack([x[i, :, s:s + frames] for i in range(b) for s in starts])


def run_gather(dev, x, starts, frames, misalign=False):
    shape = (x.shape[0] * len(starts), x.shape[1], frames) + tuple(x.shape[3:])
    out = place(dev, torch.full(shape, float("nan")), misalign)
    got = ops.window_gather(place(dev, x, misalign), starts, frames, out=out)
    assert got is out
    return out.cpu().clone()


def fold_ref(ew, table, batch):
    """float64 from the fp32 operands and the fp32 weights -> (out64, bar): bar = (K + 1) u sum_j wgt_j |e_j|."""
    total = table["count"].shape[0]
    windows = ew.shape[0] // batch
    e = ew.double().view((batch, windows) + tuple(ew.shape[1:]))
    out = torch.zeros((batch, ew.shape[1], total) + tuple(ew.shape[3:]), dtype=torch.float64)
    mag = torch.zeros_like(out)
    for f in range(total):
        for j in range(int(table["count"][f])):
            w = float(table["wgt"][f, j])
            term = e[:, int(table["win"][f, j]), :, int(table["loc"][f, j])]
            out[:, :, f] += w * term
            mag[:, :, f] += w * term.abs()
    k = torch.from_numpy(table["count"].astype(np.float64)).view(1, 1, total, 1, 1)
    return out, (k + 1) * U * mag


def run_fold(dev, ew, table, batch, misalign=False):
    total = table["count"].shape[0]
    out = place(dev, torch.full((batch, ew.shape[1], total) + tuple(ew.shape[3:]), float("nan")), misalign)
    got = ops.window_fold(place(dev, ew, misalign), table, out)
    assert got is out
    return out.cpu().clone()


def check_fold(what, got, ew, table, batch):
    out64, bar = fold_ref(ew, table, batch)
    assert torch.isfinite(got).all(), what
    err = (got.double() - out64).abs()
    frac = float((err / bar.clamp(min=1e-300)).max())
    print("%s: %.3f of the fold bar" % (what, frac))
    assert bool((err <= bar).all()), "%s: %.3f of the fold bar" % (what, frac)
    return frac


# ------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "F%d" % g[0])
@pytest.mark.parametrize("elems", ELEMS)
def test_gather_is_the_slicing_expression(backend, geometry, elems):
    total, frames, starts = geometry
    for batch in (1, 2, 3):
        x = rand5((batch, 2, total, 1, elems), seed=elems + batch)
        assert torch.equal(run_gather(backend, x, starts, frames), gather_ref(x, starts, frames)), (batch, elems)


@pytest.mark.parametrize("elems", [4, 64, 71])
def test_gather_element_path_gives_the_same_bits(backend, elems):
    """Every base one element off a 16-byte boundary: the element path."""
    total, frames, starts = GEOMETRIES[2]
    x = rand5((2, 3, total, 1, elems), seed=7)
    got = run_gather(backend, x, starts, frames, misalign=True)
    assert torch.equal(got, gather_ref(x, starts, frames)) and torch.equal(got, run_gather(backend, x, starts, frames))


@pytest.mark.parametrize("elems", [4, 1], ids=["wide", "element"])
@pytest.mark.parametrize("items", EDGES)
def test_gather_launch_plan_edges(backend, items, elems):
    """One window of one frame: items = channels."""
    x = rand5((1, items, 1, 1, elems), seed=items)
    assert torch.equal(run_gather(backend, x, [0], 1), x)


def test_gather_spatial_frames_and_a_plan_table(backend):
    """(S, S') frames and a WindowStarts kept by the caller, refilled in place."""
    x = rand5((2, 3, 7, 4, 6), seed=3)
    table = ops.WindowStarts([0, 2, 3], backend)
    assert torch.equal(ops.window_gather(x.to(backend), table, 4).cpu(), gather_ref(x, [0, 2, 3], 4))
    table.fill([3, 0, 1])
    assert torch.equal(ops.window_gather(x.to(backend), table, 4).cpu(), gather_ref(x, [3, 0, 1], 4))


# ------------------------------------------------------------------------------------------ fold: the bar
@pytest.mark.parametrize("blend", ["ramp", "uniform"])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "F%d" % g[0])
@pytest.mark.parametrize("elems", ELEMS)
def test_fold_against_float64(backend, geometry, elems, blend):
    total, frames, starts = geometry
    table, _ = design_table(total, frames, starts, blend)
    worst = 0.0
    for batch in (1, 2, 3):
        ew = rand5((batch * len(starts), 2, frames, 1, elems), seed=11 * elems + batch)
        got = run_fold(backend, ew, table, batch)
        worst = max(worst, check_fold("fold F=%d E=%d B=%d %s" % (total, elems, batch, blend), got, ew, table, batch))
    path = os.environ.get("LFDM_JOINT_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write("fold F=%d T=%d E=%d %s on %s: %.3f of the bar\n" % (total, frames, elems, blend, backend, worst))


@pytest.mark.parametrize("elems", [4, 64, 71])
def test_fold_element_path_gives_the_same_bits(backend, elems):
    total, frames, starts = GEOMETRIES[2]
    table, _ = design_table(total, frames, starts)
    ew = rand5((2 * len(starts), 3, frames, 1, elems), seed=5)
    got = run_fold(backend, ew, table, 2, misalign=True)
    check_fold("fold element path E=%d" % elems, got, ew, table, 2)
    assert torch.equal(got, run_fold(backend, ew, table, 2))


@pytest.mark.parametrize("elems", [4, 1], ids=["wide", "element"])
@pytest.mark.parametrize("items", EDGES)
def test_fold_launch_plan_edges(backend, items, elems):
    """One global frame with two contributors (two windows of one frame): items = channels."""
    table = {"count": np.array([2], dtype=np.int32), "win": np.zeros((1, KMAX), dtype=np.int32), "loc": np.zeros((1, KMAX), dtype=np.int32),
             "wgt": np.zeros((1, KMAX), dtype=np.float32)}
    table["win"][0, 1] = 1
    table["wgt"][0, :2] = (0.25, 0.75)
    ew = rand5((2, items, 1, 1, elems), seed=items)
    check_fold("fold edge items=%d E=%d" % (items, elems), run_fold(backend, ew, table, 1), ew, table, 1)


# ------------------------------------------------------------------------------------------ fold: bits
def _single_and_shared(table, windows, frames):
    """Bool masks over (window, frame inside it): the only contributor of its global frame / one of several."""
    single = torch.zeros(windows, frames, dtype=torch.bool)
    shared = torch.zeros(windows, frames, dtype=torch.bool)
    for f in range(table["count"].shape[0]):
        k = int(table["count"][f])
        for j in range(k):
            (single if k == 1 else shared)[int(table["win"][f, j]), int(table["loc"][f, j])] = True
    return single, shared


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "F%d" % g[0])
@pytest.mark.parametrize("elems", [5, 64])
def test_fold_single_contributor_frames_are_the_windows_bits(backend, geometry, elems):
    """A frame with one contributor (weight exactly 1.0f) is the window's value bit for bit - signed zeros included - also when the
    contributors of OTHER frames hold +-0, infinities and NaN payloads: nothing leaks."""
    total, frames, starts = geometry
    table, _ = design_table(total, frames, starts)
    windows, batch = len(starts), 2
    single, shared = _single_and_shared(table, windows, frames)
    assert single.any() and bool((table["wgt"][table["count"] == 1, 0] == np.float32(1.0)).all())
    bits = lambda t: t.contiguous().view(torch.int32)
    for special in (False, True):
        ew = rand5((batch * windows, 2, frames, 1, elems), seed=elems).view(batch, windows, 2, frames, 1, elems)
        ew[:, :, :, :, :, 0] = torch.where(single.view(1, windows, 1, frames, 1), torch.tensor(-0.0), ew[:, :, :, :, :, 0])      # -0 in single frames
        if special:
            vals = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan")])
            vals = torch.cat([vals, torch.tensor([0x7fc12345], dtype=torch.int32).view(torch.float32)])       # a NaN payload
            fill = vals[torch.arange(ew.numel()) % vals.numel()].view(ew.shape)
            ew = torch.where(shared.view(1, windows, 1, frames, 1, 1), fill, ew)
        ew = ew.reshape(batch * windows, 2, frames, 1, elems).contiguous()
        got = run_fold(backend, ew, table, batch)
        e = ew.view(batch, windows, 2, frames, 1, elems)
        for f in range(total):
            if int(table["count"][f]) == 1:
                want = e[:, int(table["win"][f, 0]), :, int(table["loc"][f, 0])]
                assert torch.equal(bits(got[:, :, f]), bits(want)), (f, special)
            elif special:
                assert not torch.isfinite(got[:, :, f]).all()           # (the specials did reach the frames they belong to)


def test_fold_repeats_and_a_row_does_not_depend_on_its_batch(backend):
    total, frames, starts = GEOMETRIES[2]
    table, _ = design_table(total, frames, starts)
    windows = len(starts)
    ew = rand5((3 * windows, 3, frames, 1, 71), seed=9)
    got = run_fold(backend, ew, table, 3)
    assert torch.equal(got, run_fold(backend, ew, table, 3))
    for b in range(3):
        alone = run_fold(backend, ew[b * windows:(b + 1) * windows], table, 1)
        assert torch.equal(alone[0], got[b]), b


def test_gather_then_fold_gives_the_latent_back(backend):
    """The two kernels compose: folding the gathered windows of x gives x back - every contributor of a frame holds the same values and
    the weights sum to 1 within K u, so |got - x| <= ((K + 1) + K + 1) u |x|."""
    total, frames, starts = GEOMETRIES[1]
    table, _ = design_table(total, frames, starts)
    x = rand5((2, 3, total, 4, 4), seed=2)
    xw = run_gather(backend, x, starts, frames)
    got = run_fold(backend, xw, table, 2)
    k = torch.from_numpy(table["count"].astype(np.float64)).view(1, 1, total, 1, 1)
    assert bool(((got.double() - x.double()).abs() <= (2 * k + 2) * U * x.double().abs()).all())


# ------------------------------------------------------------------------------------------ tables (host only)
TABLE_CASES = [(40, 40, 4), (41, 40, 4), (76, 40, 4), (77, 40, 4), (112, 40, 4), (13, 8, 3), (20, 8, 3), (7, 4, 2), (3, 4, 2)]
WANT_STARTS = {(40, 40, 4): [0], (41, 40, 4): [0, 1], (76, 40, 4): [0, 36], (77, 40, 4): [0, 36, 37], (112, 40, 4): [0, 36, 72],
               (13, 8, 3): [0, 5], (20, 8, 3): [0, 5, 10, 12], (7, 4, 2): [0, 2, 3], (3, 4, 2): [0]}


@pytest.mark.parametrize("blend", ["ramp", "uniform"])
@pytest.mark.parametrize("case", TABLE_CASES, ids=lambda c: "F%d_T%d_o%d" % c)
def test_joint_windows_tables(case, blend):
    total, frames, overlap = case
    starts, table = ops.joint_windows(total, frames, overlap, blend)
    assert starts.dtype == np.int32 and starts.tolist() == WANT_STARTS[case] == design_starts(total, frames, overlap)
    glob = max(total, frames)
    want, w64 = design_table(glob, frames, starts.tolist(), blend)
    for k in ("count", "win", "loc", "wgt"):
        assert table[k].dtype == want[k].dtype and np.array_equal(table[k], want[k]), k
    assert table["count"].shape == (glob,) and table["count"].min() >= 1 and table["count"].max() <= KMAX          # every frame is covered
    assert table["wgt"].dtype == np.float32 and np.array_equal(table["wgt"], w64.astype(np.float32))          # one rounding of the float64 weight
    for f in range(glob):
        k = int(table["count"][f])
        assert abs(float(table["wgt"][f, :k].astype(np.float64).sum()) - 1.0) <= k * U, f
        assert not table["wgt"][f, k:].any()
        if k == 1:
            assert table["wgt"][f, 0] == np.float32(1.0)
        if blend == "ramp":         # among one frame's contributors, the one further from its window's nearer end never weighs less
            dist = [min(int(t), frames - 1 - int(t)) for t in table["loc"][f, :k]]
            for i in range(k):
                for j in range(k):
                    if dist[i] <= dist[j]:
                        assert table["wgt"][f, i] <= table["wgt"][f, j], (f, i, j)


def test_joint_windows_refusals():
    for overlap in (0, 8):
        with pytest.raises(ValueError, match=r"overlap must lie in \[1, frames - 1 = 7\]"):
            ops.joint_windows(20, 8, overlap)
    with pytest.raises(ValueError, match="at most 8 contributors"):
        ops.joint_windows(40, 9, 8)             # stride 1: frame 8 lies in nine windows
    assert ops.joint_windows(40, 8, 7)[1]["count"].max() == 8           # eight are taken
    with pytest.raises(ValueError, match="2\\^24"):
        ops.joint_windows(1366, 40, 4, size=64)             # 3 * 64 * 64 * 1366 = 16 785 408 >= 2^24
    ops.joint_windows(1365, 40, 4, size=64)                 # 16 773 120 < 2^24
    with pytest.raises(ValueError, match="blend"):
        ops.joint_windows(20, 8, 3, "cosine")
    with pytest.raises(ValueError):
        ops.joint_windows(20.0, 8, 3)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def test_entry_points_refuse_bad_arguments(backend):
    """The C entry points themselves: null operands, a start past F - T, a count of 0 and of 9 - nothing is written."""
    from cvpr23_lfdm_amd import _native
    lib, dev = _native.library(), backend
    total, frames, starts = GEOMETRIES[1]
    table, _ = design_table(total, frames, starts)
    x, xw = rand5((1, 2, total, 1, 4), seed=1).to(dev), nan_like(dev, 3, 2, frames, 1, 4)
    st = np.asarray(starts, dtype=np.int32)
    st_dev = torch.from_numpy(st).to(dev)
    host = lambda a: ctypes.c_void_p(a.ctypes.data)
    gather = lambda x_, sd, sh, o, f=total, t=frames: lib.lfdm_window_gather_f32(_ptr(x_), _ptr(sd), sh, _ptr(o), 1, 3, 2, f, t, 4, None)
    assert gather(x, st_dev, host(st), xw) == 0
    assert torch.equal(xw.cpu(), gather_ref(x.cpu(), starts, frames))
    xw.fill_(float("nan"))
    late = np.asarray([0, 2, 4], dtype=np.int32)
    for rc in (gather(None, st_dev, host(st), xw), gather(x, None, host(st), xw), gather(x, st_dev, None, xw), gather(x, st_dev, host(st), None),
               gather(x, st_dev, host(late), xw), gather(x, st_dev, host(np.asarray([-1, 2, 3], dtype=np.int32)), xw),
               gather(x, st_dev, host(st), xw, f=0), gather(x, st_dev, host(st), xw, t=0), gather(x, st_dev, host(st), xw, t=total + 1)):
        assert rc != 0
    assert b"window_gather" in lib.lfdm_last_error() and torch.isnan(xw).all()
    ew, out = rand5((3, 2, frames, 1, 4), seed=2).to(dev), nan_like(dev, 1, 2, total, 1, 4)
    d = {k: torch.from_numpy(v).to(dev) for k, v in table.items()}
    fold = lambda e, c, w, l, g, ch, o: lib.lfdm_window_fold_f32(_ptr(e), _ptr(c), _ptr(w), _ptr(l), _ptr(g), ch, _ptr(o), 1, 3, 2, total,
                                                                 frames, 4, None)
    good = (ew, d["count"], d["win"], d["loc"], d["wgt"], host(table["count"]), out)
    assert fold(*good) == 0 and torch.isfinite(out).all()
    out.fill_(float("nan"))
    for i in range(len(good)):
        assert fold(*[None if j == i else a for j, a in enumerate(good)]) != 0, i
    for bad in (0, 9):
        count = table["count"].copy()
        count[3] = bad
        assert fold(ew, d["count"], d["win"], d["loc"], d["wgt"], host(count), out) != 0
    assert b"window_fold" in lib.lfdm_last_error() and torch.isnan(out).all()
    # the Python face refuses the same before it calls
    with pytest.raises(ValueError, match="starts span"):
        ops.window_gather(x, [0, 2, 4], frames)
    zero = dict(table, count=np.where(np.arange(total) == 3, 0, table["count"]).astype(np.int32))
    with pytest.raises(ValueError, match="contributors"):
        ops.window_fold(ew, zero, out)
    with pytest.raises(ValueError, match="names a window"):
        ops.window_fold(ew, dict(table, win=table["win"] + 1), out)
    with pytest.raises(ValueError):
        ops.window_fold(ew[:, :, :, :, ::2], table, out[:, :, :, :, ::2])
    assert torch.isnan(out).all()


def test_header_declares_the_entry_points():
    from cvpr23_lfdm_amd import _native
    from test_operand_layouts import LD_NAMES
    header = open(os.path.join(REPO, "include", "lfdm_hip.h")).read()
    assert {"lfdm_window_gather_f32", "lfdm_window_fold_f32"} <= set(_native.EXPORTED_SYMBOLS)
    for name in ("lfdm_window_gather_f32", "lfdm_window_fold_f32"):
        decl = re.search(r"/\* Layout:(?:[^*]|\*(?!/))*\*/\s*int %s\(([^;]*)\)\s*;" % name, header)
        assert decl, name
        assert not set(re.findall(r"[A-Za-z_][A-Za-z_0-9]*", decl.group(1))) & LD_NAMES            # dense operands: no leading dimension
    assert "#define LFDM_FOLD_MAX_CONTRIB 8" in header and ops.FOLD_MAX_CONTRIB == 8


def test_abi_version_stays_13(backend):
    from cvpr23_lfdm_amd import _native
    assert _native.library().lfdm_abi_version() == 14          # (13 when the entries were added, hence the name; 14: lfdm_train_loss_params)
