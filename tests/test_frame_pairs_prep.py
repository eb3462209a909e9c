"""LFAE stage-1 frame pairs from the packed store (csrc/video_prep.hip: lfdm_frame_pairs_prep_u8, video_store.PackedFramePairs /
DevicePairPrep), in the manner of tests/test_video_prep.py.

The yardstick is the body of lfae_train.FramePairs.__getitem__ with recorded draws: data.color_jitter with a replaying `rnd`, then
io_compat.resize(float32, INTER_AREA) / 255.0, then [:, ::-1], then the exchange of the two frames, then the transpose.  The contract
is torch.equal: no tolerance and no share of excused pixels.  The one bound is the sibling's: a store shrunk when packed, WITHOUT
jitter, is within its single rounding to a byte (0.5 / 255 + 1e-6) of the host path on the originals; with jitter it is compared to
the host arithmetic on the stored bytes, and its distance to the originals is only printed.
"""
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from cvpr23_lfdm_amd import data, io_compat, lfae_train, ops
from layout import SENTINEL
from test_video_prep import _Replay, _hf, _store, emu_lib  # noqa: F401  (emu_lib is a fixture)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUG_JITTER = {"brightness": 0.1, "contrast": 0.1, "saturation": 0.1, "hue": 0.1}          # the reference's mug128.yaml
# the end points of that config's ranges (hue 0.1 -> int(+-0.1 * 255) = +-25) and the neutral values
FACTORS = list(itertools.product((0.9, 1.0, 1.1), (0.9, 1.0, 1.1), (0.9, 1.0, 1.1), (-25, 0, 25)))


def _factors(b, start=0):
    # a stride coprime to 81 walks through every value of every factor within a few elements
    return [FACTORS[(start + 31 * i) % len(FACTORS)] for i in range(b)]


def _asym_store(s, seed=0):
    """test_video_prep._store with its two constant frames made different left and right: no frame equals its mirror image."""
    st = _store(s, seed)
    st[2, :, s // 2:] = 3
    st[3, :, :s // 2] = 250
    for f in st:
        assert not np.array_equal(f, f[:, ::-1])
    return st


def _yardstick(frames, size, factors=None, flip=False, exchange=False):
    """FramePairs.__getitem__ behind the decoder on the two pictures `frames`, draws replayed -> (source, driving) (3, H, H) tensors."""
    frames = list(frames)
    if factors is not None:
        bf, cf, sf, shift = factors
        frames = data.color_jitter(frames, rnd=_Replay([bf, cf, sf, _hf(shift)]))
    frames = [io_compat.resize(np.asarray(f, np.float32), size, interpolation=io_compat.INTER_AREA) / 255.0 for f in frames]
    if flip:
        frames = [f[:, ::-1] for f in frames]
    if exchange:
        frames = frames[::-1]
    return tuple(torch.from_numpy(np.ascontiguousarray(np.transpose(f, (2, 0, 1)), dtype=np.float32)) for f in frames)


def _yardstick_batch(store, pairs, size, factors, flips, valid=None):
    src, drv = [], []
    for b, (i, j) in enumerate(pairs):
        y0, x0, h, w = (0, 0) + store.shape[1:3] if valid is None else valid[b]
        s, d = _yardstick([store[i][y0:y0 + h, x0:x0 + w], store[j][y0:y0 + h, x0:x0 + w]], size, None if factors is None else factors[b],
                          bool(flips[b]))
        src.append(s)
        drv.append(d)
    return torch.stack(src), torch.stack(drv)


def _prep(dev, store, pairs, size, factors, flips, valid=None, out=None):
    st = store if torch.is_tensor(store) else torch.from_numpy(store).to(dev)
    idx = torch.tensor(pairs, dtype=torch.int32)
    fl = torch.tensor(flips, dtype=torch.int32)
    if factors is None:
        return ops.frame_pairs_prep(st, idx, None, None, fl, size, False, out=out)
    params = torch.tensor([f[:3] for f in factors], dtype=torch.float32)
    shift = torch.tensor([f[3] for f in factors], dtype=torch.int32)
    v = None if valid is None else torch.tensor(valid, dtype=torch.int32)
    return ops.frame_pairs_prep(st, idx, params, shift, fl, size, True, out=out, valid=v)


def _assert_pair(got, want, what):
    for name, g, w in zip(("source", "driving"), got, want):
        g = g.cpu()
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(w.shape), (what, name, g.shape, w.shape)
        assert torch.equal(g, w), (what, name, "%d of %d values differ, max %.3f levels" % (int((g != w).sum()), g.numel(),
                                                                                          float((g - w).abs().max()) * 255))


# H = 4: one group per row (the flip reverses inside the store only); 8: two groups swap; 12: the middle group maps to itself; 20: ordinary
SHAPES = [(h, k) for h in (4, 8, 12, 20) for k in (1, 2, 4)]
# (pairs, flips) over the 9 frames of the store: B = 1 with and without a flip, B = 3 with the flags mixed; equal rows, descending rows
# and the store's last row are all in
BATCHES = [([(0, 4)], [0]), ([(7, 1)], [1]), ([(8, 8)], [1]), ([(1, 5), (8, 0), (6, 6)], [1, 0, 1]), ([(3, 2), (4, 7), (2, 3)], [0, 1, 0])]


@pytest.mark.parametrize("size,k", SHAPES)
def test_pairs_equal_the_host_path(backend, size, k):
    store = _asym_store(size * k, seed=5 * size + k)
    dev_store = torch.from_numpy(store).to(backend)
    for case, (pairs, flips) in enumerate(BATCHES):
        got = _prep(backend, dev_store, pairs, size, None, flips)
        assert got[0].is_contiguous() and got[1].is_contiguous()
        want = _yardstick_batch(store, pairs, size, None, flips)
        _assert_pair(got, want, ("jitter off", pairs, flips))
        unflipped = _yardstick_batch(store, pairs, size, None, [0] * len(flips))
        for b, f in enumerate(flips):              # a kernel that ignored the flag would have failed above: the shrunk frames are asymmetric too
            assert not f or not (torch.equal(want[0][b], unflipped[0][b]) or torch.equal(want[1][b], unflipped[1][b])), (pairs, b)
        factors = _factors(len(pairs), start=11 * case + size + k)
        _assert_pair(_prep(backend, dev_store, pairs, size, factors, flips), _yardstick_batch(store, pairs, size, factors, flips),
                     ("jitter on", pairs, flips, factors))


def test_every_extreme_of_the_reference_config(backend):
    """All 81 combinations of 0.9 / 1.0 / 1.1 and hue shift -25 / 0 / +25, one pair each, flips alternating."""
    store = _asym_store(8, seed=2)
    pairs = [((b + 1) % 9, (3 * b) % 9) for b in range(len(FACTORS))]
    flips = [(b // 3) % 2 for b in range(len(FACTORS))]
    _assert_pair(_prep(backend, store, pairs, 8, FACTORS, flips), _yardstick_batch(store, pairs, 8, FACTORS, flips), "81 combinations")


def test_a_pair_does_not_depend_on_its_batch(backend):
    store = _asym_store(16, seed=9)
    n = len(store)
    f_mine, f_other = (0.9, 1.1, 0.9, 25), (1.1, 0.9, 1.1, -25)
    for k in (1, 2):
        for pair in ((5, 2), (4, 4), (n - 1, 0), (0, n - 1)):          # descending rows, equal rows, the store's last row
            for flip in (0, 1):
                alone = _prep(backend, store, [pair], 16 // k, [f_mine], [flip])
                batch = _prep(backend, store, [(3, 7), pair, (8, 1)], 16 // k, [f_other, f_mine, f_other], [1 - flip, flip, 1 - flip])
                assert torch.equal(batch[0][1], alone[0][0]) and torch.equal(batch[1][1], alone[1][0]), (k, pair, flip)
                first = _prep(backend, store, [pair, (6, 2)], 16 // k, [f_mine, f_other], [flip, 1 - flip])
                assert torch.equal(first[0][0], alone[0][0]) and torch.equal(first[1][0], alone[1][0]), (k, pair, flip)
                _assert_pair(alone, _yardstick_batch(store, [pair], 16 // k, [f_mine], [flip]), (k, pair, flip))
        # equal rows: the two outputs are the same picture
        same = _prep(backend, store, [(4, 4)], 16 // k, [f_mine], [1])
        assert torch.equal(same[0], same[1])


def test_padding_moves_with_the_flip(backend):
    """A 16 x 11 picture sits at x0 = (16 - 11) // 2 = 2 of the 16 x 16 stored frame: 2 columns of padding on the left, 3 on the right.
    Flipped, the padding is 3 left and 2 right, exactly 0.0, the picture is where f[:, ::-1] puts it, and the contrast grey level comes
    from picture pixels only (the yardstick jitters the 16 x 11 picture, then pads)."""
    rng = np.random.RandomState(2)
    pics = [rng.randint(0, 256, (16, 11, 3)).astype(np.uint8) for _ in range(3)]
    store = np.zeros((3, 16, 16, 3), np.uint8)
    store[:, :, 2:13] = np.stack(pics)
    valid = [[0, 2, 16, 11]] * 3
    pairs, flips, factors = [(2, 0), (1, 2), (0, 1)], [1, 0, 1], [(0.9, 1.1, 0.9, 25), (1.1, 0.9, 1.1, -25), (1.0, 1.1, 1.0, 25)]
    got = _prep(backend, store, pairs, 16, factors, flips, valid=valid)
    _assert_pair(got, _yardstick_batch(store, pairs, 16, factors, flips, valid=valid), "non-square, jitter on")
    src, drv = (t.cpu() for t in got)
    for t in (src, drv):
        assert float(t[0, :, :, :3].abs().max()) == 0.0 and float(t[0, :, :, 14:].abs().max()) == 0.0          # flipped: 3 left, 2 right
        assert float(t[1, :, :, :2].abs().max()) == 0.0 and float(t[1, :, :, 13:].abs().max()) == 0.0          # not flipped: 2 left, 3 right
        assert float(t[0, :, :, 3].abs().max()) > 0 and float(t[0, :, :, 13].abs().max()) > 0
    _assert_pair(_prep(backend, store, pairs, 16, None, flips), _yardstick_batch(store, pairs, 16, None, flips), "non-square, jitter off")


def test_out_is_written_and_nothing_else(backend):
    """source and driving placed inside one sentinel-NaN buffer, with gaps before, between and after: every float of the two is written,
    every other float keeps its bit pattern."""
    store = _asym_store(16, seed=4)
    pairs, flips, factors = [(0, 5), (8, 7), (4, 4)], [1, 0, 1], _factors(3, start=5)
    for size in (16, 8):
        n, gap = 3 * 3 * size * size, 8                      # gaps of 8 floats keep both views 16-byte aligned
        raw = torch.full((3 * gap + 2 * n,), SENTINEL, dtype=torch.int32, device=backend)
        flat = raw.view(torch.float32)
        src, drv = flat[gap:gap + n].view(3, 3, size, size), flat[2 * gap + n:2 * gap + 2 * n].view(3, 3, size, size)
        got = _prep(backend, store, pairs, size, factors, flips, out=(src, drv))
        assert got[0].data_ptr() == src.data_ptr() and got[1].data_ptr() == drv.data_ptr()
        assert got[0].is_contiguous() and got[1].is_contiguous()
        outside = torch.ones(raw.numel(), dtype=torch.bool, device=backend)
        outside[gap:gap + n] = False
        outside[2 * gap + n:2 * gap + 2 * n] = False
        assert bool((raw[outside] == SENTINEL).all()), "a float outside source and driving was overwritten"
        assert not bool(torch.isnan(flat[~outside]).any()), "a float of source or driving was not written"
        _assert_pair((src, drv), _yardstick_batch(store, pairs, size, factors, flips), "out=")


# ---------------------------------------------------------------------------------------------
# data set against data set (host + emulator)
# ---------------------------------------------------------------------------------------------
def _write_folders(root, scale=1):
    """Frame folders of several depths, frame size 16 * scale: nested RGB, nested grayscale, a flat non-square one (4 : 3), a flat one
    with a single frame (no pair to draw: skipped), a nested one with exactly two frames.  Names hold nothing that sorts below '/'."""
    rng = np.random.RandomState(11)
    s = 16 * scale

    def smooth(h, w, c, n):
        base = rng.randint(0, 256, (n, h // (4 * scale), w // (4 * scale), c))
        up = np.repeat(np.repeat(base, 4 * scale, 1), 4 * scale, 2)
        return np.clip(up + rng.randint(-6, 7, up.shape), 0, 255).astype(np.uint8)

    plan = {("subj1", "happy", "take0"): smooth(s, s, 3, 6), ("subj1", "sad"): smooth(s, s, 1, 5)[..., 0], ("clipA",): smooth(s, 3 * s // 4, 3, 7),
            ("clipB",): smooth(s, s, 3, 1), ("subj2", "angry", "take1"): smooth(s, s, 3, 2)}
    for parts, frames in plan.items():
        d = os.path.join(root, *parts)
        os.makedirs(d)
        for i, f in enumerate(frames):
            io_compat.imsave(os.path.join(d, "%03d.png" % i), f)


CONFIGS = [dict(horizontal_flip=True, time_flip=True, jitter=None), dict(horizontal_flip=False, time_flip=False, jitter=None),
           dict(horizontal_flip=True, time_flip=True, jitter=MUG_JITTER), dict(horizontal_flip=False, time_flip=False, jitter=MUG_JITTER)]


def _host_items(src, frame_shape, cfg, seed, rounds):
    ds = lfae_train.FramePairs(src, frame_shape=frame_shape, seed=3, **cfg)
    random.seed(seed)
    return ds, [ds[i] for _ in range(rounds) for i in range(len(ds))]


def _packed_items(packed, frame_shape, cfg, seed, rounds, resident=False):
    from torch.utils.data import default_collate
    from cvpr23_lfdm_amd import video_store
    ds = video_store.PackedFramePairs(packed, frame_shape=frame_shape, seed=3, resident=resident, **cfg)
    prep = video_store.DevicePairPrep(ds)
    random.seed(seed)
    items = [ds[i] for _ in range(rounds) for i in range(len(ds))]
    return ds, items, [prep(default_collate([it])) for it in items]


def test_data_set_equals_frame_pairs(tmp_path, emu_lib):
    from cvpr23_lfdm_amd import video_store
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_folders(src)
    index = video_store.pack_frame_folders(src, packed, 16, layout="any")
    assert index["frames"] == 21 and os.path.getsize(os.path.join(packed, "frames.u8")) == 21 * 16 * 16 * 3
    flipped = 0
    for cfg in CONFIGS:
        ref_ds, ref = _host_items(src, 16, cfg, seed=4, rounds=3)
        ds, items, got = _packed_items(packed, 16, cfg, seed=4, rounds=3)
        assert len(ds) == len(ref_ds) == 4                   # the single-frame folder is skipped by both
        for want, item, g in zip(ref, items, got):
            assert tuple(g["source"].shape) == (1, 3, 16, 16) and item[0].dtype == np.uint8 and item[0].shape == (2, 16, 16, 3)
            assert torch.equal(g["source"][0], want["source"]) and torch.equal(g["driving"][0], want["driving"])
            flipped += int(item[3])
            if not cfg["horizontal_flip"]:
                assert int(item[3]) == 0
            if cfg["jitter"] is None:
                assert item[1].tolist() == [1, 1, 1] and int(item[2]) == 0
        # resident and staged: the same bytes, from rows instead of pixels
        rds, ritems, rgot = _packed_items(packed, 16, cfg, seed=4, rounds=3, resident=True)
        assert ritems[0][0].dtype == np.int32 and ritems[0][0].shape == (2,)
        for g, r in zip(got, rgot):
            assert torch.equal(g["source"], r["source"]) and torch.equal(g["driving"], r["driving"])
    assert flipped > 0
    # other draws give other tensors: the comparison above is not vacuous
    _, _, other = _packed_items(packed, 16, CONFIGS[2], seed=5, rounds=1)
    _, _, same = _packed_items(packed, 16, CONFIGS[2], seed=4, rounds=1)
    assert not all(torch.equal(a["source"], b["source"]) for a, b in zip(other, same))


def test_collated_batches(tmp_path, emu_lib):
    """A DataLoader batch of several items equals the items one by one (the flags and rectangles are per item)."""
    from torch.utils.data import DataLoader
    from cvpr23_lfdm_amd import video_store
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_folders(src)
    video_store.pack_frame_folders(src, packed, 16, layout="any")
    for resident in (False, True):
        _, _, single = _packed_items(packed, 16, CONFIGS[2], seed=6, rounds=1, resident=resident)
        ds = video_store.PackedFramePairs(packed, frame_shape=16, seed=3, resident=resident, **CONFIGS[2])
        prep = video_store.DevicePairPrep(ds)
        random.seed(6)
        (batch,) = list(DataLoader(ds, batch_size=4, shuffle=False))
        got = prep(batch)
        assert sorted(got) == ["driving", "source"] and tuple(got["source"].shape) == (4, 3, 16, 16)
        for i, s in enumerate(single):
            assert torch.equal(got["source"][i], s["source"][0]) and torch.equal(got["driving"][i], s["driving"][0])


def test_layout_any_lists_what_frame_pairs_walks(tmp_path):
    from cvpr23_lfdm_amd import video_store
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_folders(src)
    index = video_store.pack_frame_folders(src, packed, 16, layout="any")
    assert index["version"] == video_store.STORE_VERSION and sorted(index) == ["frames", "store_size", "version", "videos"]
    assert [(v["label"], v["video"], v["count"]) for v in index["videos"]] == [
        ("", "clipA", 7), ("", "clipB", 1), ("subj1", "happy/take0", 6), ("subj1", "sad", 5), ("subj2", "angry/take1", 2)]
    assert [v["valid"] for v in index["videos"]][0] == [0, 2, 16, 12]
    walked = [os.path.dirname(paths[0]) for paths in lfae_train.FramePairs(src).videos]
    listed = [os.path.normpath(os.path.join(src, v["label"], v["video"])) for v in index["videos"] if v["count"] >= 2]
    assert listed == walked
    ds = video_store.PackedFramePairs(packed, frame_shape=16)
    assert [(v["label"], v["video"]) for v in ds.videos] == [("", "clipA"), ("subj1", "happy/take0"), ("subj1", "sad"), ("subj2", "angry/take1")]
    # the default layout walks exactly <label>/<video>/: of these folders only subj1/sad qualifies
    index = video_store.pack_frame_folders(src, str(tmp_path / "p2"), 16)
    assert [(v["label"], v["video"]) for v in index["videos"]] == [("subj1", "sad")]
    with pytest.raises(ValueError, match="layout"):
        video_store.pack_frame_folders(src, str(tmp_path / "p3"), 16, layout="flat")


def test_store_shrunk_when_packed(tmp_path, emu_lib):
    """Sources at 32, store and training size 16.  Without jitter: within the store's one rounding to a byte of the host path on the
    originals.  With jitter: bit for bit the host arithmetic on the STORED picture; the distance to the originals is printed only."""
    from cvpr23_lfdm_amd import video_store
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_folders(src, scale=2)
    video_store.pack_frame_folders(src, packed, 16, layout="any")
    _, ref = _host_items(src, 16, CONFIGS[0], seed=4, rounds=2)
    _, _, got = _packed_items(packed, 16, CONFIGS[0], seed=4, rounds=2)
    err = max(float((g[k][0] - w[k]).abs().max()) for g, w in zip(got, ref) for k in ("source", "driving"))
    print("jitter off: max abs difference %.3e (bound %.3e)" % (err, 0.5 / 255 + 1e-6))
    assert err <= 0.5 / 255 + 1e-6
    assert err > 0                                                  # the sources are noisy: the rounding is really exercised
    _, on_originals = _host_items(src, 16, CONFIGS[2], seed=4, rounds=2)
    _, items, got = _packed_items(packed, 16, CONFIGS[2], seed=4, rounds=2)
    far = 0.0
    for (frames, params, shift, flip, (y0, x0, h, w)), g, o in zip(items, got, on_originals):
        factors = tuple(float(p) for p in params) + (int(shift),)
        want = _yardstick([f[y0:y0 + h, x0:x0 + w] for f in frames], 16, factors, bool(flip))
        assert torch.equal(g["source"][0], want[0]) and torch.equal(g["driving"][0], want[1])
        far = max(far, float((g["source"][0] - o["source"]).abs().max()), float((g["driving"][0] - o["driving"]).abs().max()))
    print("jitter on: jitter at store resolution is %.2f levels of 255 from jitter on the originals" % (far * 255))


@pytest.mark.gpu
def test_device_pair_prep_on_the_device(tmp_path):
    """The staged path (its reused pinned buffers, and a loader that pins the batch itself) and the resident store on the product library."""
    from torch.utils.data import DataLoader
    from cvpr23_lfdm_amd import _native, video_store
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native._set_library_for_tests(None)
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_folders(src)
    video_store.pack_frame_folders(src, packed, 16, layout="any")
    for cfg in (CONFIGS[0], CONFIGS[2]):
        _, ref = _host_items(src, 16, cfg, seed=4, rounds=3)
        for resident in (False, True):
            _, _, got = _packed_items(packed, 16, cfg, seed=4, rounds=3, resident=resident)
            for want, g in zip(ref, got):
                assert g["source"].is_cuda
                assert torch.equal(g["source"][0].cpu(), want["source"]) and torch.equal(g["driving"][0].cpu(), want["driving"])
        ds = video_store.PackedFramePairs(packed, frame_shape=16, seed=3, **cfg)
        prep = video_store.DevicePairPrep(ds)
        random.seed(4)
        got = [prep(batch) for _ in range(3) for batch in DataLoader(ds, batch_size=2, shuffle=False, pin_memory=True)]
        src_all, drv_all = torch.cat([g["source"] for g in got]).cpu(), torch.cat([g["driving"] for g in got]).cpu()
        assert torch.equal(src_all, torch.stack([r["source"] for r in ref])) and torch.equal(drv_all, torch.stack([r["driving"] for r in ref]))


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refusals(backend, tmp_path):
    from cvpr23_lfdm_amd import video_store
    dev = backend
    store = torch.zeros(3, 16, 16, 3, dtype=torch.uint8, device=dev)
    idx, flip = torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    params, shift = torch.ones(1, 3), torch.zeros(1, dtype=torch.int32)
    src, drv = ops.frame_pairs_prep(store, idx, None, None, flip, 8, False)
    assert tuple(src.shape) == tuple(drv.shape) == (1, 3, 8, 8) and float(src.abs().max()) == 0.0 and float(drv.abs().max()) == 0.0
    for bad in (flip.long(), flip.float(), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), None):
        with pytest.raises(ValueError, match="flip"):
            ops.frame_pairs_prep(store, idx, None, None, bad, 16, False)
    for bad in (2, -1):
        with pytest.raises(ValueError, match="flip holds"):
            ops.frame_pairs_prep(store, idx, None, None, torch.tensor([bad], dtype=torch.int32), 16, False)
    for bad in (torch.zeros(1, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), idx.long()):
        with pytest.raises(ValueError, match="pair_index"):
            ops.frame_pairs_prep(store, bad, None, None, flip, 16, False)
    for bad in ([[0, 3]], [[-1, 0]]):
        with pytest.raises(IndexError, match="pair_index"):
            ops.frame_pairs_prep(store, torch.tensor(bad, dtype=torch.int32), None, None, flip, 16, False)
    good = torch.empty(1, 3, 16, 16, device=dev)
    wide = torch.empty(1, 3, 16, 32, device=dev)[..., :16]                                    # not contiguous
    off = torch.empty(3 * 16 * 16 + 4, device=dev)[1:1 + 3 * 16 * 16].view(1, 3, 16, 16)       # contiguous, 4 bytes off a 16-byte boundary
    for bad in ((wide, good), (good, wide), (off, good), (good, off), (good, torch.empty(1, 3, 8, 8, device=dev)), (good, good.double()),
                (good,)):
        with pytest.raises(ValueError, match="out"):
            ops.frame_pairs_prep(store, idx, None, None, flip, 16, False, out=bad)
    with pytest.raises(ValueError, match="1, 2 or 4"):
        ops.frame_pairs_prep(torch.zeros(1, 24, 24, 3, dtype=torch.uint8, device=dev), idx, None, None, flip, 8, False)       # ratio 3
    with pytest.raises(ValueError, match="1, 2 or 4"):
        ops.frame_pairs_prep(store, idx, None, None, flip, 12, False)
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.frame_pairs_prep(torch.zeros(1, 18, 18, 3, dtype=torch.uint8, device=dev), idx, None, None, flip, 9, False)
    with pytest.raises(ValueError, match="store_u8"):
        ops.frame_pairs_prep(store.float(), idx, None, None, flip, 16, False)
    with pytest.raises(ValueError, match="params"):
        ops.frame_pairs_prep(store, idx, None, shift, flip, 16, True)                          # jitter without params
    with pytest.raises(ValueError, match="params"):
        ops.frame_pairs_prep(store, idx, torch.ones(2, 3), shift, flip, 16, True)
    with pytest.raises(ValueError, match="NaN or an infinity"):
        ops.frame_pairs_prep(store, idx, torch.tensor([[1.0, float("nan"), 1.0]]), shift, flip, 16, True)
    with pytest.raises(ValueError, match="hue_shift"):
        ops.frame_pairs_prep(store, idx, params, None, flip, 16, True)
    with pytest.raises(ValueError, match="valid"):
        ops.frame_pairs_prep(store, idx, params, shift, flip, 16, True, valid=torch.tensor([[0, 8, 16, 12]], dtype=torch.int32))
    # the data set refuses a picture rectangle that the shrink would mix with padding, and a ratio the kernel does not have
    src_dir, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_folders(src_dir)
    video_store.pack_frame_folders(src_dir, packed, 16, layout="any")
    for size in (16, 8):
        video_store.PackedFramePairs(packed, frame_shape=size)
    with pytest.raises(ValueError, match="mix picture and padding"):
        video_store.PackedFramePairs(packed, frame_shape=4)
    with pytest.raises(ValueError, match="1, 2 or 4"):
        video_store.PackedFramePairs(packed, frame_shape=12)


def test_c_entry_point_checks_its_operands(backend):
    import ctypes as C
    from cvpr23_lfdm_amd import _native
    lib = _native.library()
    dev = backend
    store = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=dev)
    idx = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    params, shift, flip = torch.ones(1, 3, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    src, drv = torch.empty(1, 3, 16, 16, device=dev), torch.empty(1, 3, 16, 16, device=dev)
    off = torch.empty(3 * 16 * 16 + 4, device=dev)[1:]
    ws = torch.empty(8, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = ops._stream(lib)

    def call(store=store, n=2, idx=idx, params=params, shift=shift, flip=flip, src=src, drv=drv, b=1, s=16, h=16, jitter=1, ws=ws, ws_bytes=32):
        return lib.lfdm_frame_pairs_prep_u8(p(store), n, p(idx), p(params), p(shift), None, p(flip), p(src), p(drv), b, s, h, jitter, p(ws),
                                            ws_bytes, stream)

    assert call() == 0 and call(jitter=0, params=None, shift=None, ws=None, ws_bytes=0) == 0
    for kw, what in ((dict(store=None), "null"), (dict(idx=None), "null"), (dict(flip=None), "null"), (dict(src=None), "null"),
                     (dict(drv=None), "null"), (dict(src=off), "aligned"), (dict(drv=off), "aligned"),
                     (dict(params=None), "jitter needs"), (dict(shift=None), "jitter needs"), (dict(ws=None), "jitter needs"),
                     (dict(ws_bytes=4), "jitter needs"), (dict(b=0), ">= 1"), (dict(n=0), ">= 1"),
                     (dict(s=18, h=18), "multiples of 4"), (dict(s=24, h=8), "1, 2 or 4"), (dict(s=16, h=12), "1, 2 or 4"),
                     (dict(s=8, h=16), "1, 2 or 4")):
        assert call(**kw) == -1, kw
        msg = lib.lfdm_last_error().decode()
        assert msg.startswith("frame_pairs_prep") and what in msg, (kw, msg)


def test_product_library_refuses_cpu_tensors():
    from cvpr23_lfdm_amd import _native
    _native._set_library_for_tests(None)
    store = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_pairs_prep(store, torch.zeros(1, 2, dtype=torch.int32), None, None, torch.zeros(1, dtype=torch.int32), 8, False)


def test_abi_stays_12_with_the_new_symbol():
    import re
    from cvpr23_lfdm_amd import _build, _native
    header = open(os.path.join(REPO, "include", "lfdm_hip.h")).read()
    assert "lfdm_frame_pairs_prep_u8" in _native.EXPORTED_SYMBOLS
    assert re.search(r"/\* Layout:[^*]*\*/\s*int lfdm_frame_pairs_prep_u8\(", header)
    assert _native.NativeLibrary(_build.build_hip(), "hip").lfdm_abi_version() == 14          # (12 when the entry point was added; 13: lfdm_sampler_step_params; 14: lfdm_train_loss_params)


# ---------------------------------------------------------------------------------------------
# tools
# ---------------------------------------------------------------------------------------------
def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location("%s_under_test" % name, os.path.join(REPO, "tools", "%s.py" % name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_lfae_packed_flag(tmp_path, emu_lib):
    from cvpr23_lfdm_amd import video_store
    mod = _tool("train_lfae")
    args = mod.parse_args(["--packed", "DIR", "--resident"])
    assert args.packed == "DIR" and args.resident and not args.data_dir
    args = mod.parse_args(["--data-dir", "X"])
    assert args.data_dir == "X" and args.packed == "" and not args.resident
    for bad in (["--packed", "DIR", "--data-dir", "X"], ["--resident"], ["--data-dir", "X", "--resident"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_folders(src)
    video_store.pack_frame_folders(src, packed, 16, layout="any")
    cfg = {"dataset_params": {"augmentation_params": {"flip_param": {"horizontal_flip": True, "time_flip": False}, "jitter_param": MUG_JITTER}}}
    settings = lambda ds: (ds.frame_shape, ds.horizontal_flip, ds.time_flip, ds.jitter, ds.seed)
    # without --packed: what the tool constructed before, and no preparation step
    ds, prep = mod.make_dataset(mod.parse_args(["--data-dir", src, "--frame-shape", "16"]), cfg, 3)
    assert type(ds) is lfae_train.FramePairs and prep is None and settings(ds) == (16, True, False, MUG_JITTER, 3) and len(ds) == 4
    ds, prep = mod.make_dataset(mod.parse_args(["--data-dir", src, "--frame-shape", "16"]), {}, 0)
    assert type(ds) is lfae_train.FramePairs and settings(ds) == (16, True, True, None, 0)
    assert mod.make_dataset(mod.parse_args([]), cfg, 0) == (None, None)                       # synthetic pairs
    ds, prep = mod.make_dataset(mod.parse_args(["--packed", packed, "--frame-shape", "16"]), cfg, 3)
    assert type(ds) is video_store.PackedFramePairs and not ds.resident and settings(ds) == (16, True, False, MUG_JITTER, 3) and len(ds) == 4
    assert type(prep) is video_store.DevicePairPrep and prep.store is None
    args = mod.parse_args(["--packed", packed, "--resident", "--frame-shape", "16", "--batch", "2"])
    ds, prep = mod.make_dataset(args, {}, 1)
    assert ds.resident and settings(ds) == (16, True, True, None, 1) and tuple(prep.store.shape) == (21, 16, 16, 3)
    loader = mod.make_loader(ds, args)
    assert loader.num_workers == 0 and loader.batch_size == 2 and loader.drop_last
    assert sorted(prep(next(iter(loader)))) == ["driving", "source"]
    assert "resident" in mod.data_name(args) and packed in mod.data_name(args)
    assert mod.data_name(mod.parse_args([])) == "synthetic" and mod.data_name(mod.parse_args(["--data-dir", src])) == src
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "train_lfae.py"), "--help"], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--packed" in r.stdout and "--resident" in r.stdout and "--data-dir" in r.stdout


def test_pack_videos_tool_layout_any(tmp_path):
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    os.makedirs(os.path.join(src, "clipA"))
    os.makedirs(os.path.join(src, "clipB"))
    rng = np.random.RandomState(0)
    for d, n in (("clipA", 3), ("clipB", 2)):
        for i in range(n):
            io_compat.imsave(os.path.join(src, d, "%03d.png" % i), rng.randint(0, 256, (16, 16, 3)).astype(np.uint8))
    tool = os.path.join(REPO, "tools", "pack_videos.py")
    r = subprocess.run([sys.executable, tool, src, packed, "--store-size", "16", "--layout", "any"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert os.path.getsize(os.path.join(packed, "frames.u8")) == 5 * 16 * 16 * 3 and os.path.exists(os.path.join(packed, "index.json"))


# ---------------------------------------------------------------------------------------------
# working size, on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_working_size_on_the_device():
    """B = 32 pairs, 256 -> 128, jitter on, flips mixed, every second pair a 256 x 192 picture inside the padded square."""
    from cvpr23_lfdm_amd import _native
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native._set_library_for_tests(None)
    rng = np.random.RandomState(1)
    ys, xs = np.mgrid[0:256, 0:256]
    store = np.zeros((40, 256, 256, 3), np.uint8)
    for i in range(40):
        if i % 4 == 1:
            f = rng.randint(0, 256, (256, 256, 3))
        else:
            f = np.stack([(xs + 3 * i) % 256, (ys * (i + 1) // 8) % 256, (xs + ys + 5 * i) // 2 % 256], -1)
        if i >= 20:                                                          # rows 20 .. 39: 256 x 192 pictures at x0 = 32
            store[i, :, 32:224] = f[:, 32:224]
        else:
            store[i] = f
    pairs, valid = [], []
    for b in range(32):
        base = 20 * (b % 2)
        pairs.append((base + (7 * b + 3) % 20, base + (11 * b + (19 if b == 5 else 0)) % 20))
        valid.append([0, 32, 256, 192] if b % 2 else [0, 0, 256, 256])
    pairs[4] = (19, 19)
    pairs[31] = (39, 20)
    flips = [(b // 2 + b // 5) % 2 for b in range(32)]
    assert 8 < sum(flips) < 24 and len({(f, b % 2) for b, f in enumerate(flips)}) == 4
    factors = _factors(32, start=3)
    got = _prep("cuda", store, pairs, 128, factors, flips, valid=valid)
    _assert_pair(got, _yardstick_batch(store, pairs, 128, factors, flips, valid=valid), "working size")
