"""Packed uint8 video store and on-device batch preparation (csrc/video_prep.hip, cvpr23_lfdm_amd/video_store.py).

The yardstick is the existing host path and nothing else: `_yardstick` below is the body of data.FrameFolderVideos.__getitem__
(data.color_jitter -> io_compat.resize(float32, INTER_AREA) - mean -> transpose -> / 255 as float32) with the four jitter factors
replayed instead of drawn.  The contract is torch.equal: bit-identical float32, no tolerance and no share of excused pixels.  The one
place with a bound is a store that was itself shrunk when packed, WITHOUT jitter: its single rounding to a byte, 0.5 / 255 (+ 1e-6 for
the float32 arithmetic around it).  With jitter such a store is compared to the host arithmetic on the stored bytes (torch.equal again);
its distance to the host path on the larger originals is only printed, because no such bound exists.
"""
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from cvpr23_lfdm_amd import data, io_compat, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEANS = ((0.0, 0.0, 0.0), (104.5, 117.25, 123.0))
BF = (1 - 64 / 255, 1.0, 1 + 64 / 255)
CSF = (0.75, 1.0, 1.25)
SHIFTS = (-10, 0, 10)
# colours whose hue needs PIL's exact float / double mix (hue 156, 134, 152, 184)
BOUNDARY = ((15, 41, 100), (15, 141, 168), (168, 200, 248), (27, 21, 38))


class _Replay:
    """Stands in for `random` in data.color_jitter: returns the recorded factors in draw order."""

    def __init__(self, values):
        self.values = list(values)

    def uniform(self, lo, hi):
        return self.values.pop(0)


def _hf(shift):
    """A hue factor with int(hf * 255) == shift."""
    hf = (shift + (0.5 if shift > 0 else -0.5 if shift < 0 else 0.0)) / 255.0
    assert int(hf * 255) == shift
    return hf


def _yardstick(frames, image_size, mean, factors=None):
    """frames: list of (S, S, 3) uint8 arrays of ONE video; factors (bf, cf, sf, shift) or None -> (3, T, H, W) float32 tensor."""
    if factors is not None:
        bf, cf, sf, shift = factors
        frames = data.color_jitter(frames, rnd=_Replay([bf, cf, sf, _hf(shift)]))
    mean = np.asarray(mean, np.float32)
    frames = [io_compat.resize(np.asarray(f, np.float32), image_size, interpolation=io_compat.INTER_AREA) - mean for f in frames]
    video = np.stack([np.transpose(f, (2, 0, 1)) for f in frames], axis=1)
    return torch.from_numpy(np.array(video / 255.0, dtype=np.float32))


def _yardstick_batch(store, index, image_size, mean, factors=None):
    return torch.stack([_yardstick([store[i] for i in row], image_size, mean, None if factors is None else factors[b])
                        for b, row in enumerate(index)])


def _store(s, seed=0):
    """Edge and ordinary frames at size s: noise, smooth, 0, 255, greys, primaries + secondaries, dark noise, boundary colours, noise."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:s, 0:s]
    smooth = np.stack([(xs * 255) // (s - 1), (ys * 255) // (s - 1), ((xs + ys) * 255) // (2 * s - 2)], -1)
    greys = np.repeat(((xs * 7 + ys * 13) % 256)[..., None], 3, -1)
    prim = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255)])
    prims = prim[(xs + 3 * ys) % 8]
    perms = np.array([p for c in BOUNDARY for p in itertools.permutations(c)])
    bound = perms[(xs + 5 * ys) % len(perms)]
    frames = [rng.randint(0, 256, (s, s, 3)), smooth, np.zeros((s, s, 3)), np.full((s, s, 3), 255), greys, prims,
              rng.randint(0, 3, (s, s, 3)) * (rng.rand(s, s, 1) < 0.3), bound, rng.randint(0, 256, (s, s, 3))]
    return np.ascontiguousarray(np.stack(frames).astype(np.uint8))


def _index(b, t, n, shift=0):
    """(b, t) rows with repeats, reversed order and the store's last row."""
    rows = [[(n - 1 - (i + shift + 2 * bb)) % n for i in range(t)] for bb in range(b)]
    if t > 1:
        rows[0][1] = rows[0][0]                     # a repeat; rows run downwards from the last row: reversed order
    assert rows[0][0] == (n - 1 - shift) % n
    return np.asarray(rows, np.int32)


def _factors(b, start=0):
    combos = list(itertools.product(BF, CSF, CSF, SHIFTS))
    # a stride coprime to 81 walks through every value of every factor within a few elements
    return [combos[(start + 31 * i) % len(combos)] for i in range(b)]


def _prep(dev, store, index, image_size, mean, factors=None, valid=None):
    st = torch.from_numpy(store).to(dev)
    idx = torch.from_numpy(np.asarray(index, np.int32))
    if factors is None:
        return ops.video_prep(st, idx, None, None, mean, image_size, False).cpu()
    params = torch.tensor([f[:3] for f in factors], dtype=torch.float32)
    shift = torch.tensor([f[3] for f in factors], dtype=torch.int32)
    v = None if valid is None else torch.tensor(valid, dtype=torch.int32)
    return ops.video_prep(st, idx, params, shift, mean, image_size, True, valid=v).cpu()


SHAPES = [(h, k) for h in (8, 12, 20) for k in (1, 2, 4)]


@pytest.mark.parametrize("image_size,k", SHAPES)
def test_jitter_off_equals_the_host_path(backend, image_size, k):
    store = _store(image_size * k, seed=image_size + k)
    for b, t, mean in itertools.product((1, 2), (1, 3), MEANS):
        index = _index(b, t, len(store), shift=0 if t > 1 else b - 1)
        got = _prep(backend, store, index, image_size, mean)
        want = _yardstick_batch(store, index, image_size, mean)
        assert got.dtype == torch.float32 and tuple(got.shape) == (b, 3, t, image_size, image_size)
        assert torch.equal(got, want), (b, t, mean, float((got - want).abs().max()))


@pytest.mark.parametrize("image_size,k", SHAPES)
def test_jitter_on_equals_the_host_path(backend, image_size, k):
    store = _store(image_size * k, seed=3 * image_size + k)
    n = len(store)
    case = 0
    for b, t, mean in itertools.product((1, 2), (1, 3), MEANS):
        # t = 1 would touch one store frame per element: walk the start so that every kind of frame is jittered at every shape
        for shift in (range(0, n, 2) if t == 1 else (0, 4)):
            index = _index(b, t, n, shift=shift)
            factors = _factors(b, start=7 * case + image_size + k)
            case += 1
            got = _prep(backend, store, index, image_size, mean, factors)
            want = _yardstick_batch(store, index, image_size, mean, factors)
            assert torch.equal(got, want), (b, t, mean, factors, float((got - want).abs().max()) * 255)


def test_jitter_every_factor_combination(backend):
    """All 81 combinations of the end points and 1.0 of the four factors, one batch element each, over every kind of frame."""
    store = _store(8, seed=5)
    factors = list(itertools.product(BF, CSF, CSF, SHIFTS))
    index = np.asarray([[(b + i) % len(store) for i in range(3)] for b in range(len(factors))], np.int32)
    got = _prep(backend, store, index, 8, MEANS[1], factors)
    want = _yardstick_batch(store, index, 8, MEANS[1], factors)
    assert torch.equal(got, want)


def _sweep_frames():
    r, g = np.mgrid[0:256, 0:256]
    return np.ascontiguousarray(np.stack([np.stack([r, g, np.full_like(r, b)], -1) for b in (0, 38, 100, 248)]).astype(np.uint8))


def test_jitter_colour_sweep(backend):
    """Every (r, g) pair for four values of b through the HSV round trip with a non-zero shift (k = 1), and once more under factors
    that move every stage."""
    store = _sweep_frames()
    index = np.asarray([[0, 1, 2, 3], [3, 2, 1, 0]], np.int32)
    factors = [(1.0, 1.0, 1.0, 10), (BF[2], 0.75, 1.25, -10)]
    got = _prep(backend, store, index, 256, MEANS[0], factors)
    want = _yardstick_batch(store, index, 256, MEANS[0], factors)
    bad = (got != want)
    assert torch.equal(got, want), "%d of %d values differ" % (int(bad.sum()), bad.numel())


def test_a_frame_does_not_depend_on_its_batch(backend):
    """The contrast grey level and the factors are indexed by (b, t): a frame prepared alone equals the same frame inside a batch
    whose other frames and factors differ."""
    store = _store(16, seed=9)
    f_mine, f_other = (BF[0], 1.25, 0.75, 10), (BF[2], 0.75, 1.25, -10)
    for k in (1, 2):
        alone = _prep(backend, store, [[0]], 16 // k, MEANS[1], [f_mine])
        batch = _prep(backend, store, [[3, 7, 1], [5, 0, 8], [2, 2, 6]], 16 // k, MEANS[1], [f_other, f_mine, f_other])
        assert torch.equal(batch[1, :, 1], alone[0, :, 0])
        swapped = _prep(backend, store, [[0, 3, 7], [5, 8, 1]], 16 // k, MEANS[1], [f_mine, f_other])
        assert torch.equal(swapped[0, :, 0], alone[0, :, 0])


def test_padding_is_not_jittered(backend):
    """A non-square video is zero-padded AFTER the jitter on the host: with the picture rectangle given, the padding stays black and
    the contrast mean is the picture's alone."""
    rng = np.random.RandomState(2)
    pics = [rng.randint(0, 256, (16, 12, 3)).astype(np.uint8) for _ in range(2)]
    store = np.zeros((2, 16, 16, 3), np.uint8)
    store[:, :, 2:14] = np.stack(pics)
    factors = [(BF[0], 0.75, 1.25, 10)]
    got = _prep(backend, store, [[1, 0]], 16, MEANS[1], factors, valid=[[0, 2, 16, 12]])
    assert torch.equal(got, _yardstick(pics[::-1], 16, MEANS[1], factors[0])[None])


# ---------------------------------------------------------------------------------------------
# store round trip (host + emulator)
# ---------------------------------------------------------------------------------------------
def _write_videos(root, scale):
    """Four videos under root/<label>/<video>/: RGB, grayscale, non-square (4 : 3) and one shorter than num_frames; frame size 16 * scale."""
    rng = np.random.RandomState(11)
    s = 16 * scale

    def smooth(h, w, c, n):
        # blocks of 4 * scale pixels: an area shrink by `scale` (and by 4 * scale) averages equal values, plus a little noise
        base = rng.randint(0, 256, (n, h // (4 * scale), w // (4 * scale), c))
        up = np.repeat(np.repeat(base, 4 * scale, 1), 4 * scale, 2)
        return np.clip(up + rng.randint(-6, 7, up.shape), 0, 255).astype(np.uint8)

    plan = {("happy", "v0"): smooth(s, s, 3, 6), ("happy", "v1"): smooth(s, s, 1, 5)[..., 0], ("sad", "v0"): smooth(s, 3 * s // 4, 3, 7),
            ("sad", "v1"): smooth(s, s, 3, 2)}
    for (label, vid), frames in plan.items():
        d = os.path.join(root, label, vid)
        os.makedirs(d)
        for i, f in enumerate(frames):
            io_compat.imsave(os.path.join(d, "%03d.png" % i), f)


@pytest.fixture
def emu_lib():
    from cvpr23_lfdm_amd import _build, _native
    _native._set_library_for_tests(_native.NativeLibrary(_build.build_emu(), "emu"))
    yield
    _native._set_library_for_tests(None)


def _both_paths(src, store_dir, image_size, jitter, resident=False, mean=MEANS[1], seed=4, epochs=1, pin=False):
    from torch.utils.data import DataLoader
    from cvpr23_lfdm_amd import video_store
    ref_ds = data.FrameFolderVideos(src, image_size=image_size, num_frames=4, sampling="uniform", mean=mean, jitter=jitter)
    ds = video_store.PackedVideos(store_dir, image_size=image_size, num_frames=4, sampling="uniform", mean=mean, jitter=jitter,
                                  resident=resident)
    assert len(ds) == len(ref_ds) == 4
    random.seed(seed)
    ref = [ref_ds[i] for i in range(len(ref_ds))]
    random.seed(seed)
    prep = video_store.DevicePrep(ds)
    for _ in range(epochs):          # (more than one only without jitter: every epoch must give the same tensors from the reused buffers)
        got, labels, names = [], [], []
        for batch in DataLoader(ds, batch_size=2, shuffle=False, pin_memory=pin):
            vids = prep(batch)
            assert vids.dtype == torch.float32 and tuple(vids.shape) == (2, 3, 4, image_size, image_size)
            got.append(vids)
            labels += list(batch[3])
            names += list(batch[4])
        assert labels == [r[1] for r in ref] and names == [r[2] for r in ref]
    return torch.cat(got).cpu(), torch.stack([torch.from_numpy(r[0]) for r in ref])


def test_store_round_trip(tmp_path, emu_lib):
    from cvpr23_lfdm_amd import video_store
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_videos(src, 1)
    index = video_store.pack_frame_folders(src, packed, 16)
    assert index["frames"] == 20 and index["store_size"] == 16 and os.path.getsize(os.path.join(packed, "frames.u8")) == 20 * 16 * 16 * 3
    assert [v["valid"] for v in index["videos"]] == [[0, 0, 16, 16], [0, 0, 16, 16], [0, 2, 16, 12], [0, 0, 16, 16]]
    got, want = _both_paths(src, packed, 16, jitter=False)
    assert torch.equal(got, want)
    got, want = _both_paths(src, packed, 16, jitter=True)          # same seed, same draw order: the same factors
    assert torch.equal(got, want)
    assert not torch.equal(got, _both_paths(src, packed, 16, jitter=True, seed=5)[0])


def test_store_shrunk_when_packed(tmp_path, emu_lib):
    """Sources at 4 x, store at 2 x the training size: the two paths differ by the store's one rounding to a byte and no more."""
    from cvpr23_lfdm_amd import video_store
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_videos(src, 4)                                           # 64 x 64 (and 64 x 48) sources
    video_store.pack_frame_folders(src, packed, 32)
    got, want = _both_paths(src, packed, 16, jitter=False)
    err = float((got - want).abs().max())
    print("max abs difference %.3e (bound %.3e)" % (err, 0.5 / 255 + 1e-6))
    assert err <= 0.5 / 255 + 1e-6
    assert err > 0                                                  # the sources are noisy: the rounding is really exercised


def test_store_shrunk_when_packed_jitter_runs_at_store_resolution(tmp_path, emu_lib):
    """With jitter the 0.5 / 255 bound does NOT carry over to a store packed smaller than its sources: the device jitters the stored
    (shrunk, rounded) bytes, the host jitters the full-size frames and shrinks afterwards, and every jitter stage is non-linear
    (truncation, clamps, the contrast grey level of another resolution, the 8-bit HSV round trip).  What holds, and is asserted, is
    that the result is bit for bit the host arithmetic applied to the STORED picture.  The distance to the host path on the 64 x 64
    originals is printed, not bounded: on these noisy frames it is 3 to 4 levels of 255 (store 32 -> 16, seeds 4, 5, 6)."""
    from cvpr23_lfdm_amd import video_store
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_videos(src, 4)
    video_store.pack_frame_folders(src, packed, 32)
    for seed in (4, 5, 6):
        got, on_originals = _both_paths(src, packed, 16, jitter=True, seed=seed)
        ds = video_store.PackedVideos(packed, image_size=16, num_frames=4, sampling="uniform", mean=MEANS[1], jitter=True)
        random.seed(seed)
        on_store = []
        for frames, params, shift, _, _, (y0, x0, h, w) in (ds[i] for i in range(len(ds))):
            factors = tuple(float(p) for p in params) + (int(shift),)
            on_store.append(_yardstick([f[y0:y0 + h, x0:x0 + w] for f in frames], 16, MEANS[1], factors))
        assert torch.equal(got, torch.stack(on_store))
        print("seed %d: jitter at store resolution is %.2f levels of 255 from jitter on the originals"
              % (seed, float((got - on_originals).abs().max()) * 255))


def test_resident_equals_staged(tmp_path, emu_lib):
    from cvpr23_lfdm_amd import video_store
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_videos(src, 2)
    video_store.pack_frame_folders(src, packed, 32)
    for jitter in (False, True):
        staged, _ = _both_paths(src, packed, 16, jitter=jitter)
        resident, _ = _both_paths(src, packed, 16, jitter=jitter, resident=True)
        assert torch.equal(staged, resident)
    item = video_store.PackedVideos(packed, image_size=16, num_frames=4, resident=True)[3]
    assert item[0].dtype == np.int32 and item[0].tolist() == [18, 19, 19, 19]          # the short video repeats its last frame
    item = video_store.PackedVideos(packed, image_size=16, num_frames=4)[3]
    assert item[0].dtype == np.uint8 and item[0].shape == (4, 32, 32, 3) and item[1].tolist() == [1, 1, 1] and int(item[2]) == 0


@pytest.mark.gpu
def test_device_prep_on_the_device(tmp_path):
    """The staged path's pinned buffers (each refilled in the second epoch while the device may still hold its last copy) and the
    resident store, on the product library."""
    from cvpr23_lfdm_amd import _native, video_store
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native._set_library_for_tests(None)
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_videos(src, 1)
    video_store.pack_frame_folders(src, packed, 16)
    for resident in (False, True):
        got, want = _both_paths(src, packed, 16, jitter=False, resident=resident, epochs=2)
        assert torch.equal(got, want)
        got, want = _both_paths(src, packed, 16, jitter=True, resident=resident)
        assert torch.equal(got, want)
    # a loader that pins its batches (the trainer's): the bytes go up from the batch itself, without a second host copy
    for jitter, epochs in ((False, 2), (True, 1)):
        got, want = _both_paths(src, packed, 16, jitter=jitter, epochs=epochs, pin=True)
        assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refusals(backend, tmp_path):
    from cvpr23_lfdm_amd import video_store
    dev = backend
    store = torch.zeros(3, 16, 16, 3, dtype=torch.uint8, device=dev)
    idx = torch.zeros(1, 2, dtype=torch.int32)
    ok = ops.video_prep(store, idx, None, None, MEANS[0], 8, False)
    assert tuple(ok.shape) == (1, 3, 2, 8, 8) and float(ok.abs().max()) == 0.0
    with pytest.raises(ValueError, match="1, 2 or 4"):
        ops.video_prep(torch.zeros(1, 24, 24, 3, dtype=torch.uint8, device=dev), idx, None, None, MEANS[0], 8, False)
    with pytest.raises(ValueError, match="1, 2 or 4"):
        ops.video_prep(store, idx, None, None, MEANS[0], 12, False)
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.video_prep(torch.zeros(1, 18, 18, 3, dtype=torch.uint8, device=dev), idx, None, None, MEANS[0], 9, False)
    for bad in ([[0, 3]], [[-1, 0]]):
        with pytest.raises(IndexError, match="frame_index"):
            ops.video_prep(store, torch.tensor(bad, dtype=torch.int32), None, None, MEANS[0], 16, False)
    with pytest.raises(ValueError, match="frame_index"):
        ops.video_prep(store, idx.long(), None, None, MEANS[0], 16, False)
    with pytest.raises(ValueError, match="frame_index"):
        ops.video_prep(store, idx[0], None, None, MEANS[0], 16, False)
    with pytest.raises(ValueError, match="store_u8"):
        ops.video_prep(store.float(), idx, None, None, MEANS[0], 16, False)
    with pytest.raises(ValueError, match="store_u8"):
        ops.video_prep(store[..., :2], idx, None, None, MEANS[0], 16, False)
    params, shift = torch.ones(1, 3), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="params"):
        ops.video_prep(store, idx, torch.ones(2, 3), shift, MEANS[0], 16, True)
    with pytest.raises(ValueError, match="params"):
        ops.video_prep(store, idx, None, shift, MEANS[0], 16, True)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="NaN or an infinity"):
            ops.video_prep(store, idx, torch.tensor([[1.0, bad, 1.0]]), shift, MEANS[0], 16, True)
    with pytest.raises(ValueError, match="hue_shift"):
        ops.video_prep(store, idx, params, shift.float(), MEANS[0], 16, True)
    with pytest.raises(ValueError, match="valid"):
        ops.video_prep(store, idx, params, shift, MEANS[0], 16, True, valid=torch.tensor([[0, 8, 16, 12]], dtype=torch.int32))
    with pytest.raises(ValueError, match="mean"):
        ops.video_prep(store, idx, None, None, (0.0, 0.0), 16, False)
    with pytest.raises(ValueError, match="out"):
        ops.video_prep(store, idx, None, None, MEANS[0], 16, False, out=torch.empty(1, 3, 2, 8, 8, device=dev))
    # the store and the data set refuse what the kernel cannot shrink
    with pytest.raises(ValueError, match="multiple of 4"):
        video_store.pack_frame_folders(str(tmp_path), str(tmp_path / "p"), 18)
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_videos(src, 1)
    video_store.pack_frame_folders(src, packed, 16)
    for size in (16, 8):
        video_store.PackedVideos(packed, image_size=size)
    # the 16 x 12 video sits at x0 = 2 of the 16 x 16 stored frame: a 4 x 4 cell would mix picture and padding
    with pytest.raises(ValueError, match="mix picture and padding"):
        video_store.PackedVideos(packed, image_size=4)
    with pytest.raises(ValueError, match="1, 2 or 4"):
        video_store.PackedVideos(packed, image_size=12)
    with pytest.raises(ValueError, match="1, 2 or 4"):
        video_store.PackedVideos(packed, image_size=32)


def test_c_entry_point_checks_its_operands(backend):
    import ctypes as C
    from cvpr23_lfdm_amd import _native
    lib = _native.library()
    dev = backend
    store = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=dev)
    idx = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    params, shift = torch.ones(1, 3, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(1, 3, 2, 16, 16, device=dev)
    ws = torch.empty(8, dtype=torch.int32, device=dev)
    mean = (C.c_float * 3)(0, 0, 0)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = ops._stream(lib)
    assert lib.lfdm_video_prep_ws_bytes(1, 2) >= 8 and lib.lfdm_video_prep_ws_bytes(3, 40) >= 480
    assert lib.lfdm_video_prep_ws_bytes(0, 2) == 0

    def call(store=store, n=2, idx=idx, params=params, shift=shift, mean=mean, out=out, b=1, t=2, s=16, h=16, jitter=1, launches=3, ws=ws,
             ws_bytes=32):
        return lib.lfdm_video_prep_u8(p(store), n, p(idx), p(params), p(shift), None, mean, p(out), b, t, s, h, jitter, launches, p(ws),
                                      ws_bytes, stream)

    assert call() == 0 and call(jitter=0, params=None, shift=None, ws=None, ws_bytes=0) == 0
    for kw, what in ((dict(store=None), "null"), (dict(idx=None), "null"), (dict(out=None), "null"), (dict(mean=None), "null"),
                     (dict(params=None), "jitter needs"), (dict(shift=None), "jitter needs"), (dict(ws=None), "jitter needs"),
                     (dict(ws_bytes=4), "jitter needs"), (dict(b=0), ">= 1"), (dict(t=0), ">= 1"), (dict(n=0), ">= 1"),
                     (dict(s=18, h=18), "multiples of 4"), (dict(s=24, h=8), "1, 2 or 4"), (dict(s=16, h=12), "1, 2 or 4"),
                     (dict(s=8, h=16), "1, 2 or 4"), (dict(launches=0), "launches"), (dict(launches=4), "launches")):
        assert call(**kw) == -1, kw
        assert what in lib.lfdm_last_error().decode(), (kw, lib.lfdm_last_error())


def test_product_library_refuses_cpu_tensors():
    from cvpr23_lfdm_amd import _native
    _native._set_library_for_tests(None)
    store = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.video_prep(store, torch.zeros(1, 1, dtype=torch.int32), None, None, MEANS[0], 8, False)


def test_abi_stays_12_with_the_new_symbols():
    from cvpr23_lfdm_amd import _build, _native
    header = open(os.path.join(REPO, "include", "lfdm_hip.h")).read()
    for sym in ("lfdm_video_prep_u8", "lfdm_video_prep_ws_bytes"):
        assert sym in _native.EXPORTED_SYMBOLS and ("%s(" % sym) in header
    assert _native.NativeLibrary(_build.build_hip(), "hip").lfdm_abi_version() == 14          # (12 when the entry point was added; 13: lfdm_sampler_step_params; 14: lfdm_train_loss_params)


# ---------------------------------------------------------------------------------------------
# tools/train_dm.py --packed
# ---------------------------------------------------------------------------------------------
def _train_dm():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_dm_under_test", os.path.join(REPO, "tools", "train_dm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_dm_packed_flag(tmp_path, emu_lib):
    from cvpr23_lfdm_amd import video_store
    mod = _train_dm()
    args = mod.parse_args(["--packed", "DIR", "--resident"])
    assert args.packed == "DIR" and args.resident
    args = mod.parse_args(["--data", "X"])
    assert args.packed == "" and not args.resident
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_videos(src, 1)
    video_store.pack_frame_folders(src, packed, 16)
    # without --packed: the parent's data set, constructed as the parent constructs it, and no preparation step
    ds, prep = mod.make_dataset(mod.parse_args(["--data", src, "--size", "16", "--frames", "4"]))
    assert type(ds) is data.FrameFolderVideos and prep is None
    assert (ds.image_size, ds.num_frames, ds.sampling, ds.jitter, ds.mean.tolist()) == (16, 4, "random", True, [0, 0, 0])
    ds, prep = mod.make_dataset(mod.parse_args(["--synthetic", "--size", "16", "--frames", "4"]))
    assert type(ds) is data.SyntheticVideos and prep is None
    ds, prep = mod.make_dataset(mod.parse_args(["--packed", packed, "--resident", "--size", "16", "--frames", "4"]))
    assert type(ds) is video_store.PackedVideos and ds.resident and ds.jitter and ds.sampling == "random"
    assert isinstance(prep, video_store.DevicePrep) and tuple(prep.store.shape) == (20, 16, 16, 3)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "train_dm.py"), "--help"], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--packed" in r.stdout and "--resident" in r.stdout


def test_pack_videos_tool(tmp_path):
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_videos(src, 1)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "pack_videos.py"), src, packed, "--store-size", "16"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert os.path.getsize(os.path.join(packed, "frames.u8")) == 20 * 16 * 16 * 3 and os.path.exists(os.path.join(packed, "index.json"))


# ---------------------------------------------------------------------------------------------
# working size, on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_working_size_on_the_device():
    """B = 2, T = 40, 256 -> 128, jitter on: the per-frame integer sums and the grid at real extents."""
    from cvpr23_lfdm_amd import _native
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _native._set_library_for_tests(None)
    rng = np.random.RandomState(1)
    ys, xs = np.mgrid[0:256, 0:256]
    store = np.empty((50, 256, 256, 3), np.uint8)
    for i in range(50):
        if i % 2:
            store[i] = rng.randint(0, 256, (256, 256, 3))
        else:
            store[i] = np.stack([(xs + 3 * i) % 256, (ys * (i + 1) // 8) % 256, (xs + ys + 5 * i) // 2 % 256], -1)
    index = np.stack([np.arange(49, 9, -1), np.r_[np.arange(0, 39), 49]]).astype(np.int32)
    factors = [(BF[0], 1.25, 0.75, 10), (BF[2], 0.75, 1.25, -10)]
    got = _prep("cuda", store, index, 128, MEANS[1], factors)
    want = _yardstick_batch(store, index, 128, MEANS[1], factors)
    bad = got != want
    assert torch.equal(got, want), "%d of %d values differ" % (int(bad.sum()), bad.numel())
