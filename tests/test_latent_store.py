"""The flow-latent store and the DM training step that reads it (csrc/latent_gather.hip, cvpr23_lfdm_amd/video_store.py,
FlowDiffusion.set_train_latent).

The yardsticks are the code that exists: FlowDiffusion._latent_of's expressions in eager torch for the gather kernel (torch.equal, no
tolerance), model.encode_video for the store builder, DevicePrep for the reference frame and the online step (set_train_input) for the
step from a stored latent.  Where a bar appears it is the suite's 1e-3 parity bar (tests/test_train_step.py).

The LFAE of configs/lfae_128.yaml needs 128-pixel frames (its predictors halve the frame five times) and the x86 emulator spends about
a minute on one such pass, so every check that is about the LFAE's VALUES runs on the GPU only.  The checks that are about the
plumbing around them - fingerprint refusal, the data set's draws, the reference frame, sharding, the trainer's loop - also run on the
emulator, at 16 pixels, with `_stand_in_pass` in place of FlowDiffusion._lfae_pass where a store has to be packed."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import synth
from layout import no_nan, window
from util import assert_close, record_margin

from cvpr23_lfdm_amd import io_compat, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((2, 2), (4, 4), (6, 6), (32, 32), (36, 36), (4, 8))
FRAMES, BATCHES = (1, 3, 40), (1, 2, 5)
STORE_ROWS = 7
DTYPES = {"f32": torch.float32, "f16": torch.float16}


# ---------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------
def _store(h, w, dtype, n=STORE_ROWS, seed=0):
    """(n, 3, h, w): grid planes around the identity's range, an occlusion plane in [0, 1]; fp16 stores hold values fp16 rounds."""
    g = torch.Generator().manual_seed(seed)
    st = torch.cat((torch.rand(n, 2, h, w, generator=g) * 2.6 - 1.3, torch.rand(n, 1, h, w, generator=g)), dim=1)
    return st.to(dtype).contiguous()


def _rows(b, t, n):
    """(b, t) rows that run downwards from the store's last row, with a repeat and the store's first row."""
    rows = [[(n - 1 - (i + 2 * bb)) % n for i in range(t)] for bb in range(b)]
    if t > 1:
        rows[0][1] = rows[0][0]
        assert rows[0][0] == n - 1
    rows[-1][-1] = 0
    return torch.tensor(rows, dtype=torch.int32)


def _want(store, rows, residual):
    """FlowDiffusion._latent_of in eager torch on the gathered rows (an fp16 store as store.float())."""
    from cvpr23_lfdm_amd import FlowDiffusion
    g = store.float()[rows.long()].permute(0, 2, 1, 3, 4)          # (B, 3, T, h, w)
    grid, conf = g[:, :2], g[:, 2:3]
    if residual:
        b, _, nf, h, w = grid.shape
        grid = grid - FlowDiffusion.get_grid(None, b, nf, h, w, normalize=True)
    return torch.cat((grid, conf * 2 - 1), dim=1).contiguous()


def _nan_out(shape, dev):
    """`out` of `shape` inside a buffer of NaNs, itself NaN: (out, check) - check() asserts that nothing outside out has changed."""
    total = int(np.prod(shape))
    view, check = window((1, total), ld_extra=8, col_off=4, guard_rows=1, device=dev)
    out = view[0].view(shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == 0 and bool(torch.isnan(out).all())
    return out, check


@pytest.mark.parametrize("residual", [False, True], ids=["copy", "residual"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_gather_equals_indexing(backend, hw, dtype, residual):
    """One quad per plane (2 x 2), fewer threads than a wave, a partly empty last chunk (36 x 36: 972 quads in chunks of 256), a
    non-square plane; every frame count and batch size of the issue; bit for bit, nothing left unwritten, nothing written outside."""
    dev, (h, w) = backend, hw
    store = _store(h, w, DTYPES[dtype])
    sd = store.to(dev)
    for t in FRAMES:
        for b in BATCHES:
            rows = _rows(b, t, STORE_ROWS)
            assert int(rows.max()) == STORE_ROWS - 1 or b * t == 1
            out, check = _nan_out((b, 3, t, h, w), dev)
            got = ops.latent_gather(sd, rows, residual, out=out)
            assert got is out
            no_nan(out, "latent_gather %s" % ((b, t, h, w),))
            check("latent_gather %s" % ((b, t, h, w),))
            assert torch.equal(out.cpu(), _want(store, rows, residual)), (b, t, h, w, dtype, residual)
    fresh = ops.latent_gather(sd, _rows(2, 3, STORE_ROWS).to(dev), residual)          # a device table, an allocated result
    assert torch.equal(fresh.cpu(), _want(store, _rows(2, 3, STORE_ROWS), residual))


def test_fp16_store_is_read_as_its_float_values(backend):
    """Every finite fp16 bit pattern (and the two infinities) comes out as store.float() says: the conversion is exact."""
    dev = backend
    bits = torch.from_numpy(np.arange(1 << 16, dtype=np.uint16).view(np.float16).copy())
    bits = bits[~torch.isnan(bits)]
    assert bool(torch.isinf(bits).any()) and bits.numel() == (1 << 16) - 2 * 1023
    n = (bits.numel() + 11) // 12
    store = torch.zeros(n * 12, dtype=torch.float16)
    store[:bits.numel()] = bits
    store = store.view(n, 3, 2, 2)
    rows = torch.arange(n, dtype=torch.int32).view(1, n)
    got = ops.latent_gather(store.to(dev), rows, False).cpu()
    want = store.float().permute(1, 0, 2, 3).unsqueeze(0)
    assert torch.equal(got[:, :2], want[:, :2]) and torch.equal(got[:, 2], want[:, 2] * 2 - 1)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_gather_twice_same_bits(backend, dtype):
    dev = backend
    store, rows = _store(36, 36, DTYPES[dtype], seed=3).to(dev), _rows(5, 40, STORE_ROWS)
    a = ops.latent_gather(store, rows, True)
    b = ops.latent_gather(store, rows, True)
    assert torch.equal(a, b) and not bool(torch.isnan(a).any())


def test_refusals_write_nothing(backend):
    from cvpr23_lfdm_amd import _native
    dev = backend
    lib = _native.library()
    h = w = 4
    store = _store(h, w, torch.float32).to(dev)
    rows = _rows(2, 3, STORE_ROWS).to(dev)
    ix, iy = ops._identity_table(w, store.device), ops._identity_table(h, store.device)
    out, check = _nan_out((2, 3, 3, h, w), dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = ops._stream(lib)

    def call(store=store, code=0, n=STORE_ROWS, rows=rows, ix=None, iy=None, out=out, b=2, t=3, h=h, w=w):
        return lib.lfdm_latent_gather_f32(p(store), code, n, p(rows), p(ix), p(iy), p(out), b, t, h, w, stream)

    for kw, what in ((dict(code=2), "store_dtype"), (dict(code=-1), "store_dtype"), (dict(h=3, w=3), "multiple of 4"), (dict(h=2, w=3), "multiple of 4"),
                     (dict(ix=ix), "come together"), (dict(iy=iy), "come together"), (dict(n=0), ">= 1"), (dict(n=-5), ">= 1"),
                     (dict(t=65536), "65535"), (dict(b=65536), "65535"), (dict(b=0), ">= 1"), (dict(t=0), ">= 1"), (dict(h=0), ">= 1"),
                     (dict(store=None), "null"), (dict(rows=None), "null"), (dict(out=None), "null")):
        assert call(**kw) == -1, kw
        assert what in lib.lfdm_last_error().decode(), (kw, lib.lfdm_last_error())
        assert bool(torch.isnan(out).all()), kw
        check(str(kw))
    if dev == "cuda":
        torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the Python face: an out-of-range row is refused on the host, before anything is launched
    for bad in ([[0, STORE_ROWS]], [[-1, 0]]):
        with pytest.raises(ValueError, match="rows holds"):
            ops.latent_gather(store, torch.tensor(bad, dtype=torch.int32), False, out=out.view(-1)[:2 * 3 * h * w].view(1, 3, 2, h, w))
    assert bool(torch.isnan(out).all())
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.latent_gather(torch.zeros(2, 3, 3, 3, device=dev), torch.zeros(1, 1, dtype=torch.int32), False)
    with pytest.raises(ValueError, match="int32"):
        ops.latent_gather(store, rows.long(), False)
    with pytest.raises(ValueError, match="store must be"):
        ops.latent_gather(store.double(), rows, False)
    with pytest.raises(ValueError, match="store must be"):
        ops.latent_gather(store[:, :2], rows, False)
    assert call() == 0 and call(ix=ix, iy=iy) == 0          # (the accepted forms of the same operands)


@pytest.mark.gpu
def test_store_addressing_is_64_bit():
    """A store just past 4 GiB: 349 527 fp32 frames of 32 x 32, uninitialised but for its last two rows."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 349527
    assert n * 3 * 32 * 32 * 4 > (1 << 32)
    try:
        store = torch.empty((n, 3, 32, 32), dtype=torch.float32, device="cuda")
    except RuntimeError as e:          # (torch.cuda.OutOfMemoryError is one)
        pytest.skip("no room for a 4 GiB store: %s" % (str(e).splitlines()[0],))
    last = _store(32, 32, torch.float32, n=2, seed=9)
    store[n - 2:] = last.cuda()
    rows = torch.tensor([[n - 1, n - 2, n - 1]], dtype=torch.int32)
    for residual in (False, True):
        got = ops.latent_gather(store, rows, residual).cpu()
        assert torch.equal(got, _want(last, torch.tensor([[1, 0, 1]], dtype=torch.int32), residual))
    del store
    torch.cuda.empty_cache()


def test_header_and_abi():
    import re
    from cvpr23_lfdm_amd import _native
    header = open(os.path.join(REPO, "include", "lfdm_hip.h")).read()
    assert "lfdm_latent_gather_f32" in _native.EXPORTED_SYMBOLS
    decl = re.search(r"/\* Layout:([^*]*)\*/\s*(?:#define[^\n]*\n)*int lfdm_latent_gather_f32\(([^;]*)\)\s*;", header)
    assert decl and "dense" in decl.group(1)
    assert "#define LFDM_LATENT_F32 0" in header and "#define LFDM_LATENT_F16 1" in header
    assert ops.LATENT_DTYPES == (torch.float32, torch.float16)


# ---------------------------------------------------------------------------------------------
# the store builder, the data set and the preparation step
# ---------------------------------------------------------------------------------------------
MULTS = (1, 2)          # a two-level denoiser wherever the check is not about the denoiser's size


def _model(dev, hw, frames, *, gen_seed=4321, mults=MULTS, **kw):
    from cvpr23_lfdm_amd import FlowDiffusion
    kw.setdefault("null_cond_prob", 0.0)
    m = FlowDiffusion(img_size=hw // 4, num_frames=frames, sampling_timesteps=5, timesteps=1000, is_train=True, lr=1e-4,
                      config_pth=synth.CONFIG, pretrained_pth="", dim_mults=mults, **kw)
    m.unet.load_state_dict(synth.unet_state(dim_mults=mults))
    m.generator.load_state_dict(synth.generator_state(gen_seed))
    m.region_predictor.load_state_dict(synth.region_state())
    m.bg_predictor.load_state_dict(synth.bg_state())
    for net in (m.generator, m.region_predictor, m.bg_predictor):
        net.eval()
        m.set_requires_grad(net, False)
    return m.to(dev)


def _stand_in_pass(self, real_vid, ref_img, decode):
    """In place of FlowDiffusion._lfae_pass where the check is not about the LFAE's values: maps that depend on every frame and on the
    reference frame, in the shapes and ranges of the real ones."""
    b, _, nf, hh, ww = real_vid.shape
    s = self.diffusion.image_size
    pool = lambda x: torch.nn.functional.adaptive_avg_pool2d(x.float(), s)
    vid = pool(real_vid.permute(0, 2, 1, 3, 4).reshape(b * nf, 3, hh, ww)).reshape(b, nf, 3, s, s).permute(0, 2, 1, 3, 4)
    vid = vid - pool(ref_img).unsqueeze(2) * 0.5
    return {"optical_flow": (vid[:, :2] * 2 - 1).contiguous(), "occlusion_map": vid[:, 2:3].clamp(0, 1).contiguous()}


def _write_videos(root, size, counts=(3, 7, 2)):
    """Videos of `counts` frames under root/<label>/<video>/: smooth random frames of size x size, each a shifted mix of its first."""
    rng = np.random.RandomState(5)
    up = lambda a: np.repeat(np.repeat(a, size // 8, 0), size // 8, 1)
    for v, count in enumerate(counts):
        d = os.path.join(root, "happy" if v % 2 == 0 else "sad", "v%d" % v)
        os.makedirs(d)
        base = up(rng.randint(0, 256, (8, 8, 3))).astype(np.float32)
        for i in range(count):
            f = 0.7 * np.roll(base, (2 * i + 1, -i), (0, 1)) + 0.3 * up(rng.randint(0, 256, (8, 8, 3)))
            io_compat.imsave(os.path.join(d, "%03d.png" % i), np.clip(f, 0, 255).astype(np.uint8))


def _collate(items):
    from torch.utils.data import default_collate
    return default_collate(items)


def _packed(tmp_path, dev, monkeypatch, frames, **pack_kw):
    """(model, store dir, image size): a frame store of three videos (3, 7 and 2 frames) and its latent store - the real LFAE at
    128 pixels on the GPU, `_stand_in_pass` at 16 pixels on the emulator."""
    from cvpr23_lfdm_amd import FlowDiffusion, video_store
    size = 128 if dev == "cuda" else 16
    src, packed = str(tmp_path / "src"), str(tmp_path / "packed")
    _write_videos(src, size)
    video_store.pack_frame_folders(src, packed, size)
    model = _model(dev, size, frames)
    with monkeypatch.context() as mp:
        if dev != "cuda":
            mp.setattr(FlowDiffusion, "_lfae_pass", _stand_in_pass)
        meta = video_store.pack_latents(model, packed, image_size=size, **pack_kw)
    assert meta["frames"] == 12 and meta["latent_size"] == size // 4 and meta["dtype"] == pack_kw.get("dtype", "f32")
    assert json.load(open(os.path.join(packed, "latents.json"))) == meta
    return model, packed, size


@pytest.mark.gpu
def test_packed_latent_is_encode_video():
    """A video of exactly T frames: the stored fp32 latent, gathered under uniform sampling and passed through the kernel, IS
    model.encode_video of the same prepared frames, for both residual settings; the fp16 store is that within half an fp16 ulp; a
    chunked pack of the 7-frame video is within the 1e-3 parity bar of its one-pass latent."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tempfile
    from cvpr23_lfdm_amd import video_store
    dev, size, t = "cuda", 128, 3
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "src")
        _write_videos(src, size)
        stores = {}
        model = _model(dev, size, t)
        for name, kw in (("one", dict(dtype="f32")), ("chunked", dict(dtype="f32", chunk_frames=3)), ("half", dict(dtype="f16"))):
            stores[name] = os.path.join(tmp, name)
            video_store.pack_frame_folders(src, stores[name], size)
            video_store.pack_latents(model, stores[name], image_size=size, **kw)
        pv = video_store.PackedVideos(stores["one"], image_size=size, num_frames=t, sampling="uniform")
        vid = video_store.DevicePrep(pv)(_collate([pv[0]]))
        assert pv.videos[0]["count"] == t
        for residual in (False, True):
            model.use_residual_flow = residual
            want = model.encode_video(vid, vid[:, :, 0])
            for resident in (False, True):
                ds = video_store.PackedLatents(stores["one"], image_size=size, num_frames=t, sampling="uniform", resident=resident, model=model)
                latent, ref = video_store.DeviceLatentPrep(ds)(_collate([ds[0]]))
                assert torch.equal(latent, want), (residual, resident)
                assert torch.equal(ref, vid[:, :, 0])
            ds = video_store.PackedLatents(stores["half"], image_size=size, num_frames=t, sampling="uniform", model=model)
            half = video_store.DeviceLatentPrep(ds)(_collate([ds[0]]))[0]
            # one rounding of the stored raw value v to fp16: |error| <= 2^-11 |v| (half an ulp), doubled on the occlusion channel (* 2);
            # 1e-6: the fp32 roundings of v - identity and occ * 2 - 1 on both sides (results below 4: half an ulp is 1.2e-7 each)
            raw = torch.from_numpy(np.array(video_store.PackedLatents(stores["one"], image_size=size, num_frames=t, model=model).latents[:t]))
            bound = float(raw.abs().max()) * 2.0 ** -11 * 2 + 1e-6
            err = float((half - want).abs().max())
            print("fp16 store against encode_video, residual=%s: %.3g, bound %.3g" % (residual, err, bound))
            assert err <= bound
        model.use_residual_flow = False
        one = video_store.PackedLatents(stores["one"], image_size=size, num_frames=t, model=model)
        chunked = video_store.PackedLatents(stores["chunked"], image_size=size, num_frames=t, model=model)
        v = next(v for v in one.videos if v["count"] == 7)
        assert one.videos[0]["first"] == 0 and one.videos[0]["count"] == 3
        sl = slice(v["first"], v["first"] + 7)
        assert np.array_equal(one.latents[:3], chunked.latents[:3])          # (3 frames: one pass in both)
        assert_close(torch.from_numpy(np.array(chunked.latents[sl])), torch.from_numpy(np.array(one.latents[sl])), 1e-3,
                     "chunked pack (3 + 3 + 1 frames) against one pass of 7")


def test_a_store_of_another_lfae_is_refused(backend, tmp_path, monkeypatch):
    from cvpr23_lfdm_amd import video_store
    dev = backend
    model, packed, size = _packed(tmp_path, dev, monkeypatch, 3)
    kw = dict(image_size=size, num_frames=3)
    ds = video_store.PackedLatents(packed, model=model, **kw)
    assert len(ds) == 3 and ds.latent_size == size // 4 and not ds.residual
    assert len(video_store.PackedLatents(packed, fingerprint=video_store.lfae_fingerprint(model), residual=True, **kw)) == 3
    other = _model(dev, size, 3, gen_seed=99)
    assert video_store.lfae_fingerprint(other) != video_store.lfae_fingerprint(model)
    with pytest.raises(ValueError, match="another LFAE"):
        video_store.PackedLatents(packed, model=other, **kw)
    switched = _model(dev, size, 3)
    switched.lfae_config = dict(switched.lfae_config, revert_axis_swap=not switched.lfae_config["revert_axis_swap"])
    with pytest.raises(ValueError, match="another LFAE"):          # same weights, another switch of the config
        video_store.PackedLatents(packed, model=switched, **kw)
    with pytest.raises(ValueError, match="mean"):
        video_store.PackedLatents(packed, model=model, mean=(1.0, 0, 0), **kw)
    with pytest.raises(ValueError, match="exactly one"):
        video_store.PackedLatents(packed, **kw)
    wrong = _model(dev, 2 * size, 3)          # (the same LFAE in front of a denoiser of another latent size)
    with pytest.raises(ValueError, match="denoises"):
        video_store.PackedLatents(packed, model=wrong, **kw)


@pytest.mark.parametrize("resident", [False, True], ids=["staged", "resident"])
def test_reference_frame_and_draws_are_device_preps(backend, tmp_path, monkeypatch, resident):
    """Same seeds, jitter on, sampling "random": PackedLatents draws what PackedVideos draws, DeviceLatentPrep's ref_img is
    DevicePrep(...)[:, :, 0] bit for bit, and its latent is the stored rows through _latent_of."""
    from torch.utils.data import DataLoader
    from cvpr23_lfdm_amd import video_store
    dev = backend
    model, packed, size = _packed(tmp_path, dev, monkeypatch, 3)
    model.use_residual_flow = True
    kw = dict(image_size=size, num_frames=3, sampling="random", jitter=True, mean=(0, 0, 0))
    pv = video_store.PackedVideos(packed, resident=True, **kw)
    pl = video_store.PackedLatents(packed, resident=resident, model=model, **kw)
    outs, latent_prep = [], video_store.DeviceLatentPrep(pl)
    for ds, prep in ((pv, video_store.DevicePrep(pv)), (pl, latent_prep)):
        random.seed(4)
        np.random.seed(4)
        outs.append([(batch, prep(batch)) for batch in DataLoader(ds, batch_size=2, shuffle=False)])
    raw = torch.from_numpy(np.array(pl.latents))
    for (bv, vids), (bl, (latent, ref)) in zip(*outs):
        assert torch.equal(bv[0].to(torch.int32), bl[0]) and torch.equal(bv[1], bl[3]) and torch.equal(bv[2], bl[4])
        assert list(bv[3]) == list(bl[5]) and list(bv[4]) == list(bl[6])
        assert torch.equal(ref, vids[:, :, 0])
        assert torch.equal(latent.cpu(), _want(raw, bl[0], True))
        assert torch.equal(latent_prep.real_frames(bl), vids)          # (what the trainer decodes against at --save-img-freq)
    assert len(outs[0]) == len(outs[1]) == 2


# ---------------------------------------------------------------------------------------------
# the training step
# ---------------------------------------------------------------------------------------------
def _flat(model, what):
    return torch.cat([(p.grad if what == "grad" else p.detach()).reshape(-1) for p in model.diffusion.parameters()])


def _two_steps(b, t, **kw):
    """(online model, latent model, real_vid) after one optimizer step each from identical weights and seeds."""
    dev, hw = "cuda", 128
    ref_img, real_vid, cond, _, _ = synth.train_inputs(b, t, hw)
    ref_img, real_vid, cond = ref_img.to(dev), real_vid.to(dev), cond.to(dev)
    online, stored = _model(dev, hw, t, **kw), _model(dev, hw, t, **kw)
    torch.manual_seed(5)
    online.set_train_input(ref_img=ref_img, real_vid=real_vid, ref_text=cond)
    online.optimize_parameters()
    latent = stored.encode_video(real_vid, ref_img)
    torch.manual_seed(5)
    stored.set_train_latent(ref_img, latent, cond)
    stored.optimize_parameters()
    return online, stored, real_vid


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "residual-p05", "known_train", "full-unet"])
def test_latent_step_is_the_online_step(variant):
    """B = 1: the same launches on the same bits - loss, pred_x0, the flat gradient and the updated weights are torch.equal."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    kw = {"plain": {}, "residual-p05": dict(use_residual_flow=True, null_cond_prob=0.5, only_use_flow=False),
          "known_train": dict(known_train=dict(prob=1.0, kinds=("prefix", "random"), max_frames=2, seed=3)),
          "full-unet": dict(mults=(1, 2, 4, 8))}[variant]
    online, stored, real_vid = _two_steps(1, 3, **kw)
    assert torch.equal(stored.ref_img_fea, online.ref_img_fea)
    assert torch.equal(stored.loss, online.loss) and torch.isfinite(stored.loss)
    assert torch.equal(stored.diffusion.pred_x0, online.diffusion.pred_x0)
    assert torch.equal(_flat(stored, "grad"), _flat(online, "grad")) and float(_flat(stored, "grad").abs().max()) > 0
    assert torch.equal(_flat(stored, "weights"), _flat(online, "weights"))
    assert torch.equal(stored.fake_vid_grid, online.fake_vid_grid) and torch.equal(stored.fake_vid_conf, online.fake_vid_conf)
    assert_close(stored.real_vid_grid, online.real_vid_grid, 1e-6, "real_vid_grid back from the latent")
    assert_close(stored.real_vid_conf, online.real_vid_conf, 1e-6, "real_vid_conf back from the latent")


@pytest.mark.gpu
def test_latent_step_batch_of_two():
    """B = 2 at the 1e-3 bar of tests/test_train_step.py.  lr = 1e-4: Adam's first step moves a weight by at most lr, so even a sign flip
    of a vanishing gradient stays five times below the bar."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    online, stored, _ = _two_steps(2, 3)
    got, want = float(stored.loss), float(online.loss)
    record_margin("loss", abs(got - want), abs(want), 1e-3)
    assert abs(got - want) <= 1e-3 * max(1.0, abs(want))
    assert_close(stored.diffusion.pred_x0, online.diffusion.pred_x0, 1e-3, "pred_x0")
    ga, gb = _flat(stored, "grad"), _flat(online, "grad")
    scale = float(gb.abs().max()) + 1e-12
    assert_close(ga / scale, gb / scale, 1e-3, "flat gradient")
    assert_close(_flat(stored, "weights"), _flat(online, "weights"), 1e-3, "updated weights")


@pytest.mark.gpu
def test_latent_step_runs_nothing_of_the_lfae(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvpr23_lfdm_amd import FlowDiffusion
    dev, hw, t = "cuda", 128, 3
    ref_img, real_vid, cond, _, _ = synth.train_inputs(1, t, hw)
    ref_img, real_vid, cond = ref_img.to(dev), real_vid.to(dev), cond.to(dev)
    online, stored = _model(dev, hw, t), _model(dev, hw, t)
    torch.manual_seed(5)
    online.set_train_input(ref_img=ref_img, real_vid=real_vid, ref_text=cond)
    online.optimize_parameters()
    latent = stored.encode_video(real_vid, ref_img)

    def boom(*a, **k):
        raise AssertionError("the LFAE ran in a step from a stored latent")

    with monkeypatch.context() as mp:
        mp.setattr(FlowDiffusion, "_lfae_pass", boom)
        mp.setattr(stored.generator, "decode_video", boom)
        mp.setattr(stored.region_predictor, "forward", boom)
        mp.setattr(stored.bg_predictor, "forward", boom)
        torch.manual_seed(5)
        stored.set_train_latent(ref_img, latent, cond)
        stored.optimize_parameters()
    assert torch.equal(stored.loss, online.loss)
    for name in ("real_out_vid", "real_warped_vid", "fake_out_vid", "fake_warped_vid", "rec_loss", "rec_warp_loss"):
        assert getattr(stored, name) is None, name
    for name in ("real_vid_grid", "real_vid_conf", "fake_vid_grid", "fake_vid_conf"):
        assert getattr(stored, name) is not None, name
    stored.decode_step_logs(real_vid)
    assert float(stored.rec_loss) == float(online.rec_loss) and float(stored.rec_warp_loss) == float(online.rec_warp_loss)
    assert torch.equal(stored.fake_out_vid, online.fake_out_vid) and torch.equal(stored.fake_warped_vid, online.fake_warped_vid)
    assert_close(stored.real_out_vid, online.real_out_vid, 1e-3, "real_out_vid from the latent")
    assert_close(stored.real_warped_vid, online.real_warped_vid, 1e-3, "real_warped_vid from the latent")
    # the next online step of the same model is an online step again
    stored.set_train_input(ref_img=ref_img, real_vid=real_vid, ref_text=cond)
    stored.optimize_parameters()
    assert stored.rec_loss is not None and stored.fake_out_vid is not None and stored.train_latent is None


def test_set_train_latent_checks_and_the_functional_flavour(backend):
    from cvpr23_lfdm_amd import FlowDiffusionFunctional
    dev = backend
    m = _model(dev, 16, 2)
    with pytest.raises(RuntimeError, match="set_train_latent"):
        m.decode_step_logs(torch.zeros(1, 3, 2, 16, 16))
    with pytest.raises(ValueError, match="latent must be"):
        m.set_train_latent(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 3, 4, 4), ["a"])
    with pytest.raises(ValueError, match="batch"):
        m.set_train_latent(torch.zeros(2, 3, 16, 16), torch.zeros(1, 3, 2, 4, 4), ["a"])
    f = FlowDiffusionFunctional(img_size=4, num_frames=2, sampling_timesteps=5, is_train=True, config_pth=synth.CONFIG, dim_mults=MULTS)
    with pytest.raises(NotImplementedError):
        f.set_train_latent(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 2, 4, 4), ["a"])


# ---------------------------------------------------------------------------------------------
# two ranks over gloo on the emulator: a sharded latent step is the single-process step; an empty shard does not hang
# ---------------------------------------------------------------------------------------------
WORKER = r'''
import json, os, sys
repo = sys.argv[1]
sys.path.insert(0, repo); sys.path.insert(0, os.path.join(repo, "tests"))
import torch
import synth
import test_latent_store as T
from cvpr23_lfdm_amd import _build, _native
_native._set_library_for_tests(_native.NativeLibrary(_build.build_emu(), "emu"))
rank, HW, NF = int(os.environ.get("RANK", "0")), 16, 2
table = {"anger": torch.randn(768, generator=torch.Generator().manual_seed(1)), "fear": torch.randn(768, generator=torch.Generator().manual_seed(2))}
names = ["init_conv.bias", "mid_block1.block1.proj.weight", "final_conv.1.weight"]
out = {"rank": rank, "world": int(os.environ.get("WORLD_SIZE", "1")), "runs": []}
for batch in (2, 1):
    torch.manual_seed(11)
    m = T._model("cpu", HW, NF, null_cond_prob=0.5)
    m.diffusion.text_encoder = lambda texts: torch.stack([table[t] for t in texts])
    ref_img, real_vid, _, _, noise = synth.train_inputs(batch, NF, HW)
    torch.manual_seed(1234)
    m.set_train_latent(ref_img, (0.4 * noise).clamp(-1, 1), ["anger", "fear"][:batch])
    m.optimize_parameters()
    run = {"batch": batch, "loss": float(m.loss), "shard": int(m.ref_img.shape[0]), "mask": m.unet.null_cond_mask.tolist(),
           "none": [getattr(m, k) is None for k in ("real_out_vid", "fake_out_vid", "rec_loss", "rec_warp_loss")],
           "grid": list(m.fake_vid_grid.shape), "params": {k: m.unet.get(k).detach().double().flatten()[:2048].tolist() for k in names}}
    if batch == 1:
        m.decode_step_logs(real_vid)
        run["rec"], run["vid"] = float(m.rec_loss), list(m.fake_out_vid.shape)
    out["runs"].append(run)
open(os.path.join(os.environ["LFDM_DP_OUT"], "rank%d.json" % rank), "w").write(json.dumps(out))
import torch.distributed as dist
if dist.is_initialized():
    dist.barrier(); dist.destroy_process_group()
'''


def _launch(tmp_path, world):
    script = tmp_path / "latent_dp_worker.py"
    script.write_text(WORKER)
    outdir = tmp_path / ("out_w%d" % world)
    outdir.mkdir()
    env = dict(os.environ, LFDM_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", LFDM_DP_OUT=str(outdir), OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None), env.pop("RANK", None)
    cmd = [sys.executable, str(script), REPO] if world == 1 else \
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
         "--master-port", "29587", str(script), REPO]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    outs = [json.loads((outdir / f).read_text()) for f in sorted(os.listdir(outdir))]
    assert len(outs) == world, r.stdout[-2000:]
    return sorted(outs, key=lambda o: o["rank"])


def test_two_ranks_latent_step_emulator(tmp_path):
    """tests/test_dp_two_ranks.py's check for the step from a stored latent, at 16 pixels with a two-level denoiser: B = 2 split one
    video per rank, then B = 1, where rank 1 has no video, skips the model and still takes part in the collective."""
    from cvpr23_lfdm_amd import _build
    _build.build_emu()
    single = _launch(tmp_path, 1)[0]
    r0, r1 = _launch(tmp_path, 2)
    lr = 1e-4
    for i, (batch, shards) in enumerate(((2, (1, 1)), (1, (1, 0)))):
        s, a, b = single["runs"][i], r0["runs"][i], r1["runs"][i]
        assert s["batch"] == batch and s["shard"] == batch and (a["shard"], b["shard"]) == shards and r0["world"] == 2
        assert a["params"] == b["params"]                                     # the replicas stay bit-identical
        assert a["mask"] + b["mask"] == s["mask"]                             # the global draw, sliced
        assert a["none"] == b["none"] == s["none"] == [True] * 4
        assert a["grid"] == [shards[0], 2, 2, 4, 4] and b["grid"] == [shards[1], 2, 2, 4, 4]
        for k, v in s["params"].items():
            d = (torch.tensor(a["params"][k]) - torch.tensor(v)).abs()
            # Adam's first step is ~lr * sign(g): identical except where a gradient is numerically zero
            assert float(d.mean()) < 0.02 * lr and float((d > 0.5 * lr).float().mean()) < 0.01, (k, float(d.mean()), float(d.max()))
        weighted = (shards[0] * a["loss"] + shards[1] * b["loss"]) / batch
        assert abs(weighted - s["loss"]) <= 2e-4 * abs(s["loss"]), (weighted, s["loss"])
    s, a, b = single["runs"][1], r0["runs"][1], r1["runs"][1]
    assert b["loss"] == 0.0 and b["vid"] == [0, 3, 2, 16, 16] and b["rec"] == 0.0          # the empty rank's logs: zero videos
    assert a["vid"] == s["vid"] == [1, 3, 2, 16, 16] and abs(a["rec"] - s["rec"]) <= 1e-6


# ---------------------------------------------------------------------------------------------
# tools/train_dm.py --packed OUT --latents
# ---------------------------------------------------------------------------------------------
def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name + "_under_test", os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def emu_lib():
    from cvpr23_lfdm_amd import _build, _native
    _native._set_library_for_tests(_native.NativeLibrary(_build.build_emu(), "emu"))
    yield
    _native._set_library_for_tests(None)


def test_train_dm_from_a_latent_store(tmp_path, emu_lib, monkeypatch, capsys):
    """Two steps of the trainer from a packed store with --latents, the second one a --save-img-freq hit, on the emulator at 16 pixels.
    The store is packed by the LFAE the trainer builds (--synthetic: the random initialisation under --seed)."""
    from cvpr23_lfdm_amd import FlowDiffusion, video_store
    mod = _tool("train_dm")
    assert not mod.parse_args(["--packed", "DIR"]).latents and mod.parse_args(["--packed", "DIR", "--latents", "--resident"]).latents
    src, packed, out = str(tmp_path / "src"), str(tmp_path / "packed"), str(tmp_path / "out")
    _write_videos(src, 16)
    video_store.pack_frame_folders(src, packed, 16)
    torch.manual_seed(1234)
    np.random.seed(1234)
    packer = FlowDiffusion(is_train=False, img_size=4, num_frames=2, sampling_timesteps=1, config_pth=synth.CONFIG, dim_mults=MULTS)
    with monkeypatch.context() as mp:
        mp.setattr(FlowDiffusion, "_lfae_pass", _stand_in_pass)
        video_store.pack_latents(packer, packed, image_size=16)

    def boom(*a, **k):
        raise AssertionError("the trainer ran the LFAE with --latents")

    monkeypatch.setattr(FlowDiffusion, "_lfae_pass", boom)
    mod.main(["--packed", packed, "--latents", "--synthetic", "--size", "16", "--frames", "2", "--batch-size", "1", "--final-step", "2",
              "--save-img-freq", "2", "--print-freq", "1", "--save-freq", "100", "--num-workers", "0", "--dim-mults", "1", "2", "--out", out])
    log = capsys.readouterr().out
    lines = [l for l in log.splitlines() if l.startswith("iter ")]
    assert len(lines) == 2 and "loss_rec nan" in lines[0] and "loss_rec nan" not in lines[1], log
    files = sorted(os.listdir(out))
    assert any(f.startswith("B0001_S000002_") and f.endswith(".png") for f in files), files
    assert "flowdiff_0001_S000002.pth" in files
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "train_dm.py"), "--help"], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--latents" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "pack_latents.py"), "--help"], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--dtype" in r.stdout and "--lfae-ckpt" in r.stdout
