"""uint8 preview strips rendered on the device: csrc/render.hip through ops.flow_to_color_u8 / ops.render_strip,
FlowDiffusion.render_sample / render_sample_host, io_compat.video_strip_device / mimsave_indexed.

The references are the host functions of io_compat that the demo has always used (sample_img, conf2fig, flow_to_color, _resize_hw), which
this feature leaves untouched; the dither formula is written out again here in numpy from DESIGN.md 4.5.  Kernel tests take the `backend`
fixture: the x86 emulator build everywhere, the gfx950 build on the GPU.

The flow-colour comparison (group 3) is the only one that is not byte-exact: the device and numpy both work in fp64 and can differ only where
a last-ulp difference of atan2 / sqrt straddles a floor - at most 1 level, in at most 0.1 % of the bytes (an fp32 restatement of the same
function differs in 1.44 % of the bytes of such inputs, so an fp32 kernel does not pass)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
from cvpr23_lfdm_amd import io_compat as IO

MEAN = (10.0, -7.5, 3.25)


def _dev(t, dev):
    return None if t is None else t.to(dev)


def _render(dev, **kw):
    from cvpr23_lfdm_amd import ops
    tens = {k: _dev(v, dev) for k, v in kw.items() if isinstance(v, torch.Tensor)}
    rest = {k: v for k, v in kw.items() if not isinstance(v, torch.Tensor)}
    out = ops.render_strip(**tens, **rest)
    assert out.dtype == torch.uint8 and out.is_contiguous()
    return out.cpu().numpy()


def _edge_values():
    """Every k / 255 in fp32 and its two neighbours, 0, 1, and values outside [0, 1]."""
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    vals = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)),
                           np.array([0.0, 1.0, -0.0, -0.25, -1e-8, 1.0 + 1e-6, 1.5, -3.0, 7.0], np.float32)])
    return vals.astype(np.float32)


def _video(shape, seed):
    """Model-range video around [0, 1] with values below 0 and above 1, the edge values sown in at fixed places of every channel."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = (rng.standard_normal(shape) * 0.45 + 0.5).astype(np.float32)
    flat = v.reshape(-1)
    e = _edge_values()
    pos = rng.choice(flat.size, size=min(flat.size // 2, 8 * e.size), replace=False)
    flat[pos] = np.resize(e, pos.size)
    return torch.from_numpy(v)


def _conf(shape, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    c = rng.random(shape, dtype=np.float32)
    flat = c.reshape(-1)
    e = _edge_values()
    e = e[(e >= 0) & (e <= 1)]
    pos = rng.choice(flat.size, size=min(flat.size // 2, e.size), replace=False)
    flat[pos] = np.resize(e, pos.size)
    return torch.from_numpy(c)


def _flow_grid(b, t, s, seed, noise=0.02):
    """(B, 2, T, s, s) sampling grid = identity + smooth flow + `noise` x N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(b * t, 2, 4, 4, generator=g) * 0.25
    smooth = F.interpolate(coarse, size=(s, s), mode="bilinear", align_corners=True)
    flow = smooth + noise * torch.randn(b * t, 2, s, s, generator=g)
    ident = IO.get_grid(1, (s, s), device="cpu")
    grid = (ident + flow).reshape(b, t, 2, s, s).permute(0, 2, 1, 3, 4).contiguous()
    return grid


def _host_flow_color(grid):
    """io_compat.flow_to_color(warped - identity) per frame, the operands as flow2fig's callers build them -> (B * T, s, s, 3)."""
    b, _, t, s, _ = grid.shape
    ident = IO.get_grid(1, (s, s), device="cpu")[0].permute(1, 2, 0).numpy()
    out = np.zeros((b * t, s, s, 3), np.uint8)
    for i in range(b):
        for f in range(t):
            warped = grid[i, :, f].permute(1, 2, 0).numpy()
            out[i * t + f] = IO.flow_to_color(np.asarray(warped) - np.asarray(ident))
    return out


def _check_images(dev, b, t, size, mean, seed=0):
    src, out, warped = _video((b, 3, size, size), seed + 1), _video((b, 3, t, size, size), seed + 2), _video((b, 3, t, size, size), seed + 3)
    got = _render(dev, source=src, out_vid=out, warped_vid=warped, mean=mean, panels=("source", "out", "warped"))
    assert got.shape == (b, t, size, 3 * size, 3)
    for i in range(b):
        want_src = IO.sample_img(src, i, mean)
        for f in range(t):
            assert np.array_equal(got[i, f, :, :size], want_src), ("source", i, f)
            assert np.array_equal(got[i, f, :, size:2 * size], IO.sample_img(out[:, :, f], i, mean)), ("out", i, f)
            assert np.array_equal(got[i, f, :, 2 * size:], IO.sample_img(warped[:, :, f], i, mean)), ("warped", i, f)


def _check_conf(dev, b, t, s, seed=0):
    conf = _conf((b, 1, t, s, s), seed + 4)
    got = _render(dev, conf=conf, panels=("conf",))
    assert got.shape == (b, t, 4 * s, 4 * s, 3)
    for i in range(b):
        for f in range(t):
            want = IO.conf2fig(conf[i, :, f], img_size=4 * s)
            for c in range(3):
                assert np.array_equal(got[i, f, :, :, c], want), (i, f, c)


def _check_flow_panel(dev, b, t, s, seed=0):
    from cvpr23_lfdm_amd import ops
    grid = _flow_grid(b, t, s, seed + 5)
    colour = ops.flow_to_color_u8(grid.to(dev))
    src = torch.zeros(b, 3, 4 * s, 4 * s)
    got = _render(dev, source=src, flow_color=colour, panels=("flow",))
    colour = colour.cpu().numpy()
    assert got.shape == (b, t, 4 * s, 4 * s, 3)
    for i in range(b * t):
        want = IO._resize_hw(colour[i], 4 * s, 4 * s, IO.INTER_LINEAR)
        assert np.array_equal(got[i // t, i % t], want), i
    return colour, grid


# ------------------------------------------------------------------------------------------ 1. image panels
@pytest.mark.parametrize("mean", [(0.0, 0.0, 0.0), MEAN])
@pytest.mark.parametrize("t", [1, 5, 40])
@pytest.mark.parametrize("b", [1, 3])
def test_image_panels_are_sample_img(backend, b, t, mean):
    _check_images(backend, b, t, 32 if t == 40 else 64, mean, seed=10 * b + t)


def test_edge_values_cover_what_they_claim():
    e = _edge_values()
    assert (e < 0).any() and (e > 1).any() and (e == 0).any() and (e == 1).any()
    k = (np.arange(256) / 255.0).astype(np.float32)
    assert np.isin(np.nextafter(k, np.float32(2)), e).all() and np.isin(np.nextafter(k, np.float32(-1)), e).all()
    # the neighbours matter: k / 255 * 255 lands on or just beside an integer, where truncation is decided by the last bit
    q = (e[(e >= 0) & (e <= 1)] * np.float32(255)).astype(np.float32)
    assert (np.abs(q - np.rint(q)) < 1e-4).sum() > 500


# ------------------------------------------------------------------------------------------ 2. conf panel
@pytest.mark.parametrize("s", [32, 64])
def test_conf_panel_is_conf2fig(backend, s):
    _check_conf(backend, 2, 3, s)


# ------------------------------------------------------------------------------------------ 3. flow colour at latent resolution
def _compare_colour(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    share = float((d != 0).mean())
    print("%s: %d of %d bytes differ (%.4f %%), max |diff| %d" % (what, int((d != 0).sum()), d.size, 100 * share, int(d.max())))
    assert int(d.max()) <= 1, what
    assert share <= 1e-3, (what, share)


def test_flow_colour_matches_flow_to_color(backend):
    """40 frames of 32 x 32 smooth flow + 0.02 noise (122 880 bytes): no byte off by more than 1, at most 0.1 % of them off at all.  Frame 7
    has zero flow (white everywhere); frame 11 holds one large outlier, which must scale that frame alone."""
    from cvpr23_lfdm_amd import ops
    grid = _flow_grid(1, 40, 32, seed=2024)
    ident = IO.get_grid(1, (32, 32), device="cpu")[0]
    grid[0, :, 7] = ident
    grid[0, 0, 11, 5, 9] += 5.0
    got = ops.flow_to_color_u8(grid.to(backend))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (40, 32, 32, 3) and got.is_contiguous()
    got = got.cpu().numpy()
    want = _host_flow_color(grid)
    _compare_colour(got, want, "flow colour 40 x 32 x 32 on %s" % backend)
    assert (got[7] == 255).all() and (want[7] == 255).all()
    # the outlier frame is nearly white away from the outlier; with a per-video maximum every other frame would be too
    print("mean byte of frames 10, 11, 12: %.1f %.1f %.1f" % (want[10].mean(), want[11].mean(), want[12].mean()))
    assert want[11].mean() > 240 and want[10].mean() < 230 and want[12].mean() < 230
    again = ops.flow_to_color_u8(grid.to(backend)).cpu().numpy()
    assert np.array_equal(got, again)


def test_flow_colour_shapes_and_strided_latent(backend):
    """Other latent sizes (64: four passes of 1024 pixels; 20: a last pass that is not full; T = 1), and the first two channels of a
    (B, 3, T, s, s) latent passed as the view FlowDiffusion keeps in sample_vid_grid.  No byte may be off by more than 1 in any case; the
    0.1 % cap on the share is applied to the cases pooled (117 888 bytes, the size it was stated for: one byte of the 576 of the smallest
    case alone is 0.17 %)."""
    from cvpr23_lfdm_amd import ops
    gots, wants = [], []
    for b, t, s in ((2, 3, 64), (3, 1, 8), (2, 5, 20), (1, 40, 16), (1, 2, 12)):
        grid = _flow_grid(b, t, s, seed=31 + s)
        want = _host_flow_color(grid)
        got = ops.flow_to_color_u8(grid.to(backend)).cpu().numpy()
        assert got.shape == want.shape == (b * t, s, s, 3)
        assert np.abs(got.astype(np.int16) - want.astype(np.int16)).max() <= 1, (b, t, s)
        gots.append(got.reshape(-1))
        wants.append(want.reshape(-1))
        latent = torch.cat((grid, torch.full((b, 1, t, s, s), float("nan"))), dim=1).to(backend)
        view = latent[:, :2]
        assert b == 1 or not view.is_contiguous()
        assert np.array_equal(ops.flow_to_color_u8(view).cpu().numpy(), got)
    _compare_colour(np.concatenate(gots), np.concatenate(wants), "flow colour, five shapes pooled, on %s" % backend)


# ------------------------------------------------------------------------------------------ 4. flow panel
@pytest.mark.parametrize("s", [32, 64])
def test_flow_panel_is_the_resized_colour_image(backend, s):
    _check_flow_panel(backend, 2, 3, s)


# ------------------------------------------------------------------------------------------ 5. whole strip
def _operands(b, t, s, seed):
    size = 4 * s
    return dict(source=_video((b, 3, size, size), seed), out_vid=_video((b, 3, t, size, size), seed + 1),
                warped_vid=_video((b, 3, t, size, size), seed + 2), conf=_conf((b, 1, t, s, s), seed + 3)), _flow_grid(b, t, s, seed + 4)


ALL = ("source", "out", "warped", "flow", "conf")


def test_strip_panels_land_in_their_columns(backend):
    from cvpr23_lfdm_amd import ops
    b, t, s = 2, 3, 8
    size = 4 * s
    opnd, grid = _operands(b, t, s, 50)
    opnd["flow_color"] = ops.flow_to_color_u8(grid.to(backend)).cpu()
    single = {p: _render(backend, panels=(p,), mean=MEAN, **opnd) for p in ALL}
    for p in ALL:
        assert single[p].shape == (b, t, size, size, 3)
    assert len({single[p].tobytes() for p in ALL}) == 5
    for panels in (ALL, ALL[::-1], ("conf", "out"), ("warped", "source", "flow"), ("out",), ("flow", "flow", "conf"),
                   ("source", "out", "warped", "conf")):
        got = _render(backend, panels=panels, mean=MEAN, **opnd)
        assert got.shape == (b, t, size, len(panels) * size, 3) and got.dtype == np.uint8
        for i, p in enumerate(panels):
            assert np.array_equal(got[:, :, :, i * size:(i + 1) * size], single[p]), (panels, p)
    # only the operands of the listed panels are needed
    got = _render(backend, panels=("conf", "out"), mean=MEAN, conf=opnd["conf"], out_vid=opnd["out_vid"])
    assert np.array_equal(got[:, :, :, :size], single["conf"]) and np.array_equal(got[:, :, :, size:], single["out"])


def test_strip_batch_elements_are_independent(backend):
    from cvpr23_lfdm_amd import ops
    b, t, s = 3, 2, 8
    opnd, grid = _operands(b, t, s, 60)
    whole = _render(backend, panels=ALL, mean=MEAN, flow_color=ops.flow_to_color_u8(grid.to(backend)).cpu(), **opnd)
    for indexed in (False, True):
        whole = _render(backend, panels=ALL, mean=MEAN, indexed=indexed, flow_color=ops.flow_to_color_u8(grid.to(backend)).cpu(), **opnd)
        for i in range(b):
            one = {k: v[i:i + 1].contiguous() for k, v in opnd.items()}
            one["flow_color"] = ops.flow_to_color_u8(grid[i:i + 1].to(backend)).cpu()
            assert np.array_equal(_render(backend, panels=ALL, mean=MEAN, indexed=indexed, **one)[0], whole[i]), (indexed, i)


# ------------------------------------------------------------------------------------------ 6. indexed mode
def _bayer8():
    m = np.array([[0, 2], [3, 1]])
    for _ in range(2):
        m = np.block([[4 * m, 4 * m + 2], [4 * m + 3, 4 * m + 1]])
    return m


def _indexed_reference(rgb):
    """level = (c * 320 + 255 * bayer[y & 7][x & 7] + 127) // 16320 per channel, index = 36 r + 6 g + b; x is the column of
    the strip.  rgb (..., H, W, 3) uint8 -> (..., H, W) uint8."""
    h, w = rgb.shape[-3], rgb.shape[-2]
    th = _bayer8()[np.arange(h)[:, None] & 7, np.arange(w)[None, :] & 7]
    lv = (rgb.astype(np.int64) * 320 + 255 * th[..., None] + 127) // 16320
    assert lv.max() <= 5
    return (36 * lv[..., 0] + 6 * lv[..., 1] + lv[..., 2]).astype(np.uint8)


def test_palette():
    pal = IO.STRIP_PALETTE
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    for r in range(6):
        for g in range(6):
            for b in range(6):
                assert tuple(pal[36 * r + 6 * g + b]) == (51 * r, 51 * g, 51 * b)
    assert (pal[216:] == 0).all()


def test_indexed_strip_is_the_documented_formula(backend, tmp_path):
    from cvpr23_lfdm_amd import ops
    b, t, s = 2, 3, 8
    opnd, grid = _operands(b, t, s, 70)
    opnd["flow_color"] = ops.flow_to_color_u8(grid.to(backend)).cpu()
    for panels in (ALL, ("out", "flow", "conf")):
        rgb = _render(backend, panels=panels, mean=MEAN, **opnd)
        idx = _render(backend, panels=panels, mean=MEAN, indexed=True, **opnd)
        assert idx.shape == rgb.shape[:-1] and idx.dtype == np.uint8
        assert np.array_equal(idx, _indexed_reference(rgb)), panels
    # a GIF of those indices decodes to palette[index], frame by frame
    from PIL import Image
    path = str(tmp_path / "strip.gif")
    frames = [idx[0, f] for f in range(t)]
    IO.mimsave_indexed(path, frames)
    with Image.open(path) as im:
        assert im.n_frames == t
        for f in range(t):
            im.seek(f)
            assert np.array_equal(np.asarray(im.convert("RGB")), IO.STRIP_PALETTE[frames[f]]), f


def test_dither_keeps_the_block_mean(backend):
    """A constant colour c per channel dithers to levels whose mean over an aligned 8 x 8 block is within 1.0 of c.  Derivation: with
    5 c / 255 = k + f (0 <= f < 1) the level is k + [b >= 64 (1 - f) - 127 / 255] over the 64 thresholds b = 0 .. 63, each met once per
    aligned block, so the count n of raised pixels satisfies -0.502 < n - 64 f <= 0.498 and the block mean 51 (k + n / 64) is within
    51 * 0.502 / 64 = 0.4 of c: the step of the mean is 51 / 64 = 0.797 < 1.0."""
    s, size = 4, 16
    colours = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (1, 1, 1), (254, 254, 254), (25, 26, 27), (200, 100, 50), (51, 102, 153),
               (77, 13, 240), (50, 52, 151)]
    t = len(colours)
    vid = torch.zeros(1, 3, t, size, size)
    for f, col in enumerate(colours):
        for c in range(3):
            vid[0, c, f] = float(np.float32(col[c] / 255.0))
    rgb = _render(backend, out_vid=vid, panels=("out", "out"))
    idx = _render(backend, out_vid=vid, panels=("out", "out"), indexed=True)
    for f, col in enumerate(colours):
        assert (rgb[0, f] == np.array(col, np.uint8)).all(), col
        dec = IO.STRIP_PALETTE[idx[0, f]].astype(np.float64)                       # (16, 32, 3)
        blocks = dec.reshape(size // 8, 8, 2 * size // 8, 8, 3).mean(axis=(1, 3))
        err = np.abs(blocks - np.array(col, np.float64))
        print("colour %s: block-mean error max %.3f" % (col, err.max()))
        assert err.max() <= 1.0, (col, err.max())
    # ... and for every grey value, from the formula alone
    th = _bayer8().reshape(-1)
    for c in range(256):
        lv = (c * 320 + 255 * th + 127) // 16320
        assert lv.max() <= 5 and abs(51.0 * lv.mean() - c) <= 1.0, c


# ------------------------------------------------------------------------------------------ 7. model level
def _sampled_model(dev, monkeypatch, total=0):
    """A model that holds a sample.  GPU (and the emulator with LFDM_EMU_E2E=1): the tiny synthetic model really samples.  Emulator
    otherwise: a whole sampling run takes minutes there, so the sample attributes are filled with tensors of the shapes, layouts and ranges
    sample_one_video / sample_long_video leave (sample_vid_grid a channel slice of the latent, conf in [0, 1])."""
    nf, s, hw = 8, 8, 32
    frames = total or nf
    img, cond = synth.inputs(1, hw, seed=5)
    if dev == "cuda" or os.environ.get("LFDM_EMU_E2E", "0") == "1":
        m = synth.build_flow_diffusion(dev, img_size=s, num_frames=nf, sampling_timesteps=4)[0]
        m.diffusion.noise_source = synth.NoiseTape(5)
        m.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))
        if total:
            m.sample_long_video(1.0, total, overlap=3)
        else:
            m.sample_one_video(cond_scale=1.0)
    else:
        from cvpr23_lfdm_amd import FlowDiffusion
        m = FlowDiffusion(img_size=s, num_frames=nf, sampling_timesteps=4, is_train=False, config_pth=synth.CONFIG)
        m.set_sample_input(sample_img=img, sample_text=cond)
        latent = torch.cat((_flow_grid(1, frames, s, 80), _conf((1, 1, frames, s, s), 81) * 2 - 1), dim=1).clamp(-1, 1).contiguous()
        m.sample_latent = latent
        m.sample_vid_grid = latent[:, :2]
        m.sample_vid_conf = (latent[:, 2].unsqueeze(dim=1) + 1) * 0.5
        m.sample_out_vid = _video((1, 3, frames, hw, hw), 82)
        m.sample_warped_vid = _video((1, 3, frames, hw, hw), 83)
    assert m.sample_out_vid.shape[2] == frames
    # video_strip's fourth panel is a matplotlib drawing that the device does not make and this test does not compare
    monkeypatch.setattr(IO, "grid2fig", lambda grid, grid_size=32, img_size=256: np.zeros((img_size, img_size, 3), np.uint8))
    return m, img.to(dev)


@pytest.mark.parametrize("total", [0, 13])
def test_video_strip_device_equals_video_strip(backend, monkeypatch, total):
    """After sample_one_video (total = 0) and after sample_long_video with total_frames = 13 > num_frames = 8."""
    m, ref = _sampled_model(backend, monkeypatch, total)
    frames = total or 8
    for mean in ((0.0, 0.0, 0.0), MEAN):
        want = IO.video_strip(m, ref, mean=mean, grid_size=8)
        got = IO.video_strip_device(m, ref, mean=mean)
        assert len(got) == len(want) == frames
        for f in range(frames):
            assert got[f].shape == want[f].shape == (32, 160, 3) and got[f].dtype == np.uint8
            for col in (0, 1, 2, 4):
                assert np.array_equal(got[f][:, 32 * col:32 * (col + 1)], want[f][:, 32 * col:32 * (col + 1)]), (f, col)
            flow = IO.flow2fig(m.sample_vid_grid[0, :, f].permute(1, 2, 0).cpu().numpy(),
                               IO.get_grid(1, (8, 8), device="cpu")[0].permute(1, 2, 0).numpy(), grid_size=8, img_size=32)
            assert np.abs(got[f][:, 96:128].astype(np.int16) - flow.astype(np.int16)).max() <= 1, f
    idx = IO.video_strip_device(m, ref, mean=MEAN, indexed=True)
    rgb = m.render_sample(mean=MEAN, source=ref).cpu().numpy()
    assert len(idx) == frames and idx[0].shape == (32, 160)
    assert np.array_equal(np.stack(idx), _indexed_reference(rgb[0]))


def test_render_sample_host_reuses_its_buffer(backend, monkeypatch):
    m, ref = _sampled_model(backend, monkeypatch)
    dev = m.render_sample()
    assert dev.dtype == torch.uint8 and tuple(dev.shape) == (1, 8, 32, 160, 3) and dev.is_contiguous() and dev.device.type == backend
    a = m.render_sample_host()
    first, addr = a.copy(), a.ctypes.data
    assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and np.array_equal(a, dev.cpu().numpy())
    b = m.render_sample_host(mean=MEAN)
    assert b.ctypes.data == addr and b.shape == a.shape and not np.array_equal(b, first)
    if backend == "cuda":
        assert m._render_host.is_pinned()
    c = m.render_sample_host(panels=("out", "conf"), indexed=True)
    assert c.shape == (1, 8, 32, 64) and np.array_equal(c, m.render_sample(panels=("out", "conf"), indexed=True).cpu().numpy())
    d = m.render_sample_host()
    assert np.array_equal(d, first)


def test_render_sample_before_sampling_raises():
    from cvpr23_lfdm_amd import FlowDiffusion
    m = FlowDiffusion(img_size=8, num_frames=8, sampling_timesteps=4, is_train=False, config_pth=synth.CONFIG)
    with pytest.raises(RuntimeError, match="nothing has been sampled"):
        m.render_sample()
    with pytest.raises(RuntimeError, match="nothing has been sampled"):
        m.render_sample_host(indexed=True)


# ------------------------------------------------------------------------------------------ 8. full size on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("b,size", [(1, 128), (4, 256)])
def test_full_size_panels(b, size):
    """C2 (1, 3, 40, 128, 128) and C5 (4, 3, 40, 256, 256), random tensors, no model: image panels, conf panel, flow panel."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvpr23_lfdm_amd import _native
    _native._set_library_for_tests(None)
    _check_images("cuda", b, 40, size, MEAN, seed=100 + b)
    _check_conf("cuda", b, 40, size // 4, seed=110 + b)
    colour, grid = _check_flow_panel("cuda", b, 40, size // 4, seed=120 + b)
    _compare_colour(colour, _host_flow_color(grid), "flow colour B=%d T=40 s=%d" % (b, size // 4))


# ------------------------------------------------------------------------------------------ 9. argument checks
def test_render_ops_refuse_bad_arguments(backend):
    from cvpr23_lfdm_amd import _native, ops
    import ctypes
    dev = backend
    b, t, s = 1, 2, 8
    opnd, grid = _operands(b, t, s, 90)
    opnd = {k: v.to(dev) for k, v in opnd.items()}
    grid = grid.to(dev)
    colour = ops.flow_to_color_u8(grid)
    with pytest.raises(ValueError, match="unknown panel"):
        ops.render_strip(panels=("out", "grid"), **opnd)
    with pytest.raises(ValueError, match="1 to 8 panels"):
        ops.render_strip(panels=(), **opnd)
    with pytest.raises(ValueError, match="needs its operand"):
        ops.render_strip(panels=("out", "flow"), **opnd)
    with pytest.raises(ValueError, match="shape"):
        ops.render_strip(panels=("out", "conf"), out_vid=opnd["out_vid"], conf=opnd["conf"][:, :, :, :4, :4].contiguous())
    with pytest.raises(ValueError, match="float32"):
        ops.render_strip(panels=("out",), out_vid=opnd["out_vid"].double())
    with pytest.raises(ValueError):
        ops.flow_to_color_u8(grid[:, :1])
    with pytest.raises(ValueError):
        ops.flow_to_color_u8(torch.zeros(1, 2, 2, 6, 6).to(dev))
    # the C entry points check for themselves: null operands, S != 4 s, an empty panel list
    lib = _native.library()
    st = ops._stream(lib)
    p = ops._p
    ident = ops._identity_table(s, grid.device)
    out = torch.empty(b, t, 4 * s, 5 * 4 * s, 3, dtype=torch.uint8, device=grid.device)
    assert lib.lfdm_flow_color_u8(None, 2 * t * s * s, p(ident), p(colour), b, t, s, st) != 0 and b"flow_color" in lib.lfdm_last_error()
    assert lib.lfdm_flow_color_u8(p(grid), 2 * t * s * s, None, p(colour), b, t, s, st) != 0
    assert lib.lfdm_flow_color_u8(p(grid), 2 * t * s * s, p(ident), None, b, t, s, st) != 0
    assert lib.lfdm_flow_color_u8(p(grid), 2 * t * s * s, p(ident), p(colour), b, 0, s, st) != 0
    assert lib.lfdm_flow_color_u8(p(grid), 2 * t * s * s, p(ident), p(colour), b, t, 6, st) != 0
    assert lib.lfdm_flow_color_u8(p(grid), t * s * s, p(ident), p(colour), b, t, s, st) != 0
    mean = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    codes = (ctypes.c_int * 5)(0, 1, 2, 3, 4)
    good = [p(opnd["source"]), p(opnd["out_vid"]), p(opnd["warped_vid"]), p(colour), p(opnd["conf"]), mean, codes, 5, 0, p(out), b, t, 4 * s, s, st]
    assert lib.lfdm_render_strip_u8(*good) == 0

    def bad(**kw):
        names = ["source", "out_vid", "warped_vid", "flow_color", "conf", "mean", "panels", "n_panels", "indexed", "out", "batch", "frames",
                 "S", "s", "stream"]
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return lib.lfdm_render_strip_u8(*args)

    for name in ("source", "out_vid", "warped_vid", "flow_color", "conf", "mean", "panels", "out"):
        assert bad(**{name: None}) != 0, name
    assert bad(n_panels=0) != 0 and b"panel list is empty" in lib.lfdm_last_error()
    assert bad(n_panels=9) != 0
    assert bad(S=4 * s + 16) != 0 and b"4 * s" in lib.lfdm_last_error()
    assert bad(S=2 * s) != 0 and b"4 * s" in lib.lfdm_last_error()
    assert bad(panels=(ctypes.c_int * 5)(0, 1, 2, 3, 5)) != 0
    assert bad(frames=0) != 0 and bad(batch=0) != 0
    assert bad(source=None, panels=(ctypes.c_int * 5)(1, 1, 2, 3, 4)) == 0          # an operand no listed panel reads may be null


def test_render_ops_refuse_cpu_tensors_on_the_product_library():
    from cvpr23_lfdm_amd import _native, ops
    _native._set_library_for_tests(None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.flow_to_color_u8(torch.zeros(1, 2, 1, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_strip(panels=("out",), out_vid=torch.zeros(1, 3, 1, 32, 32))


def test_demo_render_flags_parse():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "demo.py")
    spec = importlib.util.spec_from_file_location("lfdm_demo_tool_render", path)
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    args = demo.build_parser().parse_args([])
    assert args.render == "host" and args.gif == "rgb"
    args = demo.build_parser().parse_args(["--render", "device", "--gif", "indexed"])
    assert args.render == "device" and args.gif == "indexed"
    with pytest.raises(SystemExit):
        demo.check_args(demo.build_parser().parse_args(["--gif", "indexed"]))
