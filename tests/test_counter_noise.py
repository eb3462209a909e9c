"""Per-video seeds: counter-based sampling noise (noise="counter").  Seven groups: the raw Philox4x32-10 words; the normals
made from them; the update kernel's fused draw against the same noise written to memory (one step, and whole tiny videos against the
default path on a replayed tape); the same videos against the oracle; a video being a function of its seed wherever it sits in a batch;
one captured graph serving every seed; the refusals.

Philox and the Box-Muller transform are written out again here in numpy (uint64 arithmetic) from the contract, not imported from the
package.  Whole videos run on the GPU; under the emulator they are opt-in (LFDM_EMU_E2E=1) like every end-to-end test of the suite."""
import ctypes
import os

import numpy as np
import pytest
import torch

import layout
import lfdm_oracle as O
import synth
from util import assert_close, rnd

# ------------------------------------------------------------------------------------------ the contract, restated
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
XT, KNOWN, STEP = 0, 1, 2                # counter word `stream`
Z_MAX = 5.89                              # sqrt(50 ln 2): u >= 2^-25


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (or ints) holding 32-bit words, key: two ints -> four uint64 arrays of 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) for v in ctr]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]           # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & LO, (p0 >> S32) ^ c[3] ^ k1, p0 & LO]
        k0, k1 = (k0 + np.uint64(W0)) & LO, (k1 + np.uint64(W1)) & LO
    return c


def noise_bits(seed, n, step, stream, window):
    """(ceil(n / 4), 4) uint64: the words r0..r3 of every quad of one video's draw."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    full = lambda v: np.full_like(q, v)
    return np.stack(philox4x32_10([q, full(step), full(stream), full(window)], [seed & 0xFFFFFFFF, seed >> 32]), axis=1)


def normals(r, dt):
    """Box-Muller on the quads r (Q, 4) in the arithmetic of `dt` (np.float32 / np.float64) -> (4 Q,)."""
    u = lambda w: ((w >> np.uint64(8)).astype(dt) + dt(0.5)) * dt(2.0 ** -24)
    z = np.empty(r.shape, dt)
    for a in (0, 2):
        radius = np.sqrt(dt(-2.0) * np.log(u(r[:, a])))
        angle = dt(2.0 * np.pi) * u(r[:, a + 1])
        z[:, a], z[:, a + 1] = radius * np.cos(angle), radius * np.sin(angle)
    return z.reshape(-1)


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


SEEDS = [0, 1234, (1 << 32) + 5, (1 << 64) - 1]


# ------------------------------------------------------------------------------------------ 1. bits, exact
def test_philox_known_answers():
    """The published known answers of Philox4x32-10 (counter | key -> output) hold for the restatement every other test is measured with."""
    kat = [([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
           ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
           ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])]
    for ctr, key, want in kat:
        assert [int(v) for v in philox4x32_10(ctr, key)] == want


@pytest.mark.parametrize("n", [1, 3, 4, 735, 4096 + 2])
def test_philox_bits(backend, n):
    from cvpr23_lfdm_amd import ops
    dev = backend
    test_philox_known_answers()
    case = 0
    for step in (0, 1, 999):
        for stream in (XT, KNOWN, STEP):
            for window in (0, 3):
                seeds = [SEEDS[(case + j) % 4] for j in range(3)]          # all four seeds turn up in every row position
                case += 1
                out = torch.full((3, n), 0x55555555, dtype=torch.int32).to(dev)
                ops.philox_bits(out, seeds, stream=stream, step=step, window=window)
                for b, seed in enumerate(seeds):
                    want = noise_bits(seed, n, step, stream, window).reshape(-1)[:n].astype(np.uint32)
                    assert np.array_equal(as_u32(out[b]), want), (n, step, stream, window, seed)


# ------------------------------------------------------------------------------------------ 2. normals
N_STAT = 1 << 20
_stat = {}


def _stat_case(dev):
    """One draw of 2^20 normals (seed 1234, the step-noise stream) and its restatements, made once per backend and left unchanged."""
    if dev not in _stat:
        from cvpr23_lfdm_amd import ops
        out = torch.full((1, N_STAT), float("nan")).to(dev)
        ops.philox_normal(out, [1234], stream=STEP, step=17, window=2)
        r = noise_bits(1234, N_STAT, 17, STEP, 2)
        _stat[dev] = (out[0].cpu().numpy().astype(np.float64), normals(r, np.float64), normals(r, np.float32).astype(np.float64))
    return _stat[dev]


def test_philox_normal_accuracy(backend):
    """Against the float64 restatement on the same bits.  The bar: 4 x the largest deviation of a plain fp32 numpy restatement from the
    float64 one on these 2^20 values (hardware ln / sin / cos are about 1 ulp, not correctly rounded, and ln u near u = 1 amplifies)."""
    got, z64, z32 = _stat_case(backend)
    fp32_dev = float(np.abs(z32 - z64).max())
    err = float(np.abs(got - z64).max())
    print("philox_normal on %s: max |z - float64| %.3e; fp32 numpy restatement %.3e; bar %.3e" % (backend, err, fp32_dev, 4 * fp32_dev))
    assert np.isfinite(got).all()
    assert 1e-7 < fp32_dev < 1e-3                      # (the yardstick itself is sane)
    assert err <= 4 * fp32_dev, (err, fp32_dev)


def test_philox_normal_distribution(backend):
    """Five standard errors at n = 2^20, and the truncation |z| <= sqrt(50 ln 2)."""
    got, _, _ = _stat_case(backend)
    n = got.size
    mean, var = got.mean(), got.var()
    kurt = ((got - mean) ** 4).mean() / var ** 2
    print("philox_normal on %s: mean %.3e, var %.6f, kurtosis %.4f, max |z| %.4f" % (backend, mean, var, kurt, np.abs(got).max()))
    assert abs(mean) <= 5 / np.sqrt(n)
    assert abs(var - 1) <= 5 * np.sqrt(2 / n)
    assert abs(kurt - 3) <= 5 * np.sqrt(24 / n)
    assert np.abs(got).max() <= Z_MAX


@pytest.mark.parametrize("n,ld_extra,col_off", [(735, 0, 0), (735, 1, 0), (735, 5, 3), (4096 + 2, 3, 1), (3, 6, 2), (4096, 8, 4)])
def test_philox_normal_rows_depend_on_their_seed_alone(backend, n, ld_extra, col_off):
    """Row b of a batch of three equals the batch-of-one call with that seed, also inside a strided / offset window of a NaN-filled buffer
    (16-byte aligned rows, rows on every other alignment, ragged last quads), and nothing outside the rows is written."""
    from cvpr23_lfdm_amd import ops
    dev = backend
    seeds = [SEEDS[3], SEEDS[1], SEEDS[2]]
    alone = []
    for s in seeds:
        one = torch.full((1, n), float("nan")).to(dev)
        ops.philox_normal(one, [s], stream=XT, window=3)
        layout.no_nan(one, "batch of one")
        alone.append(one[0].cpu())
    assert not torch.equal(alone[0], alone[1]) or n < 2
    view, check = layout.window((3, n), ld_extra=ld_extra, col_off=col_off, device=dev)
    ops.philox_normal(view, seeds, stream=XT, window=3)
    check("philox_normal n=%d ld_extra=%d col_off=%d" % (n, ld_extra, col_off))
    for b in range(3):
        assert torch.equal(view[b].cpu(), alone[b]), (b, n, ld_extra, col_off)
    r = noise_bits(seeds[1], n, 0, XT, 3)
    assert np.abs(alone[1].numpy().astype(np.float64) - normals(r, np.float64)[:n]).max() <= 1e-4


def test_streams_windows_and_seeds_differ(backend):
    from cvpr23_lfdm_amd import ops
    dev = backend
    base = dict(stream=XT, step=0, window=0)
    draw = lambda seed, **kw: ops.philox_normal(torch.empty(1, 768).to(dev), [seed], **dict(base, **kw)).cpu()
    ref = draw(7)
    assert torch.equal(ref, draw(7))
    for other in (draw(8), draw(7 + (1 << 32)), draw(7, window=1), draw(7, stream=KNOWN), draw(7, stream=STEP), draw(7, stream=STEP, step=1)):
        assert not torch.equal(ref, other) and float((ref - other).abs().mean()) > 0.5


# ------------------------------------------------------------------------------------------ 3. the fused draw is the tape, bit for bit
@pytest.mark.parametrize("cthw", [(3, 5, 71), (3, 7, 57143)])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("known", [False, True])
def test_sampler_step_counter_is_the_loading_step(backend, known, batch, cthw):
    """Two steps in a row of ops.sampler_step with seeds (the noise computed in the update kernel) against the same two steps reading the
    tensor ops.philox_normal writes for (seeds, window, stream 2, step = the counter's value): x, x0_out and the step counter bit for bit.
    3 x 5 x 71 = 1065 elements: one workgroup, inside the 8 prefetched elements per thread, ragged; 3 x 7 x 57143 = 1 200 003 >
    8 x 512 x 256: the loop behind the prefetched elements runs.  batch = 3 keeps the clearing launch, batch = 1 folds it."""
    from cvpr23_lfdm_amd import ops
    dev = backend
    c, t, hw = cthw
    n = c * t * hw
    if n > 1 << 20 and dev != "cuda":
        pytest.skip("above 8 x 512 x 256 elements per sample: GPU only")
    shape = (batch, c, t, hw)
    table = torch.tensor([[9.] * 6, [2.0, 0.5, 0.9, 0.3, 0.0, 0.4], [0.5, 0.25, 0.7, 0.0, 0.2, 0.3], [9.] * 6]).to(dev)
    level = torch.tensor([[9., 9.], [9., 9.], [0.8125, 0.59], [0.9, 0.4]]).to(dev)
    seeds = [SEEDS[3], SEEDS[1], SEEDS[2]][:batch]
    window = 3
    x0, eps = rnd(*shape, seed=1), [rnd(*shape, seed=2), rnd(*shape, seed=3)]
    kf = {}
    if known:
        mask = torch.zeros(batch, t, dtype=torch.bool)
        mask[0, 0] = mask[0, t - 2] = True
        kf = dict(known=rnd(*shape, seed=5).to(dev), known_noise=rnd(*shape, seed=6).to(dev), frame_mask=mask.to(dev), level=level, frames=t)
    res = {}
    for fused in (True, False):
        x = x0.clone().to(dev)
        step = torch.tensor([1], dtype=torch.int32).to(dev)
        ws = ops.sampler_ws(batch, n, dev)
        outs = []
        for i in range(2):
            x0_out = torch.empty(shape).to(dev)
            if fused:
                ops.sampler_step(x, eps[i].to(dev), None, table, step, quantile=0.9, x0_out=x0_out, ws=ws,
                                 seeds=ops.seeds_tensor(seeds, dev), window=torch.tensor([window], dtype=torch.int32).to(dev), **kf)
            else:
                z = ops.philox_normal(torch.full(shape, float("nan")).to(dev), seeds, stream=STEP, step=1 + i, window=window)
                ops.sampler_step(x, eps[i].to(dev), z, table, step, quantile=0.9, x0_out=x0_out, ws=ws, **kf)
            outs.append((x.cpu().clone(), x0_out.cpu().clone(), int(step.cpu()[0])))
        res[fused] = outs
    for i in range(2):
        (xa, oa, sa), (xb, ob, sb) = res[True][i], res[False][i]
        what = "step %d, B=%d, n=%d, known=%s" % (i + 1, batch, n, known)
        assert sa == sb == i + 2, what
        assert torch.isfinite(xa).all() and torch.equal(oa, ob), what
        assert torch.equal(xa, xb), "%s: max |fused - loaded| %.3e" % (what, float((xa - xb).abs().max()))
    # the noise took part: the same steps without it differ
    x = x0.clone().to(dev)
    ops.sampler_step(x, eps[0].to(dev), None, table, torch.tensor([1], dtype=torch.int32).to(dev), quantile=0.9)
    assert float((x.cpu() - res[True][0][0]).abs().mean()) > 0.1


def _skip_slow_emu(dev):
    if dev == "cpu" and os.environ.get("LFDM_EMU_E2E", "0") != "1":
        pytest.skip("end-to-end under the emulator is opt-in (LFDM_EMU_E2E=1); it runs on the GPU")


T, S, HW = 4, 8, 32
CASES = {"ddim5": dict(steps=5, total=1000, known=False), "ddpm8": dict(steps=8, total=8, known=False),
         "ddim5_known": dict(steps=5, total=1000, known=True)}
VIDEO_SEEDS = [(1 << 63) + 11, 77, 5]


def _model(dev, case, noise, sampler="reference"):
    c = CASES[case]
    m, dsd, gsd = synth.build_flow_diffusion(dev, img_size=S, num_frames=T, sampling_timesteps=c["steps"], timesteps=c["total"], noise=noise,
                                             sampler=sampler)
    return m, dsd, gsd


def _known(batch):
    """The same two known frames for every video of the batch (NaN at the other frames)."""
    shape = (batch, 3, T, S, S)
    k = synth.NoiseTape(23)((1, 3, T, S, S)).clamp(-1, 1).expand(shape)
    mask = torch.zeros(batch, T, dtype=torch.bool)
    mask[:, :2] = True
    return torch.where(mask[:, None, :, None, None], k, torch.full(shape, float("nan"))).contiguous(), mask


def _inputs(batch):
    """One image and one condition for every video of the batch: the videos differ in their seeds alone."""
    img, cond = synth.inputs(1, HW)
    return img.expand(batch, -1, -1, -1).contiguous(), cond.expand(batch, -1).contiguous()


def _run(m, dev, case, seeds, tape=None):
    """One sample_one_video of len(seeds) videos: with the seeds (a noise="counter" model), or - `tape` given - on that tape."""
    batch = len(seeds)
    img, cond = _inputs(batch)
    kw = {}
    if CASES[case]["known"]:
        k, mask = _known(batch)
        kw = dict(known_latent=k.to(dev), known_mask=mask.to(dev))
    m.diffusion.noise_source = tape
    m.set_sample_input(sample_img=img.to(dev), sample_text=cond.to(dev))
    m.sample_one_video(cond_scale=1.0, **kw, **({} if tape is not None else dict(seeds=seeds)))
    return {k: getattr(m, k).cpu().clone() for k in ("sample_latent", "sample_vid_grid", "sample_vid_conf", "sample_warped_vid", "sample_out_vid")}


def _tape(m, case, seeds):
    c = CASES[case]
    return m.diffusion.counter_tape(seeds, (len(seeds), 3, T, S, S), c["steps"] < c["total"], known=c["known"])


@pytest.mark.parametrize("graph_steps", ["1", "10"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_counter_video_is_the_default_path_on_its_tape(backend, case, graph_steps, monkeypatch):
    """noise="counter" with seeds against noise="torch" replaying counter_tape(...): the finished latent and the decoded video, bit for bit,
    with one step per graph replay and with ten."""
    dev = backend
    _skip_slow_emu(dev)
    monkeypatch.setenv("LFDM_GRAPH_STEPS", graph_steps)
    seeds = VIDEO_SEEDS[:2]
    mc = _model(dev, case, "counter")[0]
    got = _run(mc, dev, case, seeds=seeds)
    mt = _model(dev, case, "torch")[0]
    want = _run(mt, dev, case, seeds, tape=_tape(mt, case, seeds))
    for k in got:
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], want[k]), "%s, %s: max diff %.3e" % (case, k, float((got[k] - want[k]).abs().max()))
    assert float((got["sample_latent"][0] - got["sample_latent"][1]).abs().mean()) > 1e-2       # two seeds, two videos


# ------------------------------------------------------------------------------------------ 4. against the oracle
_oracle = {}


def _oracle_video(dev, case, seed):
    """The oracle's video for one seed: its own loop on the counter tape (made on `dev` by the fill kernel, replayed on the host).  Computed
    once per (backend, case, seed) and left unchanged."""
    key = (dev, case, seed)
    if key not in _oracle:
        from test_known_frames import _decode, oracle_known_latent
        c = CASES[case]
        m, dsd, gsd = _model(dev, case, "torch")
        sd = dict(dsd)
        sd.update(O.make_schedule(c["total"]))
        img, cond = _inputs(1)
        fea = O.generator_compute_fea(gsd, img)
        tape = _tape(m, case, [seed])
        host_tape = lambda shape: tape(shape).cpu()
        shape = (1, 3, T, S, S)
        if c["known"]:
            k, mask = _known(1)
            lat = oracle_known_latent("ddim", sd, fea, cond, shape, c["steps"], c["total"], 1.0, host_tape, torch.nan_to_num(k), mask)
        else:
            lat = O.sample(sd, fea, cond, shape, c["steps"], c["total"], 1.0, 1.0, host_tape)
        ref = _decode(gsd, img, lat, T)
        ref["sample_latent"] = lat
        _oracle[key] = ref
    return _oracle[key]


@pytest.mark.parametrize("case", sorted(CASES))
def test_counter_video_against_the_oracle(backend, case):
    dev = backend
    _skip_slow_emu(dev)
    seed = VIDEO_SEEDS[1]
    ref = _oracle_video(dev, case, seed)
    got = _run(_model(dev, case, "counter")[0], dev, case, seeds=[seed])
    for k in got:
        assert_close(got[k], ref[k], 1e-3, "%s (%s, noise='counter')" % (k, case))


# ------------------------------------------------------------------------------------------ 5. a video is its seed
@pytest.mark.parametrize("sampler,ddim", [("reference", True), ("reference", False), ("dpmpp_2m", True)])
def test_every_draw_of_a_video_depends_on_its_seed_alone(backend, sampler, ddim):
    """counter_tape is what the sampler draws (group 3): x_T, the known-frame noise and every step-noise tensor of seed s are the same bits
    whether s is sampled alone, second of three, or with the other two seeds swapped - and differ between seeds and between windows.
    dpmpp_2m draws x_T (and the known-frame noise) and nothing else."""
    from cvpr23_lfdm_amd import GaussianDiffusion
    dev = backend
    total, steps = (1000, 5) if ddim else (8, 8)
    d = GaussianDiffusion(torch.nn.Identity(), image_size=S, num_frames=T, timesteps=total, sampling_timesteps=steps, loss_type="l2",
                          sampler=sampler, noise="counter")
    a, s, c = VIDEO_SEEDS
    n_draws = 2 + (0 if sampler != "reference" else (steps - 1 if ddim else steps))

    def all_draws(seeds, window=0):
        tape = d.counter_tape(seeds, (len(seeds), 3, T, S, S), ddim, window=window, known=True)
        out = [tape((len(seeds), 3, T, S, S)).cpu() for _ in range(n_draws)]
        with pytest.raises(IndexError):
            tape((len(seeds), 3, T, S, S))
        return out

    alone, three, swapped = all_draws([s]), all_draws([a, s, c]), all_draws([c, s, a])
    for i in range(n_draws):
        assert torch.equal(alone[i][0], three[i][1]) and torch.equal(alone[i][0], swapped[i][1]), i
        assert torch.equal(three[i][0], swapped[i][2]) and torch.equal(three[i][2], swapped[i][0]), i
        assert not torch.equal(three[i][0], three[i][1]) and not torch.equal(three[i][1], three[i][2]), i
        for j in range(i):
            assert not torch.equal(alone[i], alone[j]), (i, j)
    other_window = all_draws([s], window=1)
    for i in range(n_draws):
        assert not torch.equal(alone[i], other_window[i]), i


@pytest.mark.parametrize("case,sampler", [("ddim5", "reference"), ("ddim5_known", "reference"), ("ddim5", "dpmpp_2m")])
def test_a_video_is_its_seed(backend, case, sampler):
    """The finished tiny video of seed s - alone, second of three, and with the other two seeds swapped - agrees within 2e-3 (launch plans
    differ with the batch: bit equality is not promised); under the reference sampler each of them is held to 1e-3 of the oracle's video
    for s.  Another seed gives another video."""
    dev = backend
    _skip_slow_emu(dev)
    a, s, c = VIDEO_SEEDS
    alone = _run(_model(dev, case, "counter", sampler)[0], dev, case, seeds=[s])
    m3 = _model(dev, case, "counter", sampler)[0]
    three, swapped = _run(m3, dev, case, seeds=[a, s, c]), _run(m3, dev, case, seeds=[c, s, a])
    for k in alone:
        for name, other in (("second of three", three), ("seeds swapped", swapped)):
            assert_close(other[k][1:2], alone[k], 2e-3, "%s of seed s, %s (%s, %s)" % (k, name, case, sampler))
        assert_close(swapped[k][0:1], three[k][2:3], 2e-3, "%s of seed c at position 0 and 2" % k)
    if sampler == "reference":
        ref = _oracle_video(dev, case, s)
        for k in alone:
            assert_close(alone[k], ref[k], 1e-3, "%s alone against the oracle (%s)" % (k, case))
            assert_close(three[k][1:2], ref[k], 1e-3, "%s second of three against the oracle (%s)" % (k, case))
    assert float((three["sample_latent"][0] - three["sample_latent"][1]).abs().mean()) > 1e-2


# ------------------------------------------------------------------------------------------ 6. one graph, any seed (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ddim5", "ddim5_known"])
def test_one_graph_serves_every_seed(case):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvpr23_lfdm_amd import _native
    _native._set_library_for_tests(None)
    m = _model("cuda", case, "counter")[0]
    first = _run(m, "cuda", case, seeds=[3])
    plans = dict(m.diffusion._plans)
    assert len(plans) == 1
    plan = next(iter(plans.values()))
    graph, chunks = plan["graph"], dict(plan["chunk_graphs"])
    assert graph is not None and len(chunks) == 1                  # five steps, ten per replay: one chunk length, no draw flags
    second = _run(m, "cuda", case, seeds=[(1 << 64) - 2])
    third = _run(m, "cuda", case, seeds=[3])
    assert m.diffusion._plans == plans and plan["graph"] is graph
    assert list(plan["chunk_graphs"].items()) == list(chunks.items())
    assert torch.equal(first["sample_latent"], third["sample_latent"]) and not torch.equal(first["sample_latent"], second["sample_latent"])
    for seeds, got in (([3], first), ([(1 << 64) - 2], second)):
        fresh = _run(_model("cuda", case, "counter")[0], "cuda", case, seeds=seeds)
        for k in got:
            assert torch.equal(got[k], fresh[k]), (seeds, k)


@pytest.mark.gpu
def test_long_video_windows_take_their_own_counter_word():
    """sample_long_video(seed=): window w is a `sample` call with window=w on the same seed - the hand-written chain - and repeats."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cvpr23_lfdm_amd import _native
    _native._set_library_for_tests(None)
    nf, overlap, total = 8, 3, 13
    build = lambda: synth.build_flow_diffusion("cuda", img_size=8, num_frames=nf, sampling_timesteps=5, noise="counter")[0]
    m = build()
    img, cond = synth.inputs(1, HW)
    m.set_sample_input(sample_img=img.cuda(), sample_text=cond.cuda())
    m.sample_long_video(1.0, total, overlap=overlap, seed=41)
    got = m.sample_latent.clone()
    m.sample_long_video(1.0, total, overlap=overlap, seed=41)
    assert torch.equal(got, m.sample_latent)
    f = build()
    fea = f.generator.compute_fea_from_skips(f.generator.encode(img.cuda().float().contiguous()), 1, 8, 8)
    w0 = f.diffusion.sample(fea, cond=cond.cuda(), cond_scale=1.0, seeds=[41], window=0)
    known = torch.zeros_like(w0)
    known[:, :, :overlap] = w0[:, :, nf - overlap:]
    mask = torch.zeros(1, nf, dtype=torch.bool, device="cuda")
    mask[:, :overlap] = True
    w1 = f.diffusion.sample(fea, cond=cond.cuda(), cond_scale=1.0, known=known, known_mask=mask, seeds=[41], window=1)
    assert torch.equal(got, torch.cat((w0, w1[:, :, overlap:]), dim=2)[:, :, :total])
    w1_as_w0 = f.diffusion.sample(fea, cond=cond.cuda(), cond_scale=1.0, known=known, known_mask=mask, seeds=[41], window=0)
    assert not torch.equal(w1, w1_as_w0)


# ------------------------------------------------------------------------------------------ 7. refusals (host only: nothing is launched)
def _host_model(noise):
    from cvpr23_lfdm_amd import GaussianDiffusion
    d = GaussianDiffusion(torch.nn.Identity(), image_size=S, num_frames=T, timesteps=1000, sampling_timesteps=5, loss_type="l2", noise=noise)
    d.denoise_fn = torch.nn.Linear(1, 1)           # (a parameter to read the device from)
    return d


def test_refusals():
    from cvpr23_lfdm_amd import FlowDiffusion, GaussianDiffusion
    fea, cond = torch.zeros(2, 256, S, S), torch.zeros(2, 768)
    shape = (2, 3, T, S, S)
    d = _host_model("counter")
    calls = [lambda **kw: d.sample(fea, cond=cond, **kw), lambda **kw: d.ddim_sample(fea, shape, cond=cond, **kw),
             lambda **kw: d.p_sample_loop(fea, shape, cond=cond, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="needs seeds"):
            call()
        for bad in ([1], [1, 2, 3], 7):
            with pytest.raises(ValueError, match="seeds"):
                call(seeds=bad)
        for bad in ([1, -1], [1, 1 << 64], [1, 2.0], [1, True], [1, "2"]):
            with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
                call(seeds=bad)
        with pytest.raises(ValueError, match="window"):
            call(seeds=[1, 2], window=-1)
    d.noise_source = synth.NoiseTape(1)
    for call in calls:
        with pytest.raises(ValueError, match="noise_source"):
            call(seeds=[1, 2])
    t = _host_model("torch")
    for call in (lambda **kw: t.sample(fea, cond=cond, **kw), lambda **kw: t.ddim_sample(fea, shape, cond=cond, **kw)):
        with pytest.raises(ValueError, match="noise='counter'"):
            call(seeds=[1, 2])
    with pytest.raises(ValueError, match="noise must be"):
        GaussianDiffusion(torch.nn.Identity(), image_size=S, num_frames=T, noise="philox")
    with pytest.raises(ValueError, match="noise must be"):
        FlowDiffusion(img_size=S, num_frames=T, sampling_timesteps=5, is_train=False, config_pth=synth.CONFIG, noise="philox")
    m = FlowDiffusion(img_size=S, num_frames=T, sampling_timesteps=5, is_train=False, config_pth=synth.CONFIG, noise="counter")
    assert m.diffusion.noise == "counter"
    m.set_sample_input(sample_img=torch.zeros(1, 3, HW, HW), sample_text=torch.zeros(1, 768))
    with pytest.raises(ValueError, match="needs seeds"):
        m.sample_one_video(1.0)
    with pytest.raises(ValueError, match="seeds"):
        m.sample_one_video(1.0, seeds=[1, 2])
    with pytest.raises(ValueError, match="needs seeds"):
        m.sample_long_video(1.0, 6, overlap=2)
    with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
        m.sample_long_video(1.0, 6, overlap=2, seed=-3)


def test_ops_refuse_bad_arguments(backend):
    from cvpr23_lfdm_amd import _native, ops
    dev = backend
    out = torch.zeros(2, 64).to(dev)
    for kw in (dict(seeds=[1]), dict(seeds=[1, 2, 3]), dict(seeds=[1, 1 << 64]), dict(seeds=[1, 2], stream=3), dict(seeds=[1, 2], step=-1),
               dict(seeds=torch.zeros(2, dtype=torch.int32).to(dev)), dict(seeds=torch.zeros(3, dtype=torch.int64).to(dev))):
        with pytest.raises(ValueError):
            ops.philox_normal(out, **dict(dict(stream=0), **kw))
    with pytest.raises(ValueError):
        ops.philox_normal(out.t(), [1] * 64, stream=0)
    with pytest.raises(TypeError):
        ops.philox_bits(out, [1, 2], stream=0)
    x, eps = torch.zeros(2, 3, 4, 16).to(dev), torch.zeros(2, 3, 4, 16).to(dev)
    table, step = torch.zeros(1, 6).to(dev), torch.zeros(1, dtype=torch.int32).to(dev)
    seeds, window = ops.seeds_tensor([1, 2], dev), torch.zeros(1, dtype=torch.int32).to(dev)
    with pytest.raises(ValueError, match="go together"):
        ops.sampler_step(x, eps, None, table, step, quantile=-1.0, seeds=seeds)
    with pytest.raises(ValueError, match="go together"):
        ops.sampler_step(x, eps, None, table, step, quantile=-1.0, window=window)
    with pytest.raises(ValueError, match="exclude"):
        ops.sampler_step(x, eps, x.clone(), table, step, quantile=-1.0, seeds=seeds, window=window)
    with pytest.raises(ValueError, match="window"):
        ops.sampler_step(x, eps, None, table, step, quantile=-1.0, seeds=seeds, window=torch.zeros(1).to(dev))
    # the C entry points check for themselves
    lib = _native.library()
    assert lib.lfdm_philox_normal_f32(ops._p(out), ops._p(seeds), 2, 64, 63, 0, 0, 0, ops._stream(lib)) != 0 and b"row_stride" in lib.lfdm_last_error()
    assert lib.lfdm_philox_normal_f32(ops._p(out), ops._p(seeds), 2, 64, 64, 3, 0, 0, ops._stream(lib)) != 0
    assert lib.lfdm_philox_bits_u32(ops._p(out), None, 2, 64, 64, 0, 0, 0, ops._stream(lib)) != 0
    ws = ops.sampler_ws(2, 192, dev)
    args = dict(x=ops._p(x), eps=ops._p(eps), batch=2, n=192, coef=ops._p(table), step_dev=ops._p(step), quantile=-1.0, advance=1, ws=ops._p(ws),
                ws_bytes=ws.numel() * 4)
    c_step = lambda **kw: lib.lfdm_sampler_step_f32(ctypes.byref(_native.SamplerStepParams(**dict(args, **kw))), ops._stream(lib))
    assert c_step(window=ops._p(window)) != 0 and b"seeds" in lib.lfdm_last_error()
    assert c_step(seeds=ops._p(seeds)) != 0
    assert int(step.cpu()[0]) == 0 and not x.cpu().any()                # nothing ran


def test_demo_flags_parse():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "demo.py")
    spec = importlib.util.spec_from_file_location("lfdm_demo_tool_counter", path)
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    args = demo.build_parser().parse_args([])
    assert args.noise == "torch" and args.batch == 1 and demo.video_seeds(args) is None
    args = demo.build_parser().parse_args(["--noise", "counter", "--batch", "3", "--seed", "40"])
    assert demo.video_seeds(args) == [40, 41, 42]
    args = demo.build_parser().parse_args(["--noise", "counter", "--video-seeds", "7,8,0xffffffffffffffff", "--batch", "3"])
    assert demo.video_seeds(args) == [7, 8, (1 << 64) - 1]
    args = demo.build_parser().parse_args(["--noise", "counter", "--video-seeds", "7,8", "--batch", "3"])
    with pytest.raises(SystemExit):
        demo.video_seeds(args)
