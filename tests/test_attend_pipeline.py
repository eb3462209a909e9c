"""The per-query-tile order of the attention core (csrc/attn_core.h attend_tiles: scores of tile ti+1, softmax of tile ti, P V of tile ti)
against float64, at every tile count and at the first and last padded row of a partly valid last tile.

Which order a launch takes is decided by its bias (attn_core.h bias_by_quads): the pipelined order reads the relative-position bias by
16-byte quads, so every frame count runs without bias, with an aligned bias (quads where frames % 4 == 0) and with the same bias one float
off alignment (element by element: the whole order).  Both orders must give the same numbers; tools/ab_bits.py --set attention compares
them bit for bit with the parent commit's.

Tolerance: tests/test_attention_fast_math.py's TOL (1e-4 of the output scale), the bar those entry points already meet; the references are
float64 (test_references_are_finite checks them without a GPU)."""
import functools
import math

import pytest
import torch

from cvpr23_lfdm_amd import ops
from test_attention_fast_math import TOL, attention_ref, layernorm_rows, temporal_tables
from util import assert_close, rnd

# 1 | one whole tile | first padded row of a second tile | three tiles, the last partly valid (40: the headline's frame count) | three and
# four whole tiles
FRAMES = [1, 16, 17, 33, 40, 48, 64]
BIAS = ["none", "aligned", "offset"]
HW = 4                     # sequences of the fused block (batch 1): eight waves per sequence by default, two forced beside it
CASES = [(f, bk, rot) for f in FRAMES for bk in BIAS for rot in (True, False)]


def _bias_arg(bias, kind, dev):
    """None | the table at the allocator's alignment | the same values starting one float into a buffer (not 16-byte addressable)."""
    if kind == "none":
        return None
    if kind == "aligned":
        t = bias.contiguous().to(dev)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.zeros(bias.numel() + 1, device=dev)
    buf[1:] = bias.reshape(-1).to(dev)
    t = buf[1:].view(bias.shape)
    assert t.data_ptr() % 16 == 4
    return t


def _kw(bias, cos, sin, kind, rot, dev):
    kw = dict(bias=_bias_arg(bias, kind, dev))
    if rot:
        kw.update(rot_cos=cos[:, 0::2].contiguous().to(dev), rot_sin=sin[:, 0::2].contiguous().to(dev))
    return kw


@functools.lru_cache(maxsize=None)
def _block_case(frames, kind, rot, flat_scores=False):
    """x (frames * HW, 64) in CL row order (t, pix), folded to_qkv, to_out, tables and the float64 block output.
    flat_scores: q = 0 and a constant bias - every score of a row is equal."""
    c = 64
    x = rnd(frames, HW, c, seed=1) * 2 + 0.5
    gamma = rnd(c, seed=2) * 0.3 + 1
    wq = rnd(768, c, seed=3, scale=1.0 / math.sqrt(c))
    wo = rnd(c, 256, seed=9, scale=1.0 / 16)
    bias, cos, sin = temporal_tables(frames)
    if flat_scores:
        wq[:256] = 0.0
        bias = torch.full_like(bias, 0.25)
    tokens = layernorm_rows(x.double(), gamma.double()).permute(1, 0, 2)                   # (pix, t, c)
    att = attention_ref(tokens @ wq.double().t(), None if kind == "none" else bias.double(), (cos.double(), sin.double()) if rot else None)
    ref = x.double().reshape(-1, c) + att.permute(1, 0, 2).reshape(-1, 256) @ wo.double().t()
    return x.reshape(-1, c), (wq * gamma.reshape(1, -1)).contiguous(), wo, (bias, cos, sin), ref


@functools.lru_cache(maxsize=None)
def _core_case(frames, kind, rot, special=None):
    """qkv (frames * 2, 768) in CL row order (t, pix) and the float64 attention.  special: 'dominant' - one key 141 above the others of its
    row; 'flat' - q = 0 and a constant bias."""
    hw = 2
    qkv = rnd(1, frames, hw, 768, seed=1)
    bias, cos, sin = temporal_tables(frames)
    if special == "dominant":
        qkv[..., :256] = 5.0                                          # q . k = 32 * 25 / sqrt(32) = 141 for the marked key, 0 for the others
        qkv[..., 256:512] = 0.0
        qkv[:, frames - 3, :, 256:512] = 5.0
    if special == "flat":
        qkv[..., :256] = 0.0
        bias = torch.full_like(bias, 0.25)
    ref = attention_ref(qkv.double().permute(0, 2, 1, 3), None if kind == "none" else bias.double(), (cos.double(), sin.double()) if rot else None)
    return qkv.reshape(-1, 768), (bias, cos, sin), ref.permute(0, 2, 1, 3).reshape(-1, 256)


def _run_block(dev, frames, kind, rot, monkeypatch, flat_scores=False):
    x, wf, wo, tables, ref = _block_case(frames, kind, rot, flat_scores)
    wqp, wop = ops.pack_tattn_weights(wf, wo)
    for nw in (None, "2"):                                            # the launcher's own split (eight waves here), the headline's two
        if nw is None:
            monkeypatch.delenv("LFDM_TATTN_OUT_NW", raising=False)
        else:
            monkeypatch.setenv("LFDM_TATTN_OUT_NW", nw)
        got = ops.temporal_attention_fused_out_cl(x.to(dev), wqp.to(dev), wop.to(dev), 1, frames, HW, **_kw(*tables, kind, rot, dev))
        assert bool(torch.isfinite(got).all())
        assert_close(got.cpu(), ref, TOL, "temporal attention block, %d frames, bias %s, rotary %s, %s waves" % (frames, kind, rot, nw))


def test_references_are_finite():
    for frames, kind, rot in CASES:
        assert bool(torch.isfinite(_block_case(frames, kind, rot)[-1]).all()), ("block", frames, kind, rot)
        assert bool(torch.isfinite(_core_case(frames, kind, rot)[-1]).all()), ("core", frames, kind, rot)
    assert bool(torch.isfinite(_block_case(40, "aligned", True, True)[-1]).all())
    for special in ("dominant", "flat"):
        assert bool(torch.isfinite(_core_case(40, "aligned", special == "flat", special)[-1]).all()), special


@pytest.mark.parametrize("frames,kind,rot", CASES)
def test_block_per_tile_order(backend, frames, kind, rot, monkeypatch):
    _run_block(backend, frames, kind, rot, monkeypatch)


@pytest.mark.parametrize("frames,kind,rot", CASES)
def test_core_per_tile_order(backend, frames, kind, rot):
    dev = backend
    qkv, tables, ref = _core_case(frames, kind, rot)
    out = ops.attention_cl(qkv.to(dev), 1, frames, 2, 0, **_kw(*tables, kind, rot, dev))
    assert bool(torch.isfinite(out).all())
    assert_close(out.cpu(), ref, TOL, "attention core, %d frames, bias %s, rotary %s" % (frames, kind, rot))


def test_core_one_dominant_key(backend):
    """Every other key's probability underflows: each query returns the marked key's value row; the padded keys of the last tile stay masked."""
    dev = backend
    qkv, tables, ref = _core_case(40, "aligned", False, "dominant")      # (no rotary: it would turn q . k into a function of the distance)
    want = qkv.view(40, 2, 768)[37:38, :, 512:].expand(40, 2, 256).reshape(-1, 256)
    assert float((ref - want.double()).abs().max()) < 1e-30
    out = ops.attention_cl(qkv.to(dev), 1, 40, 2, 0, **_kw(*tables, "aligned", False, dev))
    assert_close(out.cpu(), ref, TOL, "attention core, one dominant key")


def test_core_all_equal_scores(backend):
    """Every score of a row equal: the output is the mean of the 40 value rows, whatever the tile a key sits in."""
    dev = backend
    qkv, tables, ref = _core_case(40, "aligned", True, "flat")
    want = qkv.view(40, 2, 768)[:, :, 512:].double().mean(dim=0, keepdim=True).expand(40, 2, 256).reshape(-1, 256)
    assert float((ref - want).abs().max()) < 1e-12
    out = ops.attention_cl(qkv.to(dev), 1, 40, 2, 0, **_kw(*tables, "aligned", True, dev))
    assert_close(out.cpu(), ref, TOL, "attention core, all-equal scores")


def test_block_all_equal_scores(backend, monkeypatch):
    _run_block(backend, 40, "aligned", True, monkeypatch, flat_scores=True)
