"""The boundary kernels every sample and every decoded frame passes through (csrc/small.hip, csrc/conv_smalln.hip, the four glue kernels at the
bottom of csrc/norm.hip) at the launch-plan edges no per-kernel test reaches:
  conv_planar_in_cl  the matrix-pipe form's generic k-walk (K = 1, even K, K = 196 = CPI_MAX_K, kh != kw, 8 planes in `win`, tiles narrower than 32
    columns / shorter than 4 rows, a 7x1 filter over 3 channels that must not take the unrolled 7x7x3 walk) and the VALU form, which the shipped
    build selects only for cin > 8, a kernel edge above 7 or a filter that is not 16-byte aligned: float4 and scalar staging, float4 and scalar epilogue
  heads_cl_to_planar / heads_res_cl_to_planar  C = 4 ... 256, c0 + c1 = 512, c1 = 0 (x1 absent), c0 != c1, rows no multiple of 256
  heads_gn_res_cl_to_planar  2C = 512 (second trip of every prologue loop), 3 (c0 + c1) > 512 (the w_extra reads behind pe0 / pe1), 64 groups and one,
    2C = 128 away from (64, 64) on the generic path, 33 pixels on the register path, 128 rows per workgroup from 32 768 pixels on (both paths)
  linear_small  K below / at / above one wavefront, N no multiple of the four waves, every activation on either side, no bias
  sinusoidal  half = 2, 3, 65, 256 (second trip of the lane loop), t_stride 2, ldo > dim
  step_cond  exact; batch * n past the 1024-workgroup cap (the stride loop)
  conv2d_smalln_cl  cout 1, 2, 4 (the `j < cout` store guard), k = 1 and 5, three channel chunks, tiles ragged in both directions, one pixel
  affine_act_cl (every activation, ld 20 -> 16, past the 8192-workgroup cap), avgpool2_cl, planar_to_cl / cl_to_planar (ragged 32 x 32 tiles, exact)
  and what every launcher refuses, the 65 535 grid limits of linear_small and the two transposes among them (nothing is launched).
avgpool2_cl past ITS 8192-workgroup cap needs a 134 MB input and is left out.

References are float64 on the CPU from plain torch.  The bar is the family's own (test_ops_parity.py, test_norm_edges.py): 1e-4 of the output scale,
2e-5 absolute for sinusoidal (whose reference takes t * freq in fp32, as the kernel and the reference model form it - in float64 the product alone
differs by 2.5e-5 at dim 512), bit equality for step_cond and the transposes.  Inputs sit in NaN-padded rows (ld > C) and behind NaN planes where the
entry point takes a stride; destinations with a stride are NaN-filled, wider than the result, and their padding is still NaN afterwards.
Largest achieved fraction of the bar per entry point (LFDM_PARITY_LOG), MI355X / emulator - every case passes on both:
  conv_planar_in_cl 0.0032 / 0.0032 (VALU form, 3x7 x 9 channels x 192)   heads_cl_to_planar 0.0026 / 0.0035 (C = 256)
  heads_res_cl_to_planar 0.0041 / 0.0043 ((4, 508) / (256, 256))          heads_gn_res_cl_to_planar 0.0039 / 0.0034 (32 805 pixels)
  linear_small 0.0011 / 0.0011 (K = 63, GELU in, SiLU out)                sinusoidal 0.0030 / 0.0030 (6.0e-8 of 2e-5)
  conv2d_smalln_cl 0.0045 / 0.0045 (k = 5, cout = 4)                      avgpool2_cl 0.0010 / 0.0010
  affine_act_cl 0.0008 / 0.0008 (SiLU)                                    step_cond, planar_to_cl, cl_to_planar: bit equality
Runs on the emulator and on the GPU; every case is well under a second on the GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from cvpr23_lfdm_amd import ops
from util import assert_close, rnd, to_cl, unet_from_cl

TOL = 1e-4
NAN = float("nan")


def _wide(t, dev, pad=4):
    """rows (n, C) as the first C columns of a NaN-padded (n, C + pad) buffer on `dev`"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), NAN)
    buf[:, :t.shape[1]] = t
    return buf.to(dev)[:, :t.shape[1]]


def _offset(t, dev, off):
    """a dense tensor that starts `off` floats into a larger NaN-filled buffer on `dev` (off = 1: 4 bytes past a 16-byte boundary)"""
    buf = torch.full((t.numel() + off,), NAN)
    buf[off:] = t.reshape(-1)
    return buf.to(dev)[off:].view(t.shape)


def _dest(rows, c, dev, pad):
    buf = torch.full((rows, c + pad), NAN, device=dev)
    return buf, buf[:, :c]


def _padding_untouched(buf, c):
    return bool(buf[:, c:].isnan().all())


_ACT = {"none": (ops.ACT_NONE, lambda v: v), "relu": (ops.ACT_RELU, F.relu), "sigmoid": (ops.ACT_SIGMOID, torch.sigmoid),
        "silu": (ops.ACT_SILU, F.silu), "gelu": (ops.ACT_GELU, F.gelu)}


# ------------------------------------------------------------------------------------------ conv_planar_in_cl
def _stem_inputs(batch, cin, cin_total, frames, h, w, kh, kw, cout, act, add_term):
    seed = 1000 + 31 * cin + 7 * kh + 3 * kw + h + w
    x = rnd(batch, cin_total, frames, h, w, seed=seed)
    wt = rnd(cout, cin, 1, kh, kw, seed=seed + 1, scale=1.0 / math.sqrt(cin * kh * kw))
    bias = rnd(cout, seed=seed + 2)
    add = rnd(batch, cout, h, w, seed=seed + 3) if add_term else None
    ref = F.conv3d(x[:, :cin].double(), wt.double(), bias.double(), padding=(0, kh // 2, kw // 2))
    if add_term:
        ref = ref + add.double().unsqueeze(2)
    if act == "relu":
        ref = F.relu(ref)
    x = x.clone()
    x[:, cin:] = NAN                                            # planes the convolution must not read
    return x, wt, bias, add, ref


def _stem_run(dev, case, inputs, what, wgt_off=0, bias_off=0, pad=4):
    batch, cin, cin_total, frames, h, w, kh, kw, cout, act, add_term = case
    x, wt, bias, add, ref = inputs
    buf, out = _dest(batch * frames * h * w, cout, dev, pad)
    ops.conv_planar_in_cl(x.to(dev), batch, cin, cin_total, frames, h, w, _offset(ops.pack_planar_in_weight(wt), dev, wgt_off), kh, kw, cout,
                          bias=_offset(bias, dev, bias_off), add_term=to_cl(add).to(dev) if add_term else None, act=_ACT[act][0], out=out)
    assert_close(unet_from_cl(out.cpu(), batch, frames, h, w), ref, TOL, "conv_planar_in_cl %s %s" % (what, "-".join(str(v) for v in case)))
    assert _padding_untouched(buf, cout), what


_STEM_MFMA = [
    (1, 1, 1, 1, 1, 1, 1, 1, 64, "none", False),               # K = 1 (the upper k-slot starts on the zero row), one pixel
    (2, 4, 5, 2, 5, 33, 7, 7, 64, "relu", True),               # K = 196 exactly; second column tile one pixel wide; rows ragged
    (1, 8, 8, 1, 3, 31, 3, 3, 128, "none", True),              # 8 planes in `win`; two output slices
    (1, 2, 3, 3, 9, 7, 3, 5, 64, "none", False),               # kh != kw
    (1, 3, 3, 1, 4, 32, 7, 1, 64, "none", True),               # 7x1 x 3 channels: the generic walk, not the unrolled 7x7x3 one
    (1, 5, 5, 2, 7, 65, 1, 7, 64, "none", False),              # third column tile
]
_STEM_VALU = [
    (2, 12, 13, 1, 5, 9, 3, 3, 64, "relu", True),              # 90 pixels, below one 128-pixel block
    (1, 21, 21, 2, 3, 43, 3, 3, 128, "none", False),           # 258 pixels, third block ragged
    (1, 196, 196, 1, 2, 3, 1, 1, 64, "none", True),            # 196 channels, 1x1
    (1, 9, 9, 1, 11, 13, 3, 7, 192, "none", True),             # three output slices (ldo = 195: the scalar epilogue)
    (1, 1, 1, 1, 10, 5, 9, 3, 64, "relu", True),               # kernel edge above 7
    (2, 2, 2, 1, 3, 130, 1, 11, 64, "relu", True),             # kernel edge above 7
]
_ids = lambda c: "-".join(str(v) for v in c)


@pytest.mark.parametrize("case", _STEM_MFMA, ids=_ids)
def test_stem_conv_matrix_pipe_walk(backend, case):
    """conv_planar_in_mfma_kernel's generic k-walk (cin <= 8, edges <= 7, aligned filter)."""
    _stem_run(backend, case, _stem_inputs(*case), "mfma")


@pytest.mark.parametrize("case", _STEM_VALU, ids=_ids)
def test_stem_conv_valu_form(backend, case):
    """conv_planar_in_kernel as the launcher itself selects it (cin > 8 or a kernel edge above 7): float4 staging; float4 epilogue at ldo = cout + 4,
    the scalar one at ldo = cout + 3 (the 192-column case)."""
    _stem_run(backend, case, _stem_inputs(*case), "valu", pad=3 if case[8] == 192 else 4)


@pytest.mark.parametrize("case,which", [((1, 3, 3, 2, 5, 33, 7, 7, 64, "relu", True), "filter"), ((1, 3, 3, 1, 6, 9, 5, 5, 128, "relu", True), "bias")],
                         ids=["7x7x3-filter", "5x5x3-bias"])
def test_stem_conv_both_forms(backend, case, which):
    """The same shape through the aligned and the offset operand, both against float64.  A packed filter one float into its buffer is not 16-byte
    aligned: the launcher leaves the matrix-pipe form and conv_planar_in_kernel stages it by scalars.  A bias one float in: the scalar epilogue of
    whichever form runs; with both offsets, scalar staging and scalar epilogue of the VALU form."""
    inputs = _stem_inputs(*case)
    _stem_run(backend, case, inputs, "aligned")
    _stem_run(backend, case, inputs, "offset " + which, wgt_off=int(which == "filter"), bias_off=int(which == "bias"))
    _stem_run(backend, case, inputs, "offset filter and bias", wgt_off=1, bias_off=1)


# ------------------------------------------------------------------------------------------ heads
def _heads_ref(yf, yo, wf, bf, wo, bo, xe, we, batch, frames, hw):
    """the three dot products per pixel row in float64 -> planar (B, 3, T, HW)"""
    yf, yo, wf, wo = yf.double(), yo.double(), wf.double(), wo.double()
    cols = [yf @ wf[0] + bf[0].double(), yf @ wf[1] + bf[1].double(), yo @ wo[0] + bo[0].double()]
    if xe is not None:
        cols = [c + xe.double() @ we[i].double() for i, c in enumerate(cols)]
    return torch.stack(cols, dim=1).view(batch, frames, hw, 3).permute(0, 3, 1, 2)


@pytest.mark.parametrize("batch,frames,hw,ch,c0,c1", [(1, 1, 1, 4, 4, 0), (2, 3, 43, 256, 256, 256), (1, 2, 257, 128, 512, 0), (3, 1, 85, 12, 4, 508)])
def test_heads_widths_and_rows(backend, batch, frames, hw, ch, c0, c1):
    """heads_kernel<false> and <true>: C = 256 fills wl, c0 + c1 = 512 fills we, x1 absent, c0 != c1, 1 / 255 / 258 / 514 rows over blocks of 256."""
    dev = backend
    rows = batch * frames * hw
    y = rnd(rows, 2 * ch, seed=ch + 1)
    x0, x1 = rnd(rows, c0, seed=ch + 2), (rnd(rows, c1, seed=ch + 3) if c1 else None)
    wf, bf, wo, bo = rnd(2, ch, seed=7, scale=0.2), rnd(2, seed=8), rnd(1, ch, seed=9, scale=0.2), rnd(1, seed=10)
    we = rnd(3, c0 + c1, seed=11, scale=0.1)
    yd = _wide(y, dev)                                          # y_flow | y_occ: column slices of one NaN-padded row
    args = (yd[:, :ch], yd[:, ch:], wf.to(dev), bf.to(dev), wo.to(dev), bo.to(dev))
    out = ops.heads_cl_to_planar(*args, batch, frames, hw)
    assert_close(out.cpu(), _heads_ref(y[:, :ch], y[:, ch:], wf, bf, wo, bo, None, None, batch, frames, hw), TOL,
                 "heads_cl_to_planar C=%d rows=%d" % (ch, rows))
    xe = x0 if x1 is None else torch.cat((x0, x1), dim=1)
    out = ops.heads_res_cl_to_planar(*args, _wide(x0, dev), None if x1 is None else _wide(x1, dev, 8), we.to(dev), batch, frames, hw)
    assert_close(out.cpu(), _heads_ref(y[:, :ch], y[:, ch:], wf, bf, wo, bo, xe, we, batch, frames, hw), TOL,
                 "heads_res_cl_to_planar C=%d c0=%d c1=%d rows=%d" % (ch, c0, c1, rows))


@pytest.mark.parametrize("batch,frames,hw,ch,c0,c1,groups,nchunk", [
    (1, 1, 5, 256, 256, 256, 64, 5),                            # 2C = 512, 64 groups
    (2, 3, 11, 64, 128, 0, 16, 3),                              # 2C = 128 on the generic path
    (1, 1, 33, 64, 64, 64, 1, 1),                               # register path, 33 pixels, one group
    (2, 1, 7, 4, 4, 0, 2, 7),
    (1, 2, 20, 128, 508, 4, 32, 4),                             # 3 (c0 + c1) = 1536: w_extra read in place behind pe0 / pe1
    (1, 1, 32767, 4, 4, 0, 2, 7),                               # just below the 128-rows switch
    (1, 1, 32805, 4, 4, 0, 2, 5),                               # 128 rows per workgroup, ragged tail
    (1, 1, 32805, 64, 64, 64, 16, 5),                           # ... on the register path, whose row loop is its own (17 MB)
])
def test_heads_groupnorm_widths_and_rows(backend, batch, frames, hw, ch, c0, c1, groups, nchunk):
    """heads_gn_kernel; inputs, partials and reference as test_norm_edges.py::test_heads_groupnorm_generic_width builds them."""
    dev = backend
    b, pixels = batch, frames * hw
    y = rnd(b * pixels, 2 * ch, seed=1) * 1.7 + 0.4
    x0, x1 = rnd(b * pixels, c0, seed=2), (rnd(b * pixels, c1, seed=3) if c1 else None)
    gamma, beta = rnd(2 * ch, seed=4) * 0.3 + 1, rnd(2 * ch, seed=5) * 0.3
    wf, bf, wo, bo = rnd(2, ch, seed=7, scale=0.2), rnd(2, seed=8), rnd(1, ch, seed=9, scale=0.2), rnd(1, seed=10)
    we = rnd(3, c0 + c1, seed=11, scale=0.1)
    ys = y.view(b, pixels, 2 * ch)
    yn = F.silu(F.group_norm(ys.double().permute(0, 2, 1), groups, gamma.double(), beta.double(), eps=1e-5).permute(0, 2, 1)).reshape(b * pixels, 2 * ch)
    xe = x0 if x1 is None else torch.cat((x0, x1), dim=1)
    ref = _heads_ref(yn[:, :ch], yn[:, ch:], wf, bf, wo, bo, xe, we, b, frames, hw)
    assert pixels % nchunk == 0
    yg = ys.view(b, nchunk, pixels // nchunk, groups, 2 * ch // groups)
    partial = torch.stack([yg.sum(dim=(2, 4)), (yg * yg).sum(dim=(2, 4))], dim=-1).contiguous().view(b * nchunk, 2 * groups)
    out = ops.heads_gn_res_cl_to_planar(_wide(y, dev), partial.to(dev), nchunk, gamma.to(dev), beta.to(dev), wf.to(dev), bf.to(dev), wo.to(dev), bo.to(dev),
                                        _wide(x0, dev), None if x1 is None else _wide(x1, dev, 8), we.to(dev), b, frames, hw, groups=groups)
    assert_close(out.cpu(), ref, TOL, "heads_gn_res_cl_to_planar 2C=%d c0=%d c1=%d groups=%d pixels=%d" % (2 * ch, c0, c1, groups, pixels))


# ------------------------------------------------------------------------------------------ conditioning path
@pytest.mark.parametrize("batch,k,n,act_in,act_out,bias", [(1, 1, 1, "none", "none", False), (2, 63, 5, "gelu", "silu", True), (3, 65, 4, "silu", "gelu", True),
                                                           (1, 129, 7, "none", "relu", False), (2, 64, 1, "relu", "sigmoid", True)])
def test_linear_small_lanes_and_waves(backend, batch, k, n, act_in, act_out, bias):
    """one wavefront per output feature: K = 1 (one live lane), 63, 64, 65, 129 (third trip of the lane loop, one lane); N = 1, 5, 7 leave waves of the
    last workgroup without a column; rows of x, w and y in NaN-padded buffers."""
    dev = backend
    x, w = rnd(batch, k, seed=k), rnd(n, k, seed=k + 1, scale=1.0 / math.sqrt(k))
    bv = rnd(n, seed=k + 2) if bias else None
    ref = _ACT[act_out][1](F.linear(_ACT[act_in][1](x.double()), w.double(), bv.double() if bias else None))
    buf, out = _dest(batch, n, dev, 3)
    ops.linear_small(_wide(x, dev, 1), _wide(w, dev, 2), bv.to(dev) if bias else None, act_in=_ACT[act_in][0], act_out=_ACT[act_out][0], out=out)
    assert_close(out.cpu(), ref, TOL, "linear_small k=%d n=%d %s->%s" % (k, n, act_in, act_out))
    assert _padding_untouched(buf, n)


def _sinusoidal_ref(t, dim):
    """sin | cos in float64 of the fp32 product t * freq (the argument the kernel and the reference model form)"""
    arg = (t.float()[:, None] * ops.sinusoidal_freqs(dim, "cpu")[None, :]).double()
    return torch.cat((arg.sin(), arg.cos()), dim=-1)


@pytest.mark.parametrize("dim", [4, 6, 130, 512])
def test_sinusoidal_widths(backend, dim):
    """half = 2, 3 (the smallest the frequency table's half - 1 admits), 65 and 256: the second and fourth trip of the 64-lane loop."""
    dev = backend
    t = torch.tensor([0, 1, 999, 37], dtype=torch.int32)
    out = ops.sinusoidal(t.to(dev), ops.sinusoidal_freqs(dim, dev), 4, dim)
    assert_close(out.cpu(), _sinusoidal_ref(t, dim), 2e-5, "sinusoidal dim=%d" % dim)


def test_sinusoidal_strided_timesteps_and_wide_rows(backend):
    """t_stride = 2 reads every other timestep; ldo = dim + 3 leaves the columns behind a row alone."""
    dev = backend
    t = torch.tensor([5, 77, 9, 123, 0, 0], dtype=torch.int32)
    out = ops.sinusoidal(t.to(dev), ops.sinusoidal_freqs(64, dev), 3, 64, t_stride=2)
    assert_close(out.cpu(), _sinusoidal_ref(t[::2], 64), 2e-5, "sinusoidal t_stride=2")
    buf, out = _dest(4, 130, dev, 3)
    t = torch.tensor([0, 1, 999, 37], dtype=torch.int32)
    ops.sinusoidal(t.to(dev), ops.sinusoidal_freqs(130, dev), 4, 130, out=out)
    assert_close(out.cpu(), _sinusoidal_ref(t, 130), 2e-5, "sinusoidal ldo=133")
    assert _padding_untouched(buf, 130)


@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("table_rows,batch,n", [(3, 1, 1), (5, 3, 257), (2, 2, 140000)])
def test_step_cond_exact(backend, table_rows, batch, n, which):
    """out[b] = table[*step] + base[b], one fp32 add: the bits of torch's.  2 x 140 000 elements are more than 1024 workgroups of 256 cover in one trip."""
    dev = backend
    tab, base = rnd(table_rows, n, seed=n), rnd(batch, n, seed=n + 1)
    s = 0 if which == "first" else table_rows - 1
    out = torch.full((batch, n), NAN, device=dev)
    ops.step_cond(tab.to(dev), base.to(dev), torch.tensor([s], dtype=torch.int32, device=dev), out)
    assert torch.equal(out.cpu(), tab[s][None] + base)


# ------------------------------------------------------------------------------------------ conv2d_smalln_cl
@pytest.mark.parametrize("cin,k,h,w,cout,n", [(16, 1, 1, 1, 1, 1), (16, 5, 17, 15, 4, 2), (48, 3, 16, 32, 2, 3), (32, 7, 3, 50, 3, 1)])
def test_conv2d_smalln_filters_and_tiles(backend, cin, k, h, w, cout, n):
    """cout 1, 2, 4 and 3 behind the `j < cout` guard (columns cout .. 3 of the destination stay NaN), k = 1 / 5, three 16-channel chunks, a 17 x 15
    image (tiles ragged in both directions), images smaller than one 16 x 16 tile."""
    dev = backend
    x = rnd(n, cin, h, w, seed=cin + k)
    wt, bias = rnd(cout, cin, k, k, seed=2, scale=1.0 / math.sqrt(cin * k * k)), rnd(cout, seed=3)
    ref = torch.sigmoid(F.conv2d(x.double(), wt.double(), bias.double(), padding=k // 2))
    wp, bp = ops.pack_smalln_weight(wt, bias)
    buf = torch.full((n * h * w, 4), NAN, device=dev)
    ops.conv2d_smalln_cl(_wide(to_cl(x), dev), wp.to(dev), bp.to(dev), cout, k, n, h, w, act=ops.ACT_SIGMOID, out=buf)
    got = buf.cpu()
    assert_close(got[:, :cout].reshape(n, h, w, cout).permute(0, 3, 1, 2), ref, TOL, "conv2d_smalln_cl cin=%d k=%d cout=%d %dx%d" % (cin, k, cout, h, w))
    assert bool(got[:, cout:].isnan().all())


# ------------------------------------------------------------------------------------------ glue kernels of csrc/norm.hip
@pytest.mark.parametrize("n,c,h,w", [(1, 4, 2, 2), (3, 12, 2, 6), (2, 36, 6, 2)])
def test_avgpool2_ragged(backend, n, c, h, w):
    """one output pixel of one float4; one output row; one output column, nine float4 per pixel"""
    dev = backend
    x = rnd(n, c, h, w, seed=c)
    out = ops.avgpool2_cl(to_cl(x).to(dev), n, h, w)
    assert_close(out.cpu().reshape(n, h // 2, w // 2, c).permute(0, 3, 1, 2), F.avg_pool2d(x.double(), 2), TOL, "avgpool2_cl %dx%dx%dx%d" % (n, c, h, w))


@pytest.mark.parametrize("n,c,hw", [(1, 1, 1), (3, 33, 31), (2, 31, 65)])
def test_transposes_ragged_exact(backend, n, c, hw):
    """planar -> rows of ld = c + 3 -> planar: one element; 33 channels x 31 pixels (second channel tile one wide); 31 x 65 (third pixel tile one wide)."""
    dev = backend
    y = rnd(n, c, hw, seed=c + hw)
    buf, cl = _dest(n * hw, c, dev, 3)
    ops.planar_to_cl(y.to(dev), n, c, hw, out=cl)
    assert torch.equal(cl.cpu(), y.permute(0, 2, 1).reshape(n * hw, c))
    assert _padding_untouched(buf, c)
    back = ops.cl_to_planar(cl, n, c, hw, out=torch.full((n, c, hw), NAN, device=dev))
    assert torch.equal(back.cpu(), y)


@pytest.mark.parametrize("act", ["none", "relu", "sigmoid", "silu"])
def test_affine_act_strided_rows(backend, act):
    """5 rows of 12 channels read at ld 20, written at ld 16, with every activation of apply_act"""
    dev = backend
    x, a, b = rnd(5, 12, seed=1) * 2, rnd(12, seed=2), rnd(12, seed=3)
    buf, out = _dest(5, 12, dev, 4)
    ops.affine_act_cl(_wide(x, dev, 8), a.to(dev), b.to(dev), _ACT[act][0], out=out)
    assert_close(out.cpu(), _ACT[act][1](x.double() * a.double() + b.double()), TOL, "affine_act_cl ld 20->16 %s" % act)
    assert _padding_untouched(buf, 12)


def test_affine_act_past_block_cap(backend):
    """2 097 153 rows of one float4: one more than 8192 workgroups of 256 threads cover in one trip - the last row belongs to the second trip of thread 0"""
    dev = backend
    rows = 8192 * 256 + 1
    x, a, b = rnd(rows, 4, seed=4), rnd(4, seed=5), rnd(4, seed=6)
    out = ops.affine_act_cl(x.to(dev), a.to(dev), b.to(dev), ops.ACT_RELU, out=torch.full((rows, 4), NAN, device=dev)).cpu()
    ref = F.relu(x.double() * a.double() + b.double())
    assert_close(out[-1:], ref[-1:], TOL, "affine_act_cl past the cap, last row")
    assert_close(out, ref, TOL, "affine_act_cl past the cap")


# ------------------------------------------------------------------------------------------ refusals: the launcher returns before any launch
def _z(dev, *shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=dev)


def test_refusals(backend):
    dev = backend
    z = lambda *shape: _z(dev, *shape)
    stem = lambda cin, cin_total, kh, kw, cout: ops.conv_planar_in_cl(z(1, cin_total, 1, 4, 4), 1, cin, cin_total, 1, 4, 4, z(kh * kw * cin, cout), kh, kw, cout)

    def heads_res(ch, c0, c1):
        return ops.heads_res_cl_to_planar(z(2, ch), z(2, ch), z(2, ch), z(2), z(1, ch), z(1), z(2, c0), z(2, c1), z(3, c0 + c1), 1, 1, 2)

    def heads_gn(ch, groups):
        return ops.heads_gn_res_cl_to_planar(z(2, 2 * ch), z(1, 2 * groups), 1, z(2 * ch), z(2 * ch), z(2, ch), z(2), z(1, ch), z(1), z(2, 4), None, z(3, 4),
                                             1, 1, 2, groups=groups)

    smalln = lambda cin, k, cout: ops.conv2d_smalln_cl(z(4, cin), z(k * k, cin, 4), z(4), cout, k, 1, 2, 2, out=z(4, max(cout, 4)))
    cases = [
        ("conv_planar_in: unsupported shape", lambda: stem(3, 3, 4, 3, 64)),                  # an even kernel edge
        ("conv_planar_in: unsupported shape", lambda: stem(3, 3, 3, 4, 64)),
        ("conv_planar_in: unsupported shape", lambda: stem(5, 5, 7, 7, 64)),                  # K = 245 > 196
        ("conv_planar_in: unsupported shape", lambda: stem(3, 3, 3, 3, 32)),                  # cout % 64
        ("conv_planar_in: unsupported shape", lambda: stem(4, 3, 3, 3, 64)),                  # cin > cin_total
        ("heads: bad arguments", lambda: ops.heads_cl_to_planar(z(2, 260), z(2, 260), z(2, 260), z(2), z(1, 260), z(1), 1, 1, 2)),
        ("heads_res: bad arguments", lambda: heads_res(260, 4, 4)),
        ("heads_res: bad arguments", lambda: heads_res(4, 512, 4)),                           # c0 + c1 = 516
        ("heads_gn_res: bad arguments", lambda: heads_gn(260, 8)),                            # 2C = 520
        ("heads_gn_res: bad arguments", lambda: heads_gn(4, 3)),                              # 8 channels in 3 groups
        ("conv2d_smalln: needs cout <= 4", lambda: smalln(16, 3, 5)),
        ("conv2d_smalln: needs cout <= 4", lambda: smalln(16, 9, 3)),
        ("conv2d_smalln: needs cout <= 4", lambda: smalln(16, 4, 3)),
        ("conv2d_smalln: needs cout <= 4", lambda: smalln(24, 3, 3)),
        ("sinusoidal: bad arguments", lambda: ops.sinusoidal(_z(dev, 1, dtype=torch.int32), z(1), 1, 2)),
        ("sinusoidal: bad arguments", lambda: ops.sinusoidal(_z(dev, 1, dtype=torch.int32), z(3), 1, 7)),
        ("avgpool2: unsupported shape", lambda: ops.avgpool2_cl(z(6, 4), 1, 3, 2)),
    ]
    for message, call in cases:
        with pytest.raises(RuntimeError, match=message):
            call()


def test_grid_limit_refusals(backend):
    """n_img in grid z of the transposes, batch in grid y of linear_small: 65 536 is refused by name on the host, on both backends - the launch itself
    would come back as an invalid configuration on the GPU and run on the emulator."""
    dev = backend
    x = _z(dev, 65536, 1)
    with pytest.raises(RuntimeError, match="planar_to_cl: at most 65535 images"):
        ops.planar_to_cl(x.view(65536, 1, 1), 65536, 1, 1)
    with pytest.raises(RuntimeError, match="cl_to_planar: at most 65535 images"):
        ops.cl_to_planar(x, 65536, 1, 1)
    with pytest.raises(RuntimeError, match="linear_small: at most 65535 rows"):
        ops.linear_small(x, _z(dev, 1, 1))
