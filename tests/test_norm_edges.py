"""The launcher branches of the normalisation family (csrc/norm.hip, the GroupNorm-folding heads kernel of csrc/small.hip) that no per-kernel
test reaches: every float4-slot count of the one-wavefront-per-row LayerNorm, the row count at which it hands over to the grouped kernel,
the GroupNorm partial / apply pair at one float4 per group and at one row per trip, the 256-chunk cap, and the generic (not 2C = 128)
path of the heads kernel.  References are float64 on the CPU; the bar is the family's own (test_ops_parity.py: 1e-4 of the output scale -
fp32 kernels measured at or below 7.5e-7 on these shapes, so two orders of margin and no case with an exemption).  Runs on the emulator
and on the GPU; every case is a few MB at most."""
import pytest
import torch
import torch.nn.functional as F

from cvpr23_lfdm_amd import ops
from util import assert_close, rnd

TOL = 1e-4


def _layernorm_ref(x, gamma, eps=1e-5):
    """reference LayerNorm over the channel axis: (x - mean) / sqrt(var + eps) * gamma, biased variance; rows (n, C) in float64"""
    x, gamma = x.double(), gamma.double()
    mean = x.mean(dim=1, keepdim=True)
    var = x.var(dim=1, unbiased=False, keepdim=True)
    return (x - mean) / (var + eps).sqrt() * gamma


def _layernorm_case(dev, c, rows):
    x = rnd(rows, c, seed=100 + c + rows) * 3 + 1
    gamma = rnd(c, seed=7) + 1
    out = ops.layernorm_cl(x.to(dev), gamma.to(dev))
    assert_close(out.cpu(), _layernorm_ref(x, gamma), TOL, "layernorm C=%d rows=%d" % (c, rows))


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("c", [4, 192, 768, 1024])
def test_layernorm_wide_slots(backend, c, rows):
    """One wavefront per row: C = 4 uses one lane, C = 192 48 lanes of the first float4 slot, C = 768 three slots of every lane, C = 1024
    all four; one row leaves three wavefronts of the workgroup without work, five rows need a second workgroup."""
    _layernorm_case(backend, c, rows)


@pytest.mark.parametrize("c,rows", [(64, 4095), (64, 4096), (64, 4096 + 9), (128, 4095), (128, 4096), (128, 4096 + 5)])
def test_layernorm_switch_to_grouped(backend, c, rows):
    """C = 64 / 128 go to the several-rows-per-wavefront kernel from 4096 rows on: just below, at, and with a ragged last row group
    (4 rows per wavefront and trip x 2 in flight at C = 64, 2 x 2 at C = 128)."""
    _layernorm_case(backend, c, rows)


@pytest.mark.parametrize("c,pixels,b", [(32, 17, 2), (1024, 17, 2), (1024, 1, 1), (32, 4097, 1)])
def test_groupnorm_silu_edges(backend, c, pixels, b):
    """Statistics pass + apply pass with scale/shift and a residual, 8 groups: C = 32 is one float4 per group and 32 rows per trip of the
    statistics kernel (17 pixels: two ragged chunks); C = 1024 is one row per trip and reads the parameters of channels >= 512 in place;
    one pixel; 4097 pixels reach the cap of 256 chunks."""
    dev = backend
    x = rnd(b, pixels, c, seed=21) * 1.5 + 0.3
    gamma, beta = rnd(c, seed=22) + 1.0, rnd(c, seed=23)
    ss = rnd(b, 2 * c, seed=24) * 0.4
    res = rnd(b, pixels, c, seed=25)
    ref = F.group_norm(x.double().permute(0, 2, 1), 8, gamma.double(), beta.double(), eps=1e-5).permute(0, 2, 1)
    ref = F.silu(ref * (ss[:, None, :c].double() + 1) + ss[:, None, c:].double()) + res.double()
    out = ops.groupnorm_silu_cl(x.view(b * pixels, c).to(dev), b, gamma.to(dev), beta.to(dev), scale_shift=ss.to(dev),
                                residual=res.view(b * pixels, c).to(dev))
    assert_close(out.cpu().view(b, pixels, c), ref, TOL, "groupnorm C=%d pixels=%d" % (c, pixels))


def test_heads_groupnorm_generic_width(backend):
    """heads_gn_kernel away from the UNet's own width (2C = 128 keeps its fragments in registers): dim 32, the loop over LDS tables."""
    dev = backend
    b, t, s, nchunk, ch, c0, c1, groups = 2, 3, 8, 3, 32, 32, 32, 16
    pixels = t * s * s
    y = rnd(b * pixels, 2 * ch, seed=1) * 1.7 + 0.4
    x0, x1 = rnd(b * pixels, c0, seed=2), rnd(b * pixels, c1, seed=3)
    gamma, beta = rnd(2 * ch, seed=4) * 0.3 + 1, rnd(2 * ch, seed=5) * 0.3
    wf, bf, wo, bo = rnd(2, ch, seed=7, scale=0.2), rnd(2, seed=8), rnd(1, ch, seed=9, scale=0.2), rnd(1, seed=10)
    we = rnd(3, c0 + c1, seed=11, scale=0.1)
    ys = y.view(b, pixels, 2 * ch)
    yn = F.silu(F.group_norm(ys.double().permute(0, 2, 1), groups, gamma.double(), beta.double(), eps=1e-5).permute(0, 2, 1)).reshape(b * pixels, 2 * ch)
    xe, wfd, wod, wed = torch.cat((x0, x1), dim=1).double(), wf.double(), wo.double(), we.double()
    ref = torch.stack((yn[:, :ch] @ wfd[0] + bf[0] + xe @ wed[0], yn[:, :ch] @ wfd[1] + bf[1] + xe @ wed[1], yn[:, ch:] @ wod[0] + bo[0] + xe @ wed[2]), dim=1)
    ref = ref.view(b, t, s * s, 3).permute(0, 3, 1, 2)                                         # planar (B, 3, T, HW)
    yg = ys.view(b, nchunk, pixels // nchunk, groups, 2 * ch // groups)
    partial = torch.stack([yg.sum(dim=(2, 4)), (yg * yg).sum(dim=(2, 4))], dim=-1).contiguous().view(b * nchunk, 2 * groups)
    out = ops.heads_gn_res_cl_to_planar(y.to(dev), partial.to(dev), nchunk, gamma.to(dev), beta.to(dev), wf.to(dev), bf.to(dev), wo.to(dev), bo.to(dev),
                                        x0.to(dev), x1.to(dev), we.to(dev), b, t, s * s, groups=groups)
    assert_close(out.cpu(), ref, TOL, "heads with the last GroupNorm folded in, dim 32")
