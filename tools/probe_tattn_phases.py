#!/usr/bin/env python
"""Where does a wave of temporal_attn_fused_out_kernel spend its cycles?  Needs a probe build of csrc/attention_fused.hip with
-DLFDM_TATTN_STAMP (=1: the library's choice of attention order, =2: every launch on the whole order, the parent commit's) linked into a
library of its own and selected with LFDM_HIP_LIB:
  cd cvpr23_lfdm_amd && hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-mfma-vgpr-form -DLFDM_TATTN_STAMP=1 -c csrc/attention_fused.hip \
     -o build/probe/attention_fused_stamp.o && hipcc --offload-arch=gfx950 -shared -fPIC -o build/probe/tattn_stamp.so $(ls build/*.o | grep -v attention_fused.o) build/probe/attention_fused_stamp.o
  LFDM_HIP_LIB=$PWD/build/probe/tattn_stamp.so python tools/probe_tattn_phases.py
Every wave adds up s_memtime cycles per phase; a stamp is fenced, so phases that overlap in the library do not overlap here: the shares
say where the cycles go, the launch time of a probe build says nothing.  Shape: the level-0 block of the headline (40 frames, 32x32
pixels, C = 64: two waves per sequence).  With a library that has no stamps the tool only times the launch.  GPU only."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvpr23_lfdm_amd import _native, ops  # noqa: E402

t, s, dev = 40, 32, "cuda"
g = torch.Generator().manual_seed(1)
ang = torch.arange(t).float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None]
kw = dict(bias=torch.randn(8, t, t, generator=g).to(dev), rot_cos=ang.cos().contiguous().to(dev), rot_sin=ang.sin().contiguous().to(dev))
x = torch.randn(t * s * s, 64, generator=g).to(dev)
wqp, wop = ops.pack_tattn_weights(torch.randn(768, 64, generator=g) * 0.1, torch.randn(64, 256, generator=g) / 16)
wqp, wop, out = wqp.to(dev), wop.to(dev), torch.empty(t * s * s, 64, device=dev)


def launch():
    ops.temporal_attention_fused_out_cl(x, wqp, wop, 1, t, s * s, out=out, **kw)


dll = _native.library().dll
stamps = None
if hasattr(dll, "lfdm_tattn_stamp_buffer"):
    stamps = torch.zeros(256 * 8 * 8, dtype=torch.int64, device=dev)
    dll.lfdm_tattn_stamp_buffer.argtypes = [ctypes.c_void_p]
    dll.lfdm_tattn_stamp_buffer.restype = None
    dll.lfdm_tattn_stamp_buffer(stamps.data_ptr())
for _ in range(20):
    launch()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(100):
    launch()
e1.record()
torch.cuda.synchronize()
print("library %s: %.1f us per launch%s" % (_native.HIP_LIB_PATH, e0.elapsed_time(e1) * 10, " (probe build: not a timing)" if stamps is not None else ""))
if stamps is None:
    sys.exit(0)
dll.lfdm_tattn_stamp_buffer(None)
st = stamps.cpu().view(256, 8, 8)[:, :2].double()                      # two waves per sequence
names = ["projections (4 heads)", "scores (pipelined: the first tile's)", "softmax (pipelined: + the next tile's scores)", "P V + stores",
         "prologue: x rows, LayerNorm", "wait at the barrier", "to_out + residual"]
total = st[:, :, :7].sum(dim=2).mean()
print("cycles per wave, mean over 256 workgroups x 2 waves (total %.0f):" % total)
for i in (4, 0, 1, 2, 3, 5, 6):
    print("  %-48s %8.0f  %5.1f %%" % (names[i], st[:, :, i].mean(), 100 * st[:, :, i].mean() / total))
