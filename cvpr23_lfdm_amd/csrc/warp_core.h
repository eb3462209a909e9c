// Bilinear sampling geometry shared by the warp kernels forward (warp.hip) and backward (train_lfae.hip) and by grid_sample: the resize of
// the low-resolution maps, the grid_sample unnormalise step, the four taps with their weights, and the two tap gradients.  The
// floating-point association of every helper is part of the result.  Include this header in front of any `#pragma clang fp contract`
// region of the including file, so that every user compiles the helpers under the same contraction mode.
// NOT here: the reader of the low-resolution maps (pixel_taps in warp.hip, warp_taps in train_lfae.hip).  The files are compiled with
// contraction allowed, and `a * b + c * d` of `bilerp` has two legal fused forms; which one a kernel gets follows from how hipcc packs the
// blends of flow_x, flow_y and occ into v_pk_* instructions, and that follows from the text around them.  Forward and backward differ in
// that today, and behind one shared reader five kernels changed output bits (profiles/glue_core_refactor_ab.txt), so both readers keep
// their text.  (render.hip's tap4 is integer arithmetic and is not this.)
#pragma once
#include "lfdm_device.h"

// ATen upsample_bilinear2d (align_corners=False) source index
__device__ __forceinline__ void resize_src(int dst, int n_in, int n_out, int& i0, int& i1, float& l1) {
  const float scale = (float)n_in / (float)n_out;
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > n_in - 1) i0 = n_in - 1;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}

__device__ __forceinline__ float bilerp(const float* m, int fw, int y0, int y1, int x0, int x1, float ly, float lx) {
  const float v00 = m[y0 * fw + x0], v01 = m[y0 * fw + x1];
  const float v10 = m[y1 * fw + x0], v11 = m[y1 * fw + x1];
  return (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
}

// tap k = 0 .. 3 is (y0, x0) (y0, x1) (y1, x0) (y1, x1): the order every blend adds them in
struct WarpTaps {
  int x0, y0;          // north-west tap (may be out of range)
  float wx0, wx1, wy0, wy1;
};

// grid_sample unnormalise (align_corners=False)
__device__ __forceinline__ float unnormalise(float g, int size) { return ((g + 1.f) * (float)size - 1.f) * 0.5f; }

__device__ __forceinline__ WarpTaps taps_at(float ix, float iy) {
  // far-out-of-range samples contribute zeros either way; keep the int conversion defined
  ix = fminf(fmaxf(ix, -1.0e6f), 1.0e6f);
  iy = fminf(fmaxf(iy, -1.0e6f), 1.0e6f);
  const float fx = floorf(ix), fy = floorf(iy);
  WarpTaps r;
  r.x0 = (int)fx;
  r.y0 = (int)fy;
  r.wx1 = ix - fx;
  r.wx0 = (fx + 1.f) - ix;
  r.wy1 = iy - fy;
  r.wy0 = (fy + 1.f) - iy;
  return r;
}

__device__ __forceinline__ bool tap_in(const WarpTaps& t, int k, int h, int w) {
  const int yy = t.y0 + (k >> 1), xx = t.x0 + (k & 1);
  return yy >= 0 && yy < h && xx >= 0 && xx < w;
}
// weight 0 + offset 0 for an out-of-range tap: zeros padding without a branch around the load
__device__ __forceinline__ float tap_weight(const WarpTaps& t, int k, bool in) {
  return in ? ((k & 1) ? t.wx1 : t.wx0) * ((k >> 1) ? t.wy1 : t.wy0) : 0.f;
}
template <class S>
__device__ __forceinline__ S tap_offset(const WarpTaps& t, int k, bool in, S stride_y, S stride_x) {
  return in ? (t.y0 + (k >> 1)) * stride_y + (t.x0 + (k & 1)) * stride_x : 0;
}
// d blend / d ix, d iy from the four tap values (grid_sampler_2d_backward: out-of-range taps hold zero)
__device__ __forceinline__ float tap_grad_x(const WarpTaps& t, float v0, float v1, float v2, float v3) {
  return (v1 - v0) * t.wy0 + (v3 - v2) * t.wy1;
}
__device__ __forceinline__ float tap_grad_y(const WarpTaps& t, float v0, float v1, float v2, float v3) {
  return (v2 - v0) * t.wx0 + (v3 - v1) * t.wx1;
}
