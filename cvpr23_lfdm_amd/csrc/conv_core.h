// What the forward convolution schedules share behind their K loops (conv_igemm.hip, conv_ksw.hip, conv_pw.hip, conv_wino.hip; conv_wino4.hip
// and the float4 tail of conv_ksw.hip measured slower through it and stay written out): the host / device test for a float4 epilogue, the
// output-row index, and the tail of one float4 (or one value) of finished sums - bias, GroupNorm statistics, residual, activation, store.
// The floating-point association of that tail is part of the result; where a schedule differs (the table under
// "Convolution forward") the difference is a parameter or the site stays written out - nothing in this header unifies arithmetic.  The
// GroupNorm hand-off itself is gn_stats.h.
#pragma once
#include "gn_stats.h"
#include "norm_core.h"

// out, bias and residual are 16-byte addressable at every column that is a multiple of 4.  Each caller adds its own condition on the
// channel count (cout % 4 == 0, or cout == coutp).
__host__ __device__ inline bool conv_epilogue_vec4_ok(const lfdm_conv_params& p) {
  return (p.ldo % 4 == 0) && ((((uintptr_t)p.out) & 15) == 0) &&
         (!p.residual || ((p.ldr % 4 == 0) && ((((uintptr_t)p.residual) & 15) == 0))) &&
         (!p.bias || (((uintptr_t)p.bias) & 15) == 0);
}

// row of `out` (and `residual`) of the convolution's output pixel (qy, qx) of image img: out_scale / out_off_* place the four parity
// problems of a transposed convolution (lfdm_conv_params.deconv4)
__device__ __forceinline__ int64_t conv_out_row(const lfdm_conv_params& p, int img, int qy, int qx) {
  const int oy = qy * p.out_scale + p.out_off_y;      // (the pixel coordinates in 32 bits, only the row index in 64)
  const int ox = qx * p.out_scale + p.out_off_x;
  return ((int64_t)img * p.ho + oy) * p.wo + ox;
}

// out4 = act((v + bias) + residual), with stats(v + bias) in between: the value GroupNorm statistics are taken of.  `stats` is the
// caller's (per-column gn_accum4, conditional or not; the scalar fold of conv_splitk_reduce_vec_kernel).  ACT = false: no activation code
// at all (instantiations whose callers have none); true: the run-time code `act`.  ADDENDS_FIRST: act(v + (bias + residual)) - the
// pointwise schedule, which has no statistics.  THROUGH: the float4 leaves as a write-through store (lfdm_device.h, lfdm_store_f4_out;
// each schedule passes its own LFDM_ST_* switch).
template <bool ACT, bool ADDENDS_FIRST = false, bool THROUGH = false, class Stats>
__device__ __forceinline__ void conv_finish4(float4 v, const float4& bias, const float4& residual, int act, float* out4, Stats&& stats) {
  if (ADDENDS_FIRST) {
    float4 br = bias;
    add4(br, residual);
    add4(v, br);
  } else {
    add4(v, bias);
    stats(v);
    add4(v, residual);
  }
  if (ACT) {
    v = map4([act](float e) { return apply_act(e, act); }, v);
  }
#ifdef LFDM_PROBE_NOSTORE      // probe build only: everything but the store
  if (v.x == 123456.789f)
#endif
  lfdm_store_f4_out<THROUGH>(out4, v);
}
template <bool ACT, bool ADDENDS_FIRST = false, bool THROUGH = false>
__device__ __forceinline__ void conv_finish4(const float4& v, const float4& bias, const float4& residual, int act, float* out4) {
  conv_finish4<ACT, ADDENDS_FIRST, THROUGH>(v, bias, residual, act, out4, [](const float4&) {});
}

// the same tail for one value of a row that is not float4-addressable (bias / residual read in place)
template <class Stats>
__device__ __forceinline__ void conv_finish1(const lfdm_conv_params& p, float v, int64_t orow, int col, Stats&& stats) {
  if (p.bias) v += p.bias[col];
  stats(v);
  if (p.residual) v += p.residual[orow * p.ldr + col];
  p.out[orow * p.ldo + col] = apply_act(v, p.act);
}
