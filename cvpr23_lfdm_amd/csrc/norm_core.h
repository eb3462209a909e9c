// What the normalisation kernels and the pointwise kernels around them share (norm.hip, train_norm.hip, the heads kernels of small.hip,
// conv_core.h): component-wise float4 arithmetic and the row statistics of the channel LayerNorm.  The floating-point association of every
// helper is the one of the sites it replaced and is part of the result; where two sites differ (the table
// "Normalisation") the difference stays at the call site - nothing in this header unifies arithmetic.  The GroupNorm statistics and the
// per-channel table made of them are gn_stats.h; the LayerNorm helpers of the attention kernels (attn_core.h: ln_accum, ln_stats_slots4)
// use other arithmetic and are not these.
#pragma once
#include "lfdm_device.h"

// ---- float4, component by component ----
// f over the x, then y, z, w components of every operand
template <class F, class... V>
__device__ __forceinline__ float4 map4(F&& f, const V&... v) {
  return make_float4(f(v.x...), f(v.y...), f(v.z...), f(v.w...));
}
__device__ __forceinline__ void add4(float4& v, const float4& a) {
  v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
}
__device__ __forceinline__ float4 mul4(const float4& a, const float4& b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 fma4(const float4& v, const float4& a, const float4& b) {
  return make_float4(fmaf(v.x, a.x, b.x), fmaf(v.y, a.y, b.y), fmaf(v.z, a.z, b.z), fmaf(v.w, a.w, b.w));
}
__device__ __forceinline__ float4 sub4(const float4& v, float m) { return make_float4(v.x - m, v.y - m, v.z - m, v.w - m); }
// pairwise: (x + y) + (z + w)
__device__ __forceinline__ float hsum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float dot4(const float4& a, const float4& w) { return (a.x * w.x + a.y * w.y) + (a.z * w.z + a.w * w.w); }
__device__ __forceinline__ float sq4(const float4& v) { return dot4(v, v); }

// ---- channel LayerNorm: statistics of one row ----
// Two passes over values held in registers: sum -> mean, squares of the centred values -> (biased) variance.  The forward kernels divide by
// sqrtf(var + eps), the backward kernels multiply by its reciprocal: that stays with the callers.
struct ln_stats {
  float mean, var;
};

// Wide form: one wavefront per row, lane holds the float4 columns lane, lane + 64, ... < c4n of the row in v[0..3] (slots past the row: 0,
// and left out of the sums)
__device__ __forceinline__ ln_stats ln_row_stats_wave(const float4 (&v)[4], int lane, int c4n, int channels) {
  float s = 0.f, q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (lane + 64 * i < c4n) s += hsum4(v[i]);
  const float mean = wave_sum(s) / (float)channels;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (lane + 64 * i < c4n) q += sq4(sub4(v[i], mean));
  return {mean, wave_sum(q) / (float)channels};
}

// Grouped form: C4N adjacent lanes (a power of two <= 64) hold one row of 4 * C4N channels, one float4 each
template <int C4N>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = 1; m < C4N; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
// ... `centred` = v - mean, which both callers go on with
template <int C4N>
__device__ __forceinline__ ln_stats ln_row_stats_group(const float4& v, float4& centred) {
  const float mean = group_sum<C4N>(hsum4(v)) / (float)(4 * C4N);
  centred = sub4(v, mean);
  return {mean, group_sum<C4N>(sq4(centred)) / (float)(4 * C4N)};
}
