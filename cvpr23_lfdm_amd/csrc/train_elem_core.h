// The launch plan the per-sample elementwise training kernels share (train_diffusion.hip, distill.hip): grid (workgroups of a sample, B),
// TD_BLOCK lanes, one float4 per lane and load, TD_QUADS loads in flight per lane, at most TD_CAP workgroups per sample - the grid-stride
// loop takes a second trip above TD_CAP * TD_QUADS * TD_BLOCK float4 = 262 144 floats per sample.  A per-sample table index is read on the
// device and clamped to the table: no host read, no address outside the table whatever the index holds.
#pragma once
#include "lfdm_device.h"

namespace {

constexpr int TD_BLOCK = 256;
constexpr int TD_QUADS = 4;          // float4 per lane and trip
constexpr int TD_CAP = 64;           // workgroups per sample

__device__ __forceinline__ int table_index(const int64_t* t, unsigned b, int t_len) {
  const int64_t v = t[b];
  return (int)(v < 0 ? 0 : v >= t_len ? t_len - 1 : v);
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// a float4 that is loaded only where `in` holds (outside the sample, or an operand the kernel does not use: zeros, no address formed)
__device__ __forceinline__ float4 ld4_if(bool in, const float* p, size_t at) { return in ? ld4(p + at) : make_float4(0.f, 0.f, 0.f, 0.f); }

// per component: bit k of `bits` set ? a : b
__device__ __forceinline__ float4 select4(unsigned bits, float4 a, float4 b) {
  return make_float4((bits & 1u) ? a.x : b.x, (bits & 2u) ? a.y : b.y, (bits & 4u) ? a.z : b.z, (bits & 8u) ? a.w : b.w);
}
// f(a, b) per component
template <class F>
__device__ __forceinline__ float4 map4(float4 a, float4 b, F f) {
  return make_float4(f(a.x, b.x), f(a.y, b.y), f(a.z, b.z), f(a.w, b.w));
}

// what the kernels' loops share: the grid-stride trips of a sample's workgroups (for (q0 = trip_first(); q0 < n4; q0 += trip_stride())) and
// the float4 slots of this lane in the current trip
__device__ __forceinline__ unsigned trip_first() { return blockIdx.x * (TD_BLOCK * TD_QUADS) + threadIdx.x; }
__device__ __forceinline__ unsigned trip_stride() { return gridDim.x * (TD_BLOCK * TD_QUADS); }
struct Trip {
  unsigned q[TD_QUADS];
  bool in[TD_QUADS];
};
__device__ __forceinline__ Trip trip_slots(unsigned q0, unsigned n4) {
  Trip s;
#pragma unroll
  for (int k = 0; k < TD_QUADS; ++k) {
    s.q[k] = q0 + (unsigned)k * TD_BLOCK;
    s.in[k] = s.q[k] < n4;
  }
  return s;
}

inline unsigned sample_blocks(int64_t n) { return lfdm_blocks(n / 4, TD_BLOCK * TD_QUADS, TD_CAP); }

}  // namespace
