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

// what the kernels' loops share: the float4 slots of this lane in the current trip
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
