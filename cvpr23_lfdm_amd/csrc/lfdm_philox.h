// Counter-based noise: every standard normal the sampler draws in noise="counter" mode is a pure function of
// (video seed, window, stream, step, element).  One definition, two consumers: the fill kernels of sampler.hip (lfdm_philox_normal_f32,
// lfdm_philox_bits_u32) and the generating instantiation of sampler_update_kernel.
//
// THE DEFINITION (part of the contract - tests/test_counter_noise.py restates it in numpy):
//   generator  Philox4x32-10 (Salmon et al. 2011): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds;
//              one round: (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then the key is bumped.
//   key        (seed & 0xffffffff, seed >> 32) of the video's unsigned 64-bit seed
//   counter    (q, step, stream, window):  q = i >> 2 for element i of the sample's flat (3, T, S, S) latent (n < 2^24);  step = the sampler
//              step index (0 for the two per-video draws);  stream 0 = x_T, 1 = known-frame noise, 2 = step noise;  window = 0 for one video,
//              the window number in a long video
//   uniforms   u(r) = ((r >> 8) + 0.5) * 2^-24, never 0.  Evaluated in fp32 as written: exact for u < 1/2; above, the 25-bit sum rounds to the
//              24-bit grid (ties to even), so u is then a multiple of 2^-24 and u = 1 (R = 0) turns up once in 2^25 draws - never an infinity.
//              Against the real-number formula that is a deviation of z of at most sqrt(2^-24) = 2.4e-4 (R at u = 1 - 2^-25), typically 1e-5.
//   normals    from the four outputs r0..r3 of quad q (Box-Muller):  R(r) = sqrt(-2 ln u(r))
//              z[4q] = R(r0) cos(2 pi u(r1)),  z[4q+1] = R(r0) sin(2 pi u(r1)),  z[4q+2] = R(r2) cos(2 pi u(r3)),  z[4q+3] = R(r2) sin(2 pi u(r3))
//              u >= 2^-25, so |z| <= sqrt(50 ln 2) = 5.89: the tails beyond are cut (probability 3.9e-9 per value).
// The GPU build takes ln, sin and cos from the hardware (v_log_f32, v_sin_f32, v_cos_f32: about 1 ulp, not correctly rounded; the last
// two take their argument in revolutions, so 2 pi u is never rounded); the emulator build keeps logf / sinf / cosf - the same switch as
// fast_exp in lfdm_device.h.  Plain C++: 64-bit products and shifts, no inline assembly.
#pragma once
#include "lfdm_device.h"

#define LFDM_PHILOX_M0 0xD2511F53u
#define LFDM_PHILOX_M1 0xCD9E8D57u
#define LFDM_PHILOX_W0 0x9E3779B9u
#define LFDM_PHILOX_W1 0xBB67AE85u

enum { LFDM_NOISE_STREAM_XT = 0, LFDM_NOISE_STREAM_KNOWN = 1, LFDM_NOISE_STREAM_STEP = 2 };

struct lfdm_philox_quad {
  uint32_t r[4];
};

__device__ __forceinline__ lfdm_philox_quad lfdm_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                               uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)LFDM_PHILOX_M0 * c0, p1 = (uint64_t)LFDM_PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += LFDM_PHILOX_W0;
    k1 += LFDM_PHILOX_W1;
  }
  lfdm_philox_quad o;
  o.r[0] = c0;
  o.r[1] = c1;
  o.r[2] = c2;
  o.r[3] = c3;
  return o;
}

// the four raw words of quad q of one video
__device__ __forceinline__ lfdm_philox_quad lfdm_noise_bits(uint64_t seed, uint32_t q, uint32_t step, uint32_t stream_id, uint32_t window) {
  return lfdm_philox4x32_10(q, step, stream_id, window, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__device__ __forceinline__ float lfdm_philox_uniform(uint32_t r) { return ((float)(r >> 8) + 0.5f) * 5.9604644775390625e-8f; }

#if defined(LFDM_EMU_BUILD)
static inline float lfdm_noise_ln(float u) { return logf(u); }
static inline float lfdm_noise_cos_rev(float u) { return cosf(6.28318530717958647692f * u); }
static inline float lfdm_noise_sin_rev(float u) { return sinf(6.28318530717958647692f * u); }
#else
__device__ __forceinline__ float lfdm_noise_ln(float u) { return __builtin_amdgcn_logf(u) * 0.69314718055994530942f; }   // u >= 2^-25: normal
__device__ __forceinline__ float lfdm_noise_cos_rev(float u) { return __builtin_amdgcn_cosf(u); }                         // argument in revolutions
__device__ __forceinline__ float lfdm_noise_sin_rev(float u) { return __builtin_amdgcn_sinf(u); }
#endif

// THE one function both consumers call: normal number `j` (0 .. 3) of a quad.  Every caller evaluates exactly this expression, so a value
// the fill kernel stores and the value the update kernel computes in registers for the same (seed, counter, j) are the same bits.
__device__ __forceinline__ float lfdm_noise_normal(const lfdm_philox_quad& o, unsigned j) {
  const uint32_t ra = (j & 2u) ? o.r[2] : o.r[0], rb = (j & 2u) ? o.r[3] : o.r[1];
  const float radius = sqrtf(-2.0f * lfdm_noise_ln(lfdm_philox_uniform(ra)));
  const float u = lfdm_philox_uniform(rb);
  return radius * ((j & 1u) ? lfdm_noise_sin_rev(u) : lfdm_noise_cos_rev(u));
}

// element i of one video's draw (the update kernel's form: one element per thread and trip)
__device__ __forceinline__ float lfdm_noise_element(uint64_t seed, uint32_t i, uint32_t step, uint32_t stream_id, uint32_t window) {
  return lfdm_noise_normal(lfdm_noise_bits(seed, i >> 2, step, stream_id, window), i & 3u);
}
