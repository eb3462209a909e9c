// Sampler step on the planar latent (include/lfdm_hip.h: lfdm_sampler_step_f32):
//   x0 = c_x*x - c_eps*eps;  s = max(1, quantile_0.9(|x0|) per sample);  x0 = clamp(x0,-s,s)/s;
//   x <- k_x0*x0 + k_eps*eps + k_x*x + k_noise*noise
// (reference GaussianDiffusion.ddim_sample :791-827, p_sample/p_mean_variance :712-746).
// torch.quantile sorts; here the two order statistics the linear interpolation needs are found
// exactly by a 3-pass (11/11/10 bit) radix select on the IEEE bit pattern of |x0|, with
// LDS-privatised histograms merged by integer atomics (order independent -> deterministic).
// All step-dependent scalars come from a device table indexed by a device counter so the captured
// hipGraph of one step can be replayed for every step.
#include <stdio.h>
#include <stdlib.h>
#include "lfdm_device.h"
#include "lfdm_philox.h"
#include "../../include/lfdm_hip.h"

namespace {

constexpr int NB = 2048;  // bins per histogram (11 bits)
// workspace layout per sample: hist0[NB] | h1a[NB] | h1b[NB] | h2a[NB] | h2b[NB]  (uint32)
constexpr int HIST_PER_SAMPLE = 5 * NB;

struct Ranks {
  unsigned lo, hi;  // zero-based ranks of the two order statistics
  float frac;
};

// A 2048-bin histogram held eight consecutive bins per thread (256 threads).  load_bins only ISSUES the two 16-byte loads: the
// callers request every histogram they will need before the first one is searched, so a workgroup pays the global round trip
// once instead of once per search (the histograms were written by the previous kernel's atomics).
struct Bins {
  uint4 a, b;
};
__device__ __forceinline__ Bins load_bins(const unsigned* hist) {
  const uint4* p = reinterpret_cast<const uint4*>(hist) + 2 * threadIdx.x;
  Bins h;
  h.a = p[0];
  h.b = p[1];
  return h;
}

// Finds, for up to two zero-based ranks (k[0], k[1]; NK = 1 or 2) of the same histogram, the bin holding the rank and the rank
// inside that bin.  All 256 threads call it: wave-level shuffle scans of the per-thread sums, the four wave totals through LDS,
// the owning thread walks its eight registers.  (The first version let thread 0 walk 256 partial sums serially, the second one
// wavefront walk 32 bins per lane with dependent loads - six of those per workgroup cost more than streaming the data.)
template <int NK>
__device__ void find_bins(const Bins& h, const unsigned (&k)[NK], unsigned (&bin)[NK], unsigned (&krem)[NK],
                          unsigned* s_part /*[256]*/, unsigned* s_res /*[4]*/) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned v[8] = {h.a.x, h.a.y, h.a.z, h.a.w, h.b.x, h.b.y, h.b.z, h.b.w};
  const unsigned local = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  unsigned incl = local;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl(incl, lane >= d ? lane - d : lane);
    if (lane >= d) incl += up;
  }
  if (lane == 63) s_part[wave] = incl;
  __syncthreads();
  unsigned base = 0;
#pragma unroll
  for (int w = 0; w < 3; ++w)
    if (w < wave) base += s_part[w];
  incl += base;
  const unsigned excl = incl - local;
#pragma unroll
  for (int q = 0; q < NK; ++q)
    if (k[q] >= excl && k[q] < incl) {
      unsigned run = excl, bsel = 7, rsel = 0;
      bool found = false;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (!found && run + v[i] > k[q]) {
          found = true;
          bsel = (unsigned)i;
          rsel = k[q] - run;
        }
        if (!found) run += v[i];
      }
      s_res[2 * q] = 8u * (unsigned)tid + bsel;
      s_res[2 * q + 1] = rsel;
    }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NK; ++q) {
    bin[q] = s_res[2 * q];
    krem[q] = s_res[2 * q + 1];
  }
  __syncthreads();
}

__device__ __forceinline__ void flush_hist(unsigned* lds, unsigned* glob, int nbins) {
  for (int i = threadIdx.x; i < nbins; i += 256) {
    const unsigned c = lds[i];
    if (c) atomicAdd(glob + i, c);
  }
}

// pass 0: x0 (optional) + histogram of bits [31:21].  grid (nblk, B)
__global__ __launch_bounds__(256) void quantile_pass0_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ eps,
                                                             float* __restrict__ x0buf, int64_t n,
                                                             const float* __restrict__ coef,
                                                             const int32_t* __restrict__ step_dev,
                                                             unsigned* __restrict__ hists) {
  __shared__ unsigned h[NB];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < NB; i += 256) h[i] = 0;
  __syncthreads();
  float cx = 1.f, ce = 0.f;
  if (coef) {
    const float* c = coef + (int64_t)(*step_dev) * 6;
    cx = c[0];
    ce = c[1];
  }
  const float* xb = x + (int64_t)b * n;
  const float* eb = eps ? eps + (int64_t)b * n : nullptr;
  float* ob = x0buf ? x0buf + (int64_t)b * n : nullptr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float v = xb[i];
    if (eb) v = cx * v - ce * eb[i];
    if (ob) ob[i] = v;
    const unsigned u = __float_as_uint(fabsf(v));
    atomicAdd(&h[u >> 21], 1u);
  }
  __syncthreads();
  flush_hist(h, hists + (int64_t)b * HIST_PER_SAMPLE, NB);
}

// pass 1 (shift 10, 11 bits) and pass 2 (shift 0, 10 bits).  grid (nblk, B)
template <int PASS>
__global__ __launch_bounds__(256) void quantile_pass_kernel(const float* __restrict__ v, int64_t n,
                                                            Ranks rk, unsigned* __restrict__ hists) {
  __shared__ unsigned ha[NB], hb[NB];
  __shared__ unsigned s_part[256], s_res[4];
  const int b = blockIdx.y;
  unsigned* hs = hists + (int64_t)b * HIST_PER_SAMPLE;
  for (int i = threadIdx.x; i < NB; i += 256) { ha[i] = 0; hb[i] = 0; }
  const Bins h0 = load_bins(hs);
  Bins h1a = h0, h1b = h0;
  if (PASS == 2) {
    h1a = load_bins(hs + NB);
    h1b = load_bins(hs + 2 * NB);
  }
  unsigned pa, pb;
  {
    const unsigned k0[2] = {rk.lo, rk.hi};
    unsigned bin0[2], rem0[2];
    find_bins<2>(h0, k0, bin0, rem0, s_part, s_res);
    pa = bin0[0];
    pb = bin0[1];
    if (PASS == 2) {
      const unsigned ka[1] = {rem0[0]}, kb[1] = {rem0[1]};
      unsigned qa[1], qb[1], t[1];
      find_bins<1>(h1a, ka, qa, t, s_part, s_res);
      find_bins<1>(h1b, kb, qb, t, s_part, s_res);
      pa = (pa << 11) | qa[0];
      pb = (pb << 11) | qb[0];
    }
  }
  __syncthreads();
  const float* vb = v + (int64_t)b * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned u = __float_as_uint(fabsf(vb[i]));
    if (PASS == 1) {
      const unsigned top = u >> 21, mid = (u >> 10) & 2047u;
      if (top == pa) atomicAdd(&ha[mid], 1u);
      if (top == pb) atomicAdd(&hb[mid], 1u);
    } else {
      const unsigned top = u >> 10, low = u & 1023u;
      if (top == pa) atomicAdd(&ha[low], 1u);
      if (top == pb) atomicAdd(&hb[low], 1u);
    }
  }
  __syncthreads();
  flush_hist(ha, hs + (PASS == 1 ? 1 : 3) * NB, NB);
  flush_hist(hb, hs + (PASS == 1 ? 2 : 4) * NB, NB);
}

// resolves the two order statistics from the histograms (all threads of a block)
__device__ float resolve_quantile(const unsigned* hs, Ranks rk, unsigned* s_part, unsigned* s_res) {
  const Bins h0 = load_bins(hs), h1a = load_bins(hs + NB), h1b = load_bins(hs + 2 * NB), h2a = load_bins(hs + 3 * NB),
             h2b = load_bins(hs + 4 * NB);                   // all five in flight before the first search
  const unsigned k0[2] = {rk.lo, rk.hi};
  unsigned bin0[2], rem0[2], a1[1], b1[1], a2[1], b2[1], ra[1], rb[1], t[1];
  find_bins<2>(h0, k0, bin0, rem0, s_part, s_res);
  const unsigned ka[1] = {rem0[0]}, kb[1] = {rem0[1]};
  find_bins<1>(h1a, ka, a1, ra, s_part, s_res);
  find_bins<1>(h1b, kb, b1, rb, s_part, s_res);
  find_bins<1>(h2a, ra, a2, t, s_part, s_res);
  find_bins<1>(h2b, rb, b2, t, s_part, s_res);
  const float lo = __uint_as_float((bin0[0] << 21) | (a1[0] << 10) | a2[0]);
  const float hi = __uint_as_float((bin0[1] << 21) | (b1[0] << 10) | b2[0]);
  // ATen's lerp, both branches, each ONE fused multiply-add (what its vectorised CPU kernel evaluates and torch.quantile returns):
  // weight < 0.5: lo + w d, otherwise hi - (1 - w) d.  Explicit fmaf: the bits do not depend on the compiler's contraction setting.
  const float d = hi - lo;
  return rk.frac < 0.5f ? fmaf(rk.frac, d, lo) : fmaf(-d, 1.0f - rk.frac, hi);
}

// End-of-step housekeeping of both update kernels, by the workgroup that finishes last (every workgroup has read the histograms and the step
// counter before it takes its ticket): clear the histograms for the next step and advance the step counter - two launches (zero_u32,
// advance_step) of every replayed step otherwise.  The ticket word is left at zero again.  (all threads of a block)
__device__ __forceinline__ void end_of_step(unsigned* ticket, unsigned* hists, int hist_samples, int32_t* advance_dev, unsigned* s_res) {
  __syncthreads();
  if (lfdm_workgroup_last(ticket, gridDim.x * gridDim.y, s_res)) {      // (no payload: the workgroups hand over nothing but "I am done")
    const int64_t nz = (int64_t)hist_samples * HIST_PER_SAMPLE;
    for (int64_t i = threadIdx.x; i < nz; i += 256) hists[i] = 0u;
    if (advance_dev && threadIdx.x == 0) *advance_dev += 1;
  }
}

__global__ __launch_bounds__(256) void quantile_out_kernel(Ranks rk, const unsigned* __restrict__ hists,
                                                           float* __restrict__ q_out) {
  __shared__ unsigned s_part[256], s_res[4];
  const int b = blockIdx.x;
  const float q = resolve_quantile(hists + (int64_t)b * HIST_PER_SAMPLE, rk, s_part, s_res);
  if (threadIdx.x == 0) q_out[b] = q;
}

// Known-frame conditioning (replacement method; lfdm_known_operands.frame_mask): the operands of the update kernels' KNOWN variant.
// The plain instantiations carry the empty form as their last argument, so everything in front of it sits where it sat.
// ELEM (lfdm_known_operands.elem_mask): one mask byte per ELEMENT instead of one per frame - no frames, no frame_elems, no division.
template <bool KNOWN, bool ELEM = false>
struct KnownOps {};
template <>
struct KnownOps<true, false> {
  const float* known;          // (B, n)
  const float* known_noise;    // (B, n)
  const unsigned char* mask;   // (B, frames), non-zero = known
  const float* level;          // (steps + 1, 2): row step + 1 = (a, s) after this step
  unsigned frames, frame_elems;
};
template <>
struct KnownOps<true, true> {
  const float* known;          // (B, n)
  const float* known_noise;    // (B, n)
  const unsigned char* mask;   // (B, n), non-zero = known
  const float* level;          // (steps + 1, 2): row step + 1 = (a, s) after this step
};

// x[b, i] <- a * known + s * known_noise where the frame (i / frame_elems) % frames of sample b is known (x_T, once per video).  grid (nblk, B)
__global__ __launch_bounds__(256) void known_blend_kernel(float* __restrict__ x, const float* __restrict__ known,
                                                          const float* __restrict__ known_noise,
                                                          const unsigned char* __restrict__ mask, float a, float s, unsigned n,
                                                          unsigned frames, unsigned frame_elems) {
  const int b = blockIdx.y;
  const int64_t off = (int64_t)b * n;
  const unsigned char* mb = mask + (int64_t)b * frames;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
    if (mb[(i / frame_elems) % frames]) x[off + i] = a * known[off + i] + s * known_noise[off + i];
}

// the element-mask form of known_blend_kernel: mask (B, n).  grid (nblk, B)
__global__ __launch_bounds__(256) void known_blend_elem_kernel(float* __restrict__ x, const float* __restrict__ known,
                                                               const float* __restrict__ known_noise,
                                                               const unsigned char* __restrict__ mask, float a, float s, unsigned n) {
  const int64_t off = (int64_t)blockIdx.y * n;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
    if (mask[off + i]) x[off + i] = a * known[off + i] + s * known_noise[off + i];
}

// The KNOWN variant's registers: level pair, and mask byte / known / known_noise of the PRE prefetched elements.  Empty for the plain variant.
template <bool KNOWN, bool ELEM, int PRE>
struct KnownPre {
  __device__ __forceinline__ void head(const KnownOps<KNOWN, ELEM>&, const int32_t*, int, int64_t) {}
  __device__ __forceinline__ void load(const KnownOps<KNOWN, ELEM>&, int, bool, int64_t) {}
  __device__ __forceinline__ float pick(int, float v) const { return v; }
  __device__ __forceinline__ float tail(const KnownOps<KNOWN, ELEM>&, int64_t, float v) { return v; }
};
// what the frame and the element form share: the level pair, the sample's offset and mask byte / known / known_noise of the PRE prefetched elements
template <int PRE>
struct KnownPreBase {
  float a, s, kn[PRE], kz[PRE];
  unsigned mk[PRE];
  int64_t off;
  __device__ __forceinline__ void head(const float* level, const int32_t* step_dev, int b, int64_t n) {
    const float* lv = level + 2 * ((int64_t)(*step_dev) + 1);
    a = lv[0];
    s = lv[1];
    off = (int64_t)b * n;
  }
  __device__ __forceinline__ float pick(int k, float v) const { return mk[k] ? a * kn[k] + s * kz[k] : v; }
};
template <int PRE>
struct KnownPre<true, false, PRE> : KnownPreBase<PRE> {
  using KnownPreBase<PRE>::a, KnownPreBase<PRE>::s, KnownPreBase<PRE>::kn, KnownPreBase<PRE>::kz, KnownPreBase<PRE>::mk, KnownPreBase<PRE>::off;
  const unsigned char* mb;
  // Frame of the thread's current element, kept incrementally: the thread walks i0, i0 + stride, ... (n < 2^24, 32-bit), so one division per
  // thread and one of the (uniform) stride replace a division and a modulo per element - sixteen of them stood in front of the prefetch loads.
  unsigned fr, rem, d_fr, d_rem;
  __device__ __forceinline__ void head(const KnownOps<true>& kf, const int32_t* step_dev, int b, int64_t n) {
    KnownPreBase<PRE>::head(kf.level, step_dev, b, n);
    mb = kf.mask + (int64_t)b * kf.frames;
    const unsigned i0 = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
    fr = (i0 / kf.frame_elems) % kf.frames;
    rem = i0 % kf.frame_elems;
    d_fr = (stride / kf.frame_elems) % kf.frames;
    d_rem = stride % kf.frame_elems;
  }
  __device__ __forceinline__ void next(const KnownOps<true>& kf) {     // fr + d_fr + 1 <= 2 * frames - 1: one subtraction is enough
    rem += d_rem;
    const bool carry = rem >= kf.frame_elems;
    rem -= carry ? kf.frame_elems : 0u;
    fr += d_fr + (carry ? 1u : 0u);
    fr -= fr >= kf.frames ? kf.frames : 0u;
  }
  // called for k = 0 .. PRE - 1 in order, then tail() for every further element in order
  __device__ __forceinline__ void load(const KnownOps<true>& kf, int k, bool in, int64_t i) {
    const unsigned u = in ? (unsigned)i : 0u;
    mk[k] = in ? mb[fr] : 0u;
    kn[k] = in ? kf.known[off + u] : 0.f;
    kz[k] = in ? kf.known_noise[off + u] : 0.f;
    next(kf);
  }
  __device__ __forceinline__ float tail(const KnownOps<true>& kf, int64_t i, float v) {
    if (mb[fr]) v = a * kf.known[off + i] + s * kf.known_noise[off + i];
    next(kf);
    return v;
  }
};

// ELEM: the mask byte sits where the element sits - the frame variant's walk (fr, rem, next) has no counterpart, the byte is one more load of
// the prefetch batch at the element's own index.
template <int PRE>
struct KnownPre<true, true, PRE> : KnownPreBase<PRE> {
  using KnownPreBase<PRE>::a, KnownPreBase<PRE>::s, KnownPreBase<PRE>::kn, KnownPreBase<PRE>::kz, KnownPreBase<PRE>::mk, KnownPreBase<PRE>::off;
  __device__ __forceinline__ void head(const KnownOps<true, true>& kf, const int32_t* step_dev, int b, int64_t n) {
    KnownPreBase<PRE>::head(kf.level, step_dev, b, n);
  }
  __device__ __forceinline__ void load(const KnownOps<true, true>& kf, int k, bool in, int64_t i) {
    const unsigned u = in ? (unsigned)i : 0u;
    mk[k] = in ? kf.mask[off + u] : 0u;
    kn[k] = in ? kf.known[off + u] : 0.f;
    kz[k] = in ? kf.known_noise[off + u] : 0.f;
  }
  __device__ __forceinline__ float tail(const KnownOps<true, true>& kf, int64_t i, float v) {
    if (kf.mask[off + i]) v = a * kf.known[off + i] + s * kf.known_noise[off + i];
    return v;
  }
};

// Counter-based step noise (lfdm_sampler_step_params.seeds / .window): the operands of the update kernel's GENERATING variant, which
// computes noise[b, i] = lfdm_noise_element(seeds[b], i, step, 2, *window) in registers instead of loading it.  Empty for the loading variants.
template <bool GEN>
struct GenOps {};
template <>
struct GenOps<true> {
  const uint64_t* seeds;     // (B): the videos' seeds
  const uint32_t* window;    // one device word: the window number (0 for one video)
};
// The generating variant's registers: the video's key and the two uniform counter words.  The three words are wave-uniform loads; nothing
// per element is requested from memory, and the Philox rounds of the PRE prefetched elements are issued next to the prefetch loads, in front
// of the five histogram scans, whose barriers and round trips they run under.  Each thread evaluates the quad of its own element (four
// neighbouring threads share one: the element mapping is the loading variant's, one element per thread and trip, so that the update
// expression below is one source expression for both).
template <bool GEN>
struct GenPre {
  __device__ __forceinline__ void head(const GenOps<GEN>&, const int32_t*, int) {}
  __device__ __forceinline__ float draw(bool, int64_t) const { return 0.f; }
};
template <>
struct GenPre<true> {
  uint64_t seed;
  uint32_t window, step;
  __device__ __forceinline__ void head(const GenOps<true>& g, const int32_t* step_dev, int b) {
    seed = g.seeds[b];
    window = *g.window;
    step = (uint32_t)(*step_dev);
  }
  __device__ __forceinline__ float draw(bool in, int64_t i) const {          // (i < n < 2^24)
    return in ? lfdm_noise_element(seed, (uint32_t)i, step, (uint32_t)LFDM_NOISE_STREAM_STEP, window) : 0.f;
  }
};

// Both optional operand sets as ONE trailing kernel argument: empty (one byte, like KnownOps<false> alone before) for the plain instantiation,
// so the kernel-argument layout of the loading instantiations is what it was.
template <bool KNOWN, bool GEN, bool ELEM = false>
struct StepOps : KnownOps<KNOWN, ELEM>, GenOps<GEN> {};

// KNOWN: the final store of x selects a * known + s * known_noise at the frames the byte mask marks; x0_out, the threshold, the housekeeping and
// every other frame are the plain variant's.  What was chosen for the loads: the step counter and, behind it, the level pair are requested first
// (that two-trip chain runs under the five histogram scans, like the operands); the mask byte, known and known_noise of the PRE prefetched
// elements are loaded UNCONDITIONALLY in the same batch as today's prefetch (no round trip in front of the search; values at unmasked frames
// are loaded but only ever pass through a select, so they may be NaN); the loop behind the prefetched elements branches on the mask byte.
// The frame index of an element is carried along, not divided out (KnownPre).
// ELEM: the mask holds one byte per element (KnownOps<true, true>); same load order, the byte is requested at the element's own index.
// GEN: `noise` is not an operand (null); the step noise is computed where it is loaded otherwise (GenPre).
// grid (nblk, B)
template <bool KNOWN, bool GEN, bool ELEM>
__global__ __launch_bounds__(256) void sampler_update_kernel(float* __restrict__ x,
                                                             const float* __restrict__ eps,
                                                             const float* __restrict__ noise,
                                                             float* __restrict__ x0buf,
                                                             float* __restrict__ x0_out, int64_t n,
                                                             const float* __restrict__ coef,
                                                             const int32_t* step_dev,      // (no __restrict__: advance_dev is the same word)
                                                             Ranks rk, unsigned* __restrict__ hists, int hist_samples,
                                                             unsigned* __restrict__ ticket, int32_t* advance_dev, StepOps<KNOWN, GEN, ELEM> so) {
  __shared__ unsigned s_part[256], s_res[4];
  const KnownOps<KNOWN, ELEM>& kf = so;
  const GenOps<GEN>& gen = so;
  const int b = blockIdx.y;
  float* xb = x + (int64_t)b * n;
  const float* eb = eps + (int64_t)b * n;
  const float* nb = noise ? noise + (int64_t)b * n : nullptr;
  const float* x0b = x0buf + (int64_t)b * n;
  float* x0o = x0_out ? x0_out + (int64_t)b * n : nullptr;
  // The first PRE elements of this thread (all of them at the C2 latent: 122 880 / (60 x 256) = 8) are requested BEFORE the histograms are
  // searched: five scans with barriers stand between the kernel's start and the threshold, the operands' round trip runs under them (round 6).
  constexpr int PRE = 8;
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  float p_x0[PRE], p_e[PRE], p_x[PRE], p_n[PRE];
  KnownPre<KNOWN, ELEM, PRE> kp;
  kp.head(kf, step_dev, b, n);
  GenPre<GEN> gp;
  gp.head(gen, step_dev, b);
#pragma unroll
  for (int k = 0; k < PRE; ++k) {
    const int64_t i = i0 + k * stride;
    const bool in = i < n;
    p_x0[k] = in ? x0b[i] : 0.f;
    p_e[k] = in ? eb[i] : 0.f;
    p_x[k] = in ? xb[i] : 0.f;
    if constexpr (GEN)
      p_n[k] = gp.draw(in, i);
    else
      p_n[k] = (in && nb) ? nb[i] : 0.f;
    kp.load(kf, k, in, i);
  }
  // (written out in both update kernels: behind a shared inline function three KNOWN instantiations schedule differently - DESIGN.md section 3)
  float s = 1.0f;                       // rk.frac < 0: static clipping, x0.clamp(-1, 1) (use_dynamic_thres=False, :729-732)
  if (rk.frac >= 0.f) {
    s = resolve_quantile(hists + (int64_t)b * HIST_PER_SAMPLE, rk, s_part, s_res);
    s = fmaxf(s, 1.0f);
  }
  const float* c = coef + (int64_t)(*step_dev) * 6;
  const float k_x0 = c[2], k_eps = c[3], k_x = c[4], k_noise = c[5];
#pragma unroll
  for (int k = 0; k < PRE; ++k) {
    const int64_t i = i0 + k * stride;
    if (i < n) {
      float x0 = fminf(fmaxf(p_x0[k], -s), s) / s;
      if (x0o) x0o[i] = x0;
      float v = k_x0 * x0 + k_eps * p_e[k];
      if (k_x != 0.f) v += k_x * p_x[k];
      if (k_noise != 0.f && (GEN || nb)) v += k_noise * p_n[k];
      v = kp.pick(k, v);
      xb[i] = v;
    }
  }
  for (int64_t i = i0 + PRE * stride; i < n; i += stride) {
    float x0 = x0b[i];
    x0 = fminf(fmaxf(x0, -s), s) / s;
    if (x0o) x0o[i] = x0;
    float v = k_x0 * x0 + k_eps * eb[i];
    if (k_x != 0.f) v += k_x * xb[i];
    if constexpr (GEN) {
      if (k_noise != 0.f) v += k_noise * gp.draw(true, i);
    } else {
      if (k_noise != 0.f && nb) v += k_noise * nb[i];
    }
    v = kp.tail(kf, i, v);
    xb[i] = v;
  }
  end_of_step(ticket, hists, hist_samples, advance_dev, s_res);
}

// Multistep form of the update (lfdm_sampler_step_params.multistep: DPM-Solver++ on the thresholded data prediction m = clamp(x0,-s,s)/s):
//   x <- k_x*x + k_m*m + k_prev*m_prev,   hist <- m       coef[step] = { c_x, c_eps, k_x, k_m, k_prev, - }
// m_prev is the previous step's m, read from hist and replaced by this step's m by the same thread (one buffer suffices).  eps is not an
// operand any more (pass 0 consumed it).  k_prev == 0 / k_x == 0 skip their operand: on a first-order step hist may be uninitialised
// memory.  Prefetch, end-of-step housekeeping and the KNOWN variant (only the store of x differs: hist and x0_out receive m at every frame)
// as in sampler_update_kernel.  grid (nblk, B)
template <bool KNOWN, bool ELEM>
__global__ __launch_bounds__(256) void sampler_update_ms_kernel(float* __restrict__ x,
                                                                float* __restrict__ hist,
                                                                const float* __restrict__ x0buf,
                                                                float* __restrict__ x0_out, int64_t n,
                                                                const float* __restrict__ coef,
                                                                const int32_t* step_dev,      // (no __restrict__: advance_dev is the same word)
                                                                Ranks rk, unsigned* __restrict__ hists, int hist_samples,
                                                                unsigned* __restrict__ ticket, int32_t* advance_dev, KnownOps<KNOWN, ELEM> kf) {
  __shared__ unsigned s_part[256], s_res[4];
  const int b = blockIdx.y;
  float* xb = x + (int64_t)b * n;
  float* hb = hist + (int64_t)b * n;
  const float* x0b = x0buf + (int64_t)b * n;
  float* x0o = x0_out ? x0_out + (int64_t)b * n : nullptr;
  constexpr int PRE = 8;               // requested before the five histogram scans, like sampler_update_kernel's
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  float p_x0[PRE], p_x[PRE], p_m[PRE];
  KnownPre<KNOWN, ELEM, PRE> kp;
  kp.head(kf, step_dev, b, n);
#pragma unroll
  for (int k = 0; k < PRE; ++k) {
    const int64_t i = i0 + k * stride;
    const bool in = i < n;
    p_x0[k] = in ? x0b[i] : 0.f;
    p_x[k] = in ? xb[i] : 0.f;
    p_m[k] = in ? hb[i] : 0.f;         // (possibly uninitialised memory: only used when k_prev != 0)
    kp.load(kf, k, in, i);
  }
  float s = 1.0f;                       // rk.frac < 0: static clamp to [-1, 1]
  if (rk.frac >= 0.f) {
    s = resolve_quantile(hists + (int64_t)b * HIST_PER_SAMPLE, rk, s_part, s_res);
    s = fmaxf(s, 1.0f);
  }
  const float* c = coef + (int64_t)(*step_dev) * 6;
  const float k_x = c[2], k_m = c[3], k_prev = c[4];
#pragma unroll
  for (int k = 0; k < PRE; ++k) {
    const int64_t i = i0 + k * stride;
    if (i < n) {
      const float m = fminf(fmaxf(p_x0[k], -s), s) / s;
      if (x0o) x0o[i] = m;
      float v = k_m * m;
      if (k_prev != 0.f) v += k_prev * p_m[k];
      if (k_x != 0.f) v += k_x * p_x[k];
      v = kp.pick(k, v);
      hb[i] = m;
      xb[i] = v;
    }
  }
  for (int64_t i = i0 + PRE * stride; i < n; i += stride) {
    const float m = fminf(fmaxf(x0b[i], -s), s) / s;
    if (x0o) x0o[i] = m;
    float v = k_m * m;
    if (k_prev != 0.f) v += k_prev * hb[i];
    if (k_x != 0.f) v += k_x * xb[i];
    v = kp.tail(kf, i, v);
    hb[i] = m;
    xb[i] = v;
  }
  end_of_step(ticket, hists, hist_samples, advance_dev, s_res);
}

// classifier-free guidance: out = null + (cond - null) * scale   (reference :525-526)
__device__ __forceinline__ float cfg_guided(float cond, float null, float scale) { return null + (cond - null) * scale; }

__global__ __launch_bounds__(256) void cfg_combine_kernel(const float* __restrict__ cond_eps,
                                                          const float* __restrict__ null_eps,
                                                          float scale, float* __restrict__ out,
                                                          int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float a = null_eps[i];
    out[i] = cfg_guided(cond_eps[i], a, scale);
  }
}

// Guidance rescale (Lin et al. 2024): out = g * (phi * std(cond) / std(g) + 1 - phi), g = cfg_guided(cond, null, scale), the
// standard deviations per sample over its n elements, unbiased.  Two launches, no atomics:
//   cfg_rescale_stats_kernel   grid (G, batch): workgroup j of sample b strides over the sample's quads (4 adjacent elements; thread t of trip
//                              r owns quad (r G + j) 256 + t), every thread keeps sum cond, sum cond^2, sum g, sum g^2 in double, the workgroup
//                              folds them (block_sum_f64) and writes ONE 4-double partial
//   cfg_rescale_apply_kernel   grid (G, batch): every workgroup folds its sample's G <= 256 partials (thread t holds partial t), forms the factor
//                              in double, rounds it to fp32 once and streams out = g * factor over its quads
// A quad is ONE 16-byte load / store where the sample's bases are 16-byte aligned and the quad lies inside the sample, four element accesses
// otherwise; a thread adds its quad's elements in index order on either path, and G is a function of n alone: which thread adds what, and in
// which order, does not depend on the batch, the addresses or the run.  The product of two floats is exact in double, so an fma contraction
// of the accumulations changes no bit.
constexpr int kRescaleQuadsPerBlock = 256;        // one trip of a workgroup: 256 quads = 1024 elements
constexpr int kRescaleMaxBlocks = 256;            // G's cap: the fold of launch B is one partial per thread
inline unsigned rescale_blocks(int64_t n) { return lfdm_blocks((n + 3) / 4, kRescaleQuadsPerBlock, kRescaleMaxBlocks); }

// elements j < cnt of quad q of a sample: cnt = 4 inside the sample, n - 4 q in its ragged last quad
__device__ __forceinline__ int rescale_load_quad(const float* __restrict__ cb, const float* __restrict__ nb, bool wide, int64_t q, int64_t n,
                                                 float (&c)[4], float (&a)[4]) {
  const int64_t i = 4 * q;
  if (wide && i + 4 <= n) {
    const float4 cv = *reinterpret_cast<const float4*>(cb + i), av = *reinterpret_cast<const float4*>(nb + i);
    c[0] = cv.x; c[1] = cv.y; c[2] = cv.z; c[3] = cv.w;
    a[0] = av.x; a[1] = av.y; a[2] = av.z; a[3] = av.w;
    return 4;
  }
  const int cnt = n - i < 4 ? (int)(n - i) : 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = j < cnt ? cb[i + j] : 0.f;
    a[j] = j < cnt ? nb[i + j] : 0.f;
  }
  return cnt;
}

__global__ __launch_bounds__(256) void cfg_rescale_stats_kernel(const float* cond_eps, const float* null_eps, float scale, int64_t n,
                                                                double* __restrict__ partial) {
  __shared__ double slots[4][4];
  const int b = blockIdx.y;
  const float* cb = cond_eps + (int64_t)b * n;
  const float* nb = null_eps + (int64_t)b * n;
  const bool wide = ((reinterpret_cast<uintptr_t>(cb) | reinterpret_cast<uintptr_t>(nb)) & 15u) == 0;
  const int64_t quads = (n + 3) >> 2;
  double s[4] = {0.0, 0.0, 0.0, 0.0};               // sum cond, sum cond^2, sum g, sum g^2
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    float c[4], a[4];
    const int cnt = rescale_load_quad(cb, nb, wide, q, n, c, a);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) {
        const double cd = (double)c[j], gd = (double)cfg_guided(c[j], a[j], scale);
        s[0] += cd;
        s[1] += cd * cd;
        s[2] += gd;
        s[3] += gd * gd;
      }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = block_sum_f64(s[k], slots[k]);
  if (threadIdx.x == 0) {
    double* p = partial + ((int64_t)b * gridDim.x + blockIdx.x) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = s[k];
  }
}

// out may alias cond_eps or null_eps (no __restrict__ on the three): a thread reads its quad before it writes it and no other thread touches it
__global__ __launch_bounds__(256) void cfg_rescale_apply_kernel(const float* cond_eps, const float* null_eps, float scale, float phi, float* out,
                                                                float* factor_out, int64_t n, const double* __restrict__ partial) {
  __shared__ double slots[4][4];
  const int b = blockIdx.y;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (threadIdx.x < gridDim.x) {                     // (launch A ran on the same G; x + 0.0 is x in the other threads)
    const double* p = partial + ((int64_t)b * gridDim.x + threadIdx.x) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = p[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = block_sum_f64(s[k], slots[k]);
  const double nd = (double)n;
  const double var_c = fmax((s[1] - s[0] * s[0] / nd) / (nd - 1.0), 0.0);
  const double var_g = fmax((s[3] - s[2] * s[2] / nd) / (nd - 1.0), 0.0);
  const double std_g = sqrt(var_g);
  const double fd = std_g == 0.0 ? 1.0 : (double)phi * (sqrt(var_c) / std_g) + (1.0 - (double)phi);
  const float f = (float)fd;
  if (factor_out && blockIdx.x == 0 && threadIdx.x == 0) factor_out[b] = f;
  const float* cb = cond_eps + (int64_t)b * n;
  const float* nb = null_eps + (int64_t)b * n;
  float* ob = out + (int64_t)b * n;
  const bool wide = ((reinterpret_cast<uintptr_t>(cb) | reinterpret_cast<uintptr_t>(nb) | reinterpret_cast<uintptr_t>(ob)) & 15u) == 0;
  const int64_t quads = (n + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    float c[4], a[4];
    const int cnt = rescale_load_quad(cb, nb, wide, q, n, c, a);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = cfg_guided(c[j], a[j], scale) * f;
    const int64_t i = 4 * q;
    if (wide && cnt == 4) {
      *reinterpret_cast<float4*>(ob + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) ob[i + j] = v[j];
    }
  }
}

// Histogram clear.  NOT hipMemsetAsync: a memset node inside a captured hipGraph stopped writing zeros
// after a few replays on ROCm 7.2 / gfx950 (it filled a stale 32-bit pattern instead), which silently
// corrupted every quantile of the second video onwards; a plain kernel node replays correctly.
__global__ __launch_bounds__(256) void zero_u32_kernel(unsigned* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0u;
}

__global__ void advance_step_kernel(int32_t* step_dev) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *step_dev += 1;
}

// Counter-based noise written to memory (lfdm_philox_normal_f32 / lfdm_philox_bits_u32): out[b * row_stride + i], i < n, of video seeds[b].
// One thread owns quad q = i >> 2 (no output is computed twice) and stores it as ONE 16-byte word where the row's base is 16-byte aligned
// and the quad lies inside the row; the ragged last quad and rows on other alignments are stored element by element.  BITS: the raw
// Philox words instead of the normals (tests).  grid (nblk, B)
template <bool BITS>
__global__ __launch_bounds__(256) void philox_fill_kernel(uint32_t* __restrict__ out, const uint64_t* __restrict__ seeds, uint32_t n,
                                                          int64_t row_stride, uint32_t stream_id, uint32_t step, uint32_t window) {
  const int b = blockIdx.y;
  const uint64_t seed = seeds[b];
  uint32_t* ob = out + (int64_t)b * row_stride;
  const bool wide = (reinterpret_cast<uintptr_t>(ob) & 15u) == 0;
  const uint32_t quads = (n + 3u) >> 2;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < quads; q += gridDim.x * 256u) {
    const lfdm_philox_quad o = lfdm_noise_bits(seed, q, step, stream_id, window);
    uint32_t v[4];
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) v[j] = BITS ? o.r[j] : __float_as_uint(lfdm_noise_normal(o, j));
    const uint32_t i = 4u * q;
    if (wide && i + 4u <= n) {
      uint4 w;
      w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3];
      *reinterpret_cast<uint4*>(ob + i) = w;
    } else {
#pragma unroll
      for (unsigned j = 0; j < 4; ++j)
        if (i + j < n) ob[i + j] = v[j];
    }
  }
}

template <bool BITS>
int run_philox_fill(const char* what, void* out, const uint64_t* seeds, int batch, int64_t n, int64_t row_stride, unsigned stream_id,
                    unsigned step, unsigned window, hipStream_t stream) {
  if (!out || !seeds || batch <= 0 || n <= 0 || n >= (1 << 24) || row_stride < n || stream_id > 2u)
    return lfdm_fail(LFDM_EINVAL, "%s: bad arguments (0 < n < 2^24, row_stride >= n, stream_id 0 .. 2)", what);
  const int64_t quads = (n + 3) / 4;
  LFDM_LAUNCH((philox_fill_kernel<BITS>), dim3(lfdm_blocks(quads, 256, 1024), batch), dim3(256), 0, stream, reinterpret_cast<uint32_t*>(out), seeds, (uint32_t)n,
              row_stride, (uint32_t)stream_id, (uint32_t)step, (uint32_t)window);
  return lfdm_check_launch(what);
}

Ranks make_ranks(int64_t n, float quantile) {
  // torch.quantile: rank = q * (n - 1) evaluated in the input dtype (fp32), then floor / lerp
  const float pos = quantile * (float)(n - 1);
  const float fl = floorf(pos);
  Ranks r;
  r.lo = (unsigned)fl;
  r.hi = r.lo + 1 < (unsigned)n ? r.lo + 1 : (unsigned)(n - 1);
  r.frac = pos - fl;
  return r;
}

unsigned blocks_for(int64_t n) { return lfdm_blocks(n, 256 * 8, 512); }

// The sampler workspace: per-sample histograms | the x0 prediction of every sample | the ticket word (64 bytes).  lfdm_sampler_ws_bytes and
// every entry point that is handed the workspace cut it here; lfdm_abs_quantile_f32 is handed the histograms alone and takes only them.
unsigned* carve_hists(lfdm_carver& c, int batch) { return c.take<unsigned>((size_t)batch * HIST_PER_SAMPLE); }
struct SamplerWs {
  unsigned* hists;
  float* x0buf;
  unsigned* ticket;
  size_t bytes;
};
SamplerWs carve_sampler_ws(void* ws, int batch, int64_t n) {
  lfdm_carver c(ws);
  SamplerWs w;
  w.hists = carve_hists(c, batch);
  w.x0buf = c.take<float>((size_t)batch * (size_t)n);
  w.ticket = c.take<unsigned>(16);
  w.bytes = c.bytes;
  return w;
}

void clear_hists(unsigned* hists, int batch, hipStream_t stream) {
  const int64_t nz = (int64_t)batch * HIST_PER_SAMPLE;
  LFDM_LAUNCH(zero_u32_kernel, dim3(lfdm_blocks(nz, 256, 64)), dim3(256), 0, stream, hists, nz);
}

int run_select(const float* v, int batch, int64_t n, Ranks rk, unsigned* hists, hipStream_t stream) {
  const dim3 grid(blocks_for(n), batch), block(256);
  LFDM_LAUNCH((quantile_pass_kernel<1>), grid, block, 0, stream, v, n, rk, hists);
  LFDM_LAUNCH((quantile_pass_kernel<2>), grid, block, 0, stream, v, n, rk, hists);
  return 0;
}

}  // namespace

extern "C" int lfdm_cfg_combine_f32(const float* cond_eps, const float* null_eps, float scale,
                                    float* out, int64_t n, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!cond_eps || !null_eps || !out || n <= 0)
    return lfdm_fail(LFDM_EINVAL, "cfg_combine: bad arguments");
  LFDM_LAUNCH(cfg_combine_kernel, dim3(lfdm_blocks(n, 256, 2048)), dim3(256), 0, stream, cond_eps, null_eps, scale,
              out, n);
  return lfdm_check_launch("cfg_combine");
}

// one 4-double partial per workgroup of launch A; 0 for arguments the entry point refuses
extern "C" size_t lfdm_cfg_rescale_ws_bytes(int batch, int64_t n) {
  if (batch <= 0 || n < 2) return 0;
  return (size_t)batch * rescale_blocks(n) * 4 * sizeof(double);
}

extern "C" int lfdm_cfg_combine_rescale_f32(const float* cond_eps, const float* null_eps, float scale, float phi, float* out, float* factor_out,
                                            int batch, int64_t n, void* ws, size_t ws_bytes, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!cond_eps || !null_eps || !out || !ws || batch <= 0 || batch > 65535 || n < 2 || !(phi >= 0.f && phi <= 1.f))
    return lfdm_fail(LFDM_EINVAL, "cfg_combine_rescale: bad arguments (0 < batch < 65536, n >= 2 - an unbiased deviation -, phi in [0, 1], a workspace)");
  if (!lfdm_aligned<8>(ws) || ws_bytes < lfdm_cfg_rescale_ws_bytes(batch, n))
    return lfdm_fail(LFDM_EINVAL, "cfg_combine_rescale: workspace too small (lfdm_cfg_rescale_ws_bytes) or not 8-byte aligned");
  const dim3 grid(rescale_blocks(n), batch), block(256);
  double* partial = (double*)ws;
  LFDM_LAUNCH(cfg_rescale_stats_kernel, grid, block, 0, stream, cond_eps, null_eps, scale, n, partial);
  LFDM_LAUNCH(cfg_rescale_apply_kernel, grid, block, 0, stream, cond_eps, null_eps, scale, phi, out, factor_out, n, (const double*)partial);
  return lfdm_check_launch("cfg_combine_rescale");
}

extern "C" size_t lfdm_sampler_ws_bytes(int batch, int64_t n) {
  return carve_sampler_ws(nullptr, batch, n).bytes;
}

extern "C" int lfdm_sampler_ws_init(void* ws, size_t ws_bytes, int batch, int64_t n, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ws || batch <= 0 || n <= 0 || ws_bytes < lfdm_sampler_ws_bytes(batch, n))
    return lfdm_fail(LFDM_EWORKSPACE, "sampler_ws_init: workspace too small");
  const SamplerWs w = carve_sampler_ws(ws, batch, n);
  clear_hists(w.hists, batch, stream);
  LFDM_LAUNCH(zero_u32_kernel, dim3(1), dim3(256), 0, stream, w.ticket, (int64_t)16);
  return lfdm_check_launch("sampler_ws_init");
}

extern "C" int lfdm_abs_quantile_f32(const float* x, int batch, int64_t n, float quantile,
                                     float* q_out, void* ws, size_t ws_bytes, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !q_out || batch <= 0 || n <= 0 || n >= (1 << 24) || quantile < 0.f || quantile > 1.f)
    return lfdm_fail(LFDM_EINVAL, "abs_quantile: bad arguments (n < 2^24)");
  lfdm_carver c(ws);
  unsigned* hists = carve_hists(c, batch);
  if (!ws || ws_bytes < c.bytes)
    return lfdm_fail(LFDM_EWORKSPACE, "abs_quantile: workspace too small");
  clear_hists(hists, batch, stream);
  const Ranks rk = make_ranks(n, quantile);
  LFDM_LAUNCH(quantile_pass0_kernel, dim3(blocks_for(n), batch), dim3(256), 0, stream, x,
              (const float*)nullptr, (float*)nullptr, n, (const float*)nullptr,
              (const int32_t*)nullptr, hists);
  run_select(x, batch, n, rk, hists, stream);
  LFDM_LAUNCH(quantile_out_kernel, dim3(batch), dim3(256), 0, stream, rk, (const unsigned*)hists, q_out);
  clear_hists(hists, batch, stream);      // leave the histograms cleared: lfdm_sampler_step_f32 relies on that when it is handed the same workspace
  return lfdm_check_launch("abs_quantile");
}

extern "C" int lfdm_philox_normal_f32(float* out, const uint64_t* seeds, int batch, int64_t n, int64_t row_stride, unsigned stream_id,
                                      unsigned step, unsigned window, lfdm_stream_t stream_) {
  return run_philox_fill<false>("philox_normal", out, seeds, batch, n, row_stride, stream_id, step, window, (hipStream_t)stream_);
}

extern "C" int lfdm_philox_bits_u32(uint32_t* out, const uint64_t* seeds, int batch, int64_t n, int64_t row_stride, unsigned stream_id,
                                    unsigned step, unsigned window, lfdm_stream_t stream_) {
  return run_philox_fill<true>("philox_bits", out, seeds, batch, n, row_stride, stream_id, step, window, (hipStream_t)stream_);
}

namespace {

// The one check of lfdm_known_operands, for the step (with_level) and the blend (host scalars: level is not looked at): the form the fields
// select, or a refusal (negative).
enum { KNOWN_NONE = 0, KNOWN_FRAME = 1, KNOWN_ELEM = 2 };
int check_known(const char* what, const lfdm_known_operands& k, int64_t n, bool with_level) {
  const bool mask = k.frame_mask || k.elem_mask, level = with_level && k.level;
  if (!k.known && !k.known_noise && !mask && !level && !k.frames && !k.frame_elems) return KNOWN_NONE;
  if (!k.known || !k.known_noise || !mask || (with_level && !k.level))
    return lfdm_fail(LFDM_EINVAL, "%s: known, known_noise, a mask (frame_mask or elem_mask)%s must all be given", what, with_level ? " and level" : "");
  if (k.frame_mask && k.elem_mask)
    return lfdm_fail(LFDM_EINVAL, "%s: frame_mask and elem_mask exclude each other", what);
  if (n <= 0 || n >= (1 << 24))
    return lfdm_fail(LFDM_EINVAL, "%s: n = %lld must lie in (0, 2^24)", what, (long long)n);
  if (k.elem_mask) {
    if (k.frames || k.frame_elems)
      return lfdm_fail(LFDM_EINVAL, "%s: elem_mask has no frame split (frames and frame_elems must be 0)", what);
    return KNOWN_ELEM;
  }
  if (k.frames <= 0 || k.frame_elems <= 0 || k.frames > n || k.frame_elems > n || n % ((int64_t)k.frames * k.frame_elems) != 0)
    return lfdm_fail(LFDM_EINVAL, "%s: n = %lld must be a multiple of frames * frame_elems = %d * %lld", what, (long long)n, k.frames, (long long)k.frame_elems);
  return KNOWN_FRAME;
}

// The one check of the generating operands: 0 = the loading update, 1 = the generating one, or a refusal (negative).
int check_gen(const char* what, const lfdm_sampler_step_params& p) {
  if (!p.seeds && !p.window) return 0;
  if (!p.seeds || !p.window)
    return lfdm_fail(LFDM_EINVAL, "%s: seeds (batch 64-bit words) and window (one 32-bit word) must both be given, on the device", what);
  if (p.multistep)
    return lfdm_fail(LFDM_EINVAL, "%s: seeds with multistep: the multistep update draws nothing", what);
  if (p.noise)
    return lfdm_fail(LFDM_EINVAL, "%s: seeds (the noise is computed in the kernel) and noise exclude each other", what);
  return 1;
}

template <bool KNOWN, bool ELEM>
KnownOps<KNOWN, ELEM> known_ops(const lfdm_known_operands& k) {
  KnownOps<KNOWN, ELEM> kf;
  if constexpr (KNOWN) {
    kf.known = k.known;
    kf.known_noise = k.known_noise;
    kf.mask = ELEM ? k.elem_mask : k.frame_mask;
    kf.level = k.level;
    if constexpr (!ELEM) {
      kf.frames = (unsigned)k.frames;
      kf.frame_elems = (unsigned)k.frame_elems;
    }
  }
  return kf;
}

// what the update launch takes besides the caller's parameters
struct UpdateLaunch {
  dim3 grid;
  float* x0buf;
  Ranks rk;
  unsigned* hists;
  int hist_samples;
  unsigned* ticket;
  hipStream_t stream;
};

// MS: the multistep update (hist) instead of the DDIM / DDPM one (noise); KNOWN: the update kernel's known-frame instantiation, ELEM: its
// element-mask one; GEN: the generating one.
template <bool MS, bool KNOWN, bool GEN, bool ELEM>
void launch_update(const lfdm_sampler_step_params& p, const UpdateLaunch& u) {
  static_assert(!(MS && GEN), "the multistep update draws nothing");
  const KnownOps<KNOWN, ELEM> kf = known_ops<KNOWN, ELEM>(p.known);
  int32_t* advance_dev = p.advance ? p.step_dev : nullptr;
  if constexpr (MS) {
    LFDM_LAUNCH((sampler_update_ms_kernel<KNOWN, ELEM>), u.grid, dim3(256), 0, u.stream, p.x, p.hist, (const float*)u.x0buf, p.x0_out, p.n, p.coef,
                (const int32_t*)p.step_dev, u.rk, u.hists, u.hist_samples, u.ticket, advance_dev, kf);
  } else {
    GenOps<GEN> gen;
    if constexpr (GEN) {
      gen.seeds = p.seeds;
      gen.window = p.window;
    }
    LFDM_LAUNCH((sampler_update_kernel<KNOWN, GEN, ELEM>), u.grid, dim3(256), 0, u.stream, p.x, p.eps, p.noise, u.x0buf, p.x0_out, p.n,
                p.coef, (const int32_t*)p.step_dev, u.rk, u.hists, u.hist_samples, u.ticket, advance_dev, StepOps<KNOWN, GEN, ELEM>{kf, gen});
  }
}

// the nine instantiations in use: {plain, frame, element} x {DDIM / DDPM loading, DDIM / DDPM generating, multistep}
template <bool KNOWN, bool ELEM>
void launch_update(const lfdm_sampler_step_params& p, bool gen, const UpdateLaunch& u) {
  if (p.multistep)
    launch_update<true, KNOWN, false, ELEM>(p, u);
  else if (gen)
    launch_update<false, KNOWN, true, ELEM>(p, u);
  else
    launch_update<false, KNOWN, false, ELEM>(p, u);
}

}  // namespace

// The one launch sequence of every sampler step: [histogram clear for batch > 2] pass 0, two select passes, update.
extern "C" int lfdm_sampler_step_f32(const lfdm_sampler_step_params* pp, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* what = "sampler_step";
  if (!pp) return lfdm_fail(LFDM_EINVAL, "%s: null parameters", what);
  const lfdm_sampler_step_params& p = *pp;
  const int gen = check_gen(what, p);
  if (gen < 0) return gen;
  const int known = check_known(what, p.known, p.n, true);
  if (known < 0) return known;
  if (!p.x || !p.eps || (p.multistep && !p.hist) || !p.coef || !p.step_dev || p.batch <= 0 || p.n <= 0 || p.n >= (1 << 24))
    return lfdm_fail(LFDM_EINVAL, "%s: bad arguments (n < 2^24)", what);
  const SamplerWs w = carve_sampler_ws(p.ws, p.batch, p.n);
  if (!p.ws || p.ws_bytes < w.bytes)
    return lfdm_fail(LFDM_EWORKSPACE, "%s: workspace too small", what);
  const bool dynamic = p.quantile >= 0.f;         // quantile < 0: static clipping to [-1, 1] (GaussianDiffusion's own default)
  if (dynamic && p.quantile > 1.f)
    return lfdm_fail(LFDM_EINVAL, "%s: quantile must lie in [0, 1] (or be negative for the static clamp to [-1, 1])", what);
  Ranks rk = make_ranks(p.n, dynamic ? p.quantile : 0.f);
  if (!dynamic) rk.frac = -1.f;
  // the histograms are clear on entry: lfdm_sampler_ws_init, then the last workgroup of every update kernel - for one or two samples
  // (a single workgroup clearing more would lengthen the kernel's tail: larger batches keep the clearing launch)
  const bool fold_clear = p.batch <= 2;
  if (!fold_clear) clear_hists(w.hists, p.batch, stream);
  const dim3 grid(blocks_for(p.n), p.batch), block(256);
  LFDM_LAUNCH(quantile_pass0_kernel, grid, block, 0, stream, (const float*)p.x, p.eps, w.x0buf, p.n, p.coef,
              (const int32_t*)p.step_dev, w.hists);     // (also the x0 = c_x*x - c_eps*eps pass: columns 0-1 of either table)
  if (dynamic) run_select(w.x0buf, p.batch, p.n, rk, w.hists, stream);
  const UpdateLaunch u = {grid, w.x0buf, rk, w.hists, fold_clear ? p.batch : 0, w.ticket, stream};
  if (known == KNOWN_ELEM)
    launch_update<true, true>(p, gen != 0, u);
  else if (known == KNOWN_FRAME)
    launch_update<true, false>(p, gen != 0, u);
  else
    launch_update<false, false>(p, gen != 0, u);
  return lfdm_check_launch(what);
}

extern "C" int lfdm_known_blend_f32(float* x, const lfdm_known_operands* k, float a, float s, int batch, int64_t n, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !k || batch <= 0)
    return lfdm_fail(LFDM_EINVAL, "known_blend: bad arguments");
  const int known = check_known("known_blend", *k, n, false);
  if (known < 0) return known;
  if (known == KNOWN_NONE)
    return lfdm_fail(LFDM_EINVAL, "known_blend: known, known_noise and a mask (frame_mask or elem_mask) must all be given");
  const dim3 grid(blocks_for(n), batch), block(256);
  if (known == KNOWN_ELEM) {
    LFDM_LAUNCH(known_blend_elem_kernel, grid, block, 0, stream, x, k->known, k->known_noise, k->elem_mask, a, s, (unsigned)n);
  } else {
    LFDM_LAUNCH(known_blend_kernel, grid, block, 0, stream, x, k->known, k->known_noise, k->frame_mask, a, s, (unsigned)n, (unsigned)k->frames,
                (unsigned)k->frame_elems);
  }
  return lfdm_check_launch("known_blend");
}
