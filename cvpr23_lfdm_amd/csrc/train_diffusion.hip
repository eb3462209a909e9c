// The diffusion edge of the DM training step with known frames / elements held clean (include/lfdm_hip.h: lfdm_train_qsample_f32,
// lfdm_masked_loss_fwd_f32, lfdm_masked_loss_bwd_f32).  Random-mask training (RaMViD, Hoeppe et al. 2022): some frames or
// elements of x_start stay clean inside x_noisy, the loss counts the unknown elements only.
//   train_qsample_kernel<MASK>      x_noisy = known ? x_start : a[t_b] * x_start + s[t_b] * noise
//   masked_loss_fwd_kernel<MASK,L2> S_b = sum_unknown |noise - pred| (or its square), N_b = the unknown count, pred_x0 = r[t_b] * x_noisy
//                                   - m[t_b] * pred (known: x_noisy) in the same pass; the last workgroup folds the partials:
//                                   loss = (1 / B) sum_b S_b / max(N_b, 1), inv_count[b] = 1 / max(N_b, 1)
//   masked_loss_bwd_kernel<MASK,L2> dpred = -sign(noise - pred) * g * inv_count[b] / B (l2: 2 (pred - noise) in place of the sign), known: 0.f
//   objective_loss_fwd_kernel<OBJ,MASK,L2> / objective_loss_bwd_kernel<OBJ,MASK,L2>  the same two for a training objective (the noise, x0
//                                   or v) with a per-timestep loss weight and the per-sample means (lfdm_objective_loss_*_f32)
// MASK: 0 none, 1 one byte per frame (B, frames), 2 one byte per element (B, n) - the forms of the sampler's known operands (sampler.hip).
// All three: grid (workgroups of a sample, B), one float4 per lane and load, TD_QUADS loads in flight per lane, at most TD_CAP workgroups per
// sample (the grid-stride loop takes a second trip above TD_CAP * TD_QUADS * 256 float4 = 262 144 floats per sample).  t, the table values
// and the first mask bytes are requested in front of the element loads; t is read on the device and clamped to the table (no host read, no
// address outside the table whatever t holds).  No floating-point atomics, one owner per output element, no scratch.
// The reduction (lfdm_device.h, "In-launch hand-off between workgroups", single-writer form): a lane sums the 16 terms of one trip in fp32 (pairwise
// inside a float4, then a chain of four) and adds that to a double; lanes -> workgroup by a fixed tree of doubles in LDS; workgroup partials
// (S and N as doubles) are 8-byte agent-scope words; the workgroup that takes the last ticket folds each sample's partials in index order
// and the samples in index order, in double.  Two runs on the same inputs give the same bits.
#include "train_elem_core.h"
#include "../../include/lfdm_hip.h"

// a * x_start + s * noise and r * x_noisy - m * pred are torch's expressions: two products and one sum, each rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int MASK_NONE = 0, MASK_FRAME = 1, MASK_ELEM = 2;

struct TrainMask {
  const unsigned char* mask;         // MASK_FRAME: (B, frames); MASK_ELEM: (B, n); non-zero = known
  unsigned frames, frame_elems;      // MASK_FRAME only; frame_elems % 4 == 0: a float4 never straddles two frames
};

// the four known flags (bit k: element i + k) of the float4 at element i of sample b
template <int MASK>
__device__ __forceinline__ unsigned known_bits(const TrainMask& m, unsigned b, unsigned n, unsigned i) {
  if constexpr (MASK == MASK_FRAME) {
    return m.mask[(size_t)b * m.frames + (i / m.frame_elems) % m.frames] ? 0xFu : 0u;
  } else if constexpr (MASK == MASK_ELEM) {
    const unsigned w = *reinterpret_cast<const unsigned*>(m.mask + (size_t)b * n + i);
    return ((w & 0xFFu) ? 1u : 0u) | ((w & 0xFF00u) ? 2u : 0u) | ((w & 0xFF0000u) ? 4u : 0u) | ((w & 0xFF000000u) ? 8u : 0u);
  } else {
    return 0u;
  }
}

template <int MASK>
__global__ __launch_bounds__(TD_BLOCK) void train_qsample_kernel(const float* __restrict__ x_start, const float* __restrict__ noise,
                                                                 const int64_t* __restrict__ t, const float* __restrict__ a_tab,
                                                                 const float* __restrict__ s_tab, int t_len, TrainMask m,
                                                                 float* __restrict__ x_noisy, unsigned n) {
  const unsigned b = blockIdx.y, n4 = n >> 2;
  const size_t off = (size_t)b * n;
  const int ti = table_index(t, b, t_len);
  const float a = a_tab[ti], s = s_tab[ti];
  for (unsigned q0 = blockIdx.x * (TD_BLOCK * TD_QUADS) + threadIdx.x; q0 < n4; q0 += gridDim.x * (TD_BLOCK * TD_QUADS)) {
    const Trip sl = trip_slots(q0, n4);
    unsigned kb[TD_QUADS];
    float4 x0[TD_QUADS], z[TD_QUADS];
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) kb[k] = sl.in[k] ? known_bits<MASK>(m, b, n, sl.q[k] * 4u) : 0u;
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      x0[k] = sl.in[k] ? ld4(x_start + off + (size_t)sl.q[k] * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      z[k] = sl.in[k] ? ld4(noise + off + (size_t)sl.q[k] * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      if (!sl.in[k]) continue;
      float4 o;
      o.x = (kb[k] & 1u) ? x0[k].x : a * x0[k].x + s * z[k].x;
      o.y = (kb[k] & 2u) ? x0[k].y : a * x0[k].y + s * z[k].y;
      o.z = (kb[k] & 4u) ? x0[k].z : a * x0[k].z + s * z[k].z;
      o.w = (kb[k] & 8u) ? x0[k].w : a * x0[k].w + s * z[k].w;
      st4(x_noisy + off + (size_t)sl.q[k] * 4, o);
    }
  }
}

static_assert(TD_BLOCK == 256, "block_tree_sum (lfdm_device.h) folds 256 lanes");

template <bool L2>
__device__ __forceinline__ float loss_term(float nz, float pr) {
  const float d = nz - pr;
  return L2 ? d * d : fabsf(d);
}

template <int MASK, bool L2>
__global__ __launch_bounds__(TD_BLOCK) void masked_loss_fwd_kernel(const float* __restrict__ noise, const float* __restrict__ pred,
                                                                   const float* __restrict__ x_noisy, const int64_t* __restrict__ t,
                                                                   const float* __restrict__ r_tab, const float* __restrict__ m_tab, int t_len,
                                                                   TrainMask m, float* __restrict__ loss, float* __restrict__ inv_count,
                                                                   float* __restrict__ pred_x0, unsigned n, unsigned long long* part,
                                                                   unsigned* ticket) {
  __shared__ double s_sum[TD_BLOCK];
  __shared__ double s_cnt[TD_BLOCK];
  __shared__ unsigned s_last;
  const unsigned b = blockIdx.y, n4 = n >> 2;
  const size_t off = (size_t)b * n;
  const int ti = table_index(t, b, t_len);
  const float r = r_tab[ti], mm = m_tab[ti];
  double acc = 0.0;
  unsigned unknown = 0;
  for (unsigned q0 = blockIdx.x * (TD_BLOCK * TD_QUADS) + threadIdx.x; q0 < n4; q0 += gridDim.x * (TD_BLOCK * TD_QUADS)) {
    const Trip sl = trip_slots(q0, n4);
    unsigned kb[TD_QUADS];
    float4 nz[TD_QUADS], pr[TD_QUADS], xn[TD_QUADS];
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) kb[k] = sl.in[k] ? known_bits<MASK>(m, b, n, sl.q[k] * 4u) : 0xFu;     // (outside the sample: counts as known)
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      nz[k] = sl.in[k] ? ld4(noise + off + (size_t)sl.q[k] * 4) : zero;
      pr[k] = sl.in[k] ? ld4(pred + off + (size_t)sl.q[k] * 4) : zero;
      xn[k] = sl.in[k] ? ld4(x_noisy + off + (size_t)sl.q[k] * 4) : zero;
    }
    float trip = 0.f;       // 16 terms: pairwise inside a float4, a chain over the four
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      const float ex = (kb[k] & 1u) ? 0.f : loss_term<L2>(nz[k].x, pr[k].x), ey = (kb[k] & 2u) ? 0.f : loss_term<L2>(nz[k].y, pr[k].y);
      const float ez = (kb[k] & 4u) ? 0.f : loss_term<L2>(nz[k].z, pr[k].z), ew = (kb[k] & 8u) ? 0.f : loss_term<L2>(nz[k].w, pr[k].w);
      trip += (ex + ey) + (ez + ew);
      unknown += 4u - (unsigned)__builtin_popcount(kb[k]);
      if (!sl.in[k]) continue;
      float4 o;
      o.x = (kb[k] & 1u) ? xn[k].x : r * xn[k].x - mm * pr[k].x;
      o.y = (kb[k] & 2u) ? xn[k].y : r * xn[k].y - mm * pr[k].y;
      o.z = (kb[k] & 4u) ? xn[k].z : r * xn[k].z - mm * pr[k].z;
      o.w = (kb[k] & 8u) ? xn[k].w : r * xn[k].w - mm * pr[k].w;
      st4(pred_x0 + off + (size_t)sl.q[k] * 4, o);
    }
    acc += (double)trip;
  }
  s_sum[threadIdx.x] = acc;
  s_cnt[threadIdx.x] = (double)unknown;
  block_tree_sum(s_sum);
  block_tree_sum(s_cnt);
  // (partials as 8-byte agent-scope words, one writer per workgroup who drains before the ticket: lfdm_device.h, "In-launch hand-off
  // between workgroups")
  const unsigned nbx = gridDim.x, nblocks = gridDim.x * gridDim.y;
  unsigned long long* part_cnt = part + (size_t)nblocks;
  if (threadIdx.x == 0) {
    lfdm_agent_store_u64(part + (size_t)b * nbx + blockIdx.x, __builtin_bit_cast(unsigned long long, s_sum[0]));
    lfdm_agent_store_u64(part_cnt + (size_t)b * nbx + blockIdx.x, __builtin_bit_cast(unsigned long long, s_cnt[0]));
    LFDM_DRAIN_STORES();
  }
  if (!lfdm_workgroup_last(ticket, nblocks, &s_last)) return;
  // the last workgroup: one lane per sample folds the sample's partials in index order, then the samples in a fixed tree
  const unsigned batch = gridDim.y;
  double mine = 0.0;
  for (unsigned bb = threadIdx.x; bb < batch; bb += TD_BLOCK) {
    double sum = 0.0, cnt = 0.0;
    for (unsigned j = 0; j < nbx; ++j) {
      sum += __builtin_bit_cast(double, lfdm_agent_load_u64(part + (size_t)bb * nbx + j));
      cnt += __builtin_bit_cast(double, lfdm_agent_load_u64(part_cnt + (size_t)bb * nbx + j));
    }
    const double inv = 1.0 / (cnt < 1.0 ? 1.0 : cnt);
    inv_count[bb] = (float)inv;
    mine += sum * inv;
  }
  s_sum[threadIdx.x] = mine;
  block_tree_sum(s_sum);
  if (threadIdx.x == 0) *loss = (float)(s_sum[0] / (double)batch);
}

template <int MASK, bool L2>
__global__ __launch_bounds__(TD_BLOCK) void masked_loss_bwd_kernel(const float* __restrict__ noise, const float* __restrict__ pred, TrainMask m,
                                                                   const float* __restrict__ inv_count, const float* __restrict__ gout,
                                                                   float* __restrict__ dpred, unsigned n) {
  const unsigned b = blockIdx.y, n4 = n >> 2;
  const size_t off = (size_t)b * n;
  const float c = (*gout * inv_count[b]) / (float)gridDim.y;
  for (unsigned q0 = blockIdx.x * (TD_BLOCK * TD_QUADS) + threadIdx.x; q0 < n4; q0 += gridDim.x * (TD_BLOCK * TD_QUADS)) {
    const Trip sl = trip_slots(q0, n4);
    unsigned kb[TD_QUADS];
    float4 nz[TD_QUADS], pr[TD_QUADS];
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) kb[k] = sl.in[k] ? known_bits<MASK>(m, b, n, sl.q[k] * 4u) : 0u;
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      nz[k] = sl.in[k] ? ld4(noise + off + (size_t)sl.q[k] * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      pr[k] = sl.in[k] ? ld4(pred + off + (size_t)sl.q[k] * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    auto grad = [c](float z, float p) {
      if constexpr (L2) return (2.f * (p - z)) * c;
      else return z > p ? -c : (z < p ? c : 0.f);
    };
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      if (!sl.in[k]) continue;
      float4 o;
      o.x = (kb[k] & 1u) ? 0.f : grad(nz[k].x, pr[k].x);
      o.y = (kb[k] & 2u) ? 0.f : grad(nz[k].y, pr[k].y);
      o.z = (kb[k] & 4u) ? 0.f : grad(nz[k].z, pr[k].z);
      o.w = (kb[k] & 8u) ? 0.f : grad(nz[k].w, pr[k].w);
      st4(dpred + off + (size_t)sl.q[k] * 4, o);
    }
  }
}

// ---- training objectives: what the denoiser's output `out` is compared with, and how x0 comes back from it
//   OBJ_NOISE  target = noise                        pred_x0 = r * x_noisy - m * out
//   OBJ_X0     target = x_start                      pred_x0 = out
//   OBJ_V      target = a * noise - s * x_start      pred_x0 = a * x_noisy - s * out      (Salimans & Ho 2022)
// The target lives in registers only.  An operand the objective does not use is never loaded (it may be null).
constexpr int OBJ_NOISE = LFDM_OBJ_NOISE, OBJ_X0 = LFDM_OBJ_X0, OBJ_V = LFDM_OBJ_V;

struct ObjTables {
  const float *a, *s, *r, *m, *w;    // w: the per-timestep loss weight, null = 1
  int len;
};

template <int OBJ>
__device__ __forceinline__ float obj_target(float x0, float z, float a, float s) {
  if constexpr (OBJ == OBJ_NOISE) return z;
  else if constexpr (OBJ == OBJ_X0) return x0;
  else return a * z - s * x0;
}

// (cx, ce): (r, m) for OBJ_NOISE, (a, s) for OBJ_V
template <int OBJ>
__device__ __forceinline__ float obj_pred_x0(float xn, float o, float cx, float ce) {
  if constexpr (OBJ == OBJ_X0) return o;
  else return cx * xn - ce * o;
}

template <int OBJ>
__device__ __forceinline__ float4 obj_target4(float4 x0, float4 z, float a, float s) {
  return make_float4(obj_target<OBJ>(x0.x, z.x, a, s), obj_target<OBJ>(x0.y, z.y, a, s), obj_target<OBJ>(x0.z, z.z, a, s),
                     obj_target<OBJ>(x0.w, z.w, a, s));
}

// masked_loss_fwd_kernel with the objective's target and pred_x0, the per-sample means and the weight in the last workgroup's fold; for
// OBJ_NOISE without weights every shared output has masked_loss_fwd_kernel's bits (same terms, same order).
template <int OBJ, int MASK, bool L2>
__global__ __launch_bounds__(TD_BLOCK) void objective_loss_fwd_kernel(const float* __restrict__ x_start, const float* __restrict__ noise,
                                                                      const float* __restrict__ out, const float* __restrict__ x_noisy,
                                                                      const int64_t* __restrict__ t, ObjTables tab, TrainMask m,
                                                                      float* __restrict__ loss, float* __restrict__ inv_count,
                                                                      float* __restrict__ sample_loss, float* __restrict__ pred_x0, unsigned n,
                                                                      unsigned long long* part, unsigned* ticket) {
  constexpr bool USE_X0 = OBJ != OBJ_NOISE, USE_Z = OBJ != OBJ_X0, USE_XN = OBJ != OBJ_X0 || MASK != MASK_NONE;
  __shared__ double s_sum[TD_BLOCK];
  __shared__ double s_cnt[TD_BLOCK];
  __shared__ unsigned s_last;
  const unsigned b = blockIdx.y, n4 = n >> 2;
  const size_t off = (size_t)b * n;
  const int ti = table_index(t, b, tab.len);
  float a = 0.f, s = 0.f, cx = 0.f, ce = 0.f;
  if constexpr (OBJ == OBJ_V) { a = tab.a[ti]; s = tab.s[ti]; cx = a; ce = s; }
  if constexpr (OBJ == OBJ_NOISE) { cx = tab.r[ti]; ce = tab.m[ti]; }
  double acc = 0.0;
  unsigned unknown = 0;
  for (unsigned q0 = blockIdx.x * (TD_BLOCK * TD_QUADS) + threadIdx.x; q0 < n4; q0 += gridDim.x * (TD_BLOCK * TD_QUADS)) {
    const Trip sl = trip_slots(q0, n4);
    unsigned kb[TD_QUADS];
    float4 x0[TD_QUADS], nz[TD_QUADS], pr[TD_QUADS], xn[TD_QUADS];
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) kb[k] = sl.in[k] ? known_bits<MASK>(m, b, n, sl.q[k] * 4u) : 0xFu;     // (outside the sample: counts as known)
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      const size_t at = off + (size_t)sl.q[k] * 4;
      x0[k] = zero, nz[k] = zero, xn[k] = zero;
      if constexpr (USE_X0) x0[k] = sl.in[k] ? ld4(x_start + at) : zero;
      if constexpr (USE_Z) nz[k] = sl.in[k] ? ld4(noise + at) : zero;
      pr[k] = sl.in[k] ? ld4(out + at) : zero;
      if constexpr (USE_XN) xn[k] = sl.in[k] ? ld4(x_noisy + at) : zero;
    }
    float trip = 0.f;       // 16 terms: pairwise inside a float4, a chain over the four
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      const float4 tg = obj_target4<OBJ>(x0[k], nz[k], a, s);
      const float ex = (kb[k] & 1u) ? 0.f : loss_term<L2>(tg.x, pr[k].x), ey = (kb[k] & 2u) ? 0.f : loss_term<L2>(tg.y, pr[k].y);
      const float ez = (kb[k] & 4u) ? 0.f : loss_term<L2>(tg.z, pr[k].z), ew = (kb[k] & 8u) ? 0.f : loss_term<L2>(tg.w, pr[k].w);
      trip += (ex + ey) + (ez + ew);
      unknown += 4u - (unsigned)__builtin_popcount(kb[k]);
      if (!sl.in[k]) continue;
      float4 o;
      o.x = (kb[k] & 1u) ? xn[k].x : obj_pred_x0<OBJ>(xn[k].x, pr[k].x, cx, ce);
      o.y = (kb[k] & 2u) ? xn[k].y : obj_pred_x0<OBJ>(xn[k].y, pr[k].y, cx, ce);
      o.z = (kb[k] & 4u) ? xn[k].z : obj_pred_x0<OBJ>(xn[k].z, pr[k].z, cx, ce);
      o.w = (kb[k] & 8u) ? xn[k].w : obj_pred_x0<OBJ>(xn[k].w, pr[k].w, cx, ce);
      st4(pred_x0 + off + (size_t)sl.q[k] * 4, o);
    }
    acc += (double)trip;
  }
  s_sum[threadIdx.x] = acc;
  s_cnt[threadIdx.x] = (double)unknown;
  block_tree_sum(s_sum);
  block_tree_sum(s_cnt);
  // (the hand-off of masked_loss_fwd_kernel: single-writer partials, drained before the ticket)
  const unsigned nbx = gridDim.x, nblocks = gridDim.x * gridDim.y;
  unsigned long long* part_cnt = part + (size_t)nblocks;
  if (threadIdx.x == 0) {
    lfdm_agent_store_u64(part + (size_t)b * nbx + blockIdx.x, __builtin_bit_cast(unsigned long long, s_sum[0]));
    lfdm_agent_store_u64(part_cnt + (size_t)b * nbx + blockIdx.x, __builtin_bit_cast(unsigned long long, s_cnt[0]));
    LFDM_DRAIN_STORES();
  }
  if (!lfdm_workgroup_last(ticket, nblocks, &s_last)) return;
  // the last workgroup: one lane per sample folds the sample's partials in index order and applies the weight of its timestep in double
  const unsigned batch = gridDim.y;
  double mine = 0.0;
  for (unsigned bb = threadIdx.x; bb < batch; bb += TD_BLOCK) {
    double sum = 0.0, cnt = 0.0;
    for (unsigned j = 0; j < nbx; ++j) {
      sum += __builtin_bit_cast(double, lfdm_agent_load_u64(part + (size_t)bb * nbx + j));
      cnt += __builtin_bit_cast(double, lfdm_agent_load_u64(part_cnt + (size_t)bb * nbx + j));
    }
    const double inv = 1.0 / (cnt < 1.0 ? 1.0 : cnt);
    inv_count[bb] = (float)inv;
    sample_loss[bb] = (float)(sum * inv);      // unweighted
    if (tab.w) mine += (double)tab.w[table_index(t, bb, tab.len)] * sum * inv;
    else mine += sum * inv;
  }
  s_sum[threadIdx.x] = mine;
  block_tree_sum(s_sum);
  if (threadIdx.x == 0) *loss = (float)(s_sum[0] / (double)batch);
}

// dout = c_b * d term / d out, c_b = ((g * inv_count[b]) * w[t_b]) / B in fp32 in that order (null w: no product - masked_loss_bwd_kernel's
// bits for OBJ_NOISE); the target is recomputed from x_start / noise; known: 0.f
template <int OBJ, int MASK, bool L2>
__global__ __launch_bounds__(TD_BLOCK) void objective_loss_bwd_kernel(const float* __restrict__ x_start, const float* __restrict__ noise,
                                                                      const float* __restrict__ out, const int64_t* __restrict__ t,
                                                                      ObjTables tab, TrainMask m, const float* __restrict__ inv_count,
                                                                      const float* __restrict__ gout, float* __restrict__ dout, unsigned n) {
  constexpr bool USE_X0 = OBJ != OBJ_NOISE, USE_Z = OBJ != OBJ_X0;
  const unsigned b = blockIdx.y, n4 = n >> 2;
  const size_t off = (size_t)b * n;
  const int ti = table_index(t, b, tab.len);
  float a = 0.f, s = 0.f;
  if constexpr (OBJ == OBJ_V) { a = tab.a[ti]; s = tab.s[ti]; }
  float c = *gout * inv_count[b];
  if (tab.w) c = c * tab.w[ti];
  c = c / (float)gridDim.y;
  for (unsigned q0 = blockIdx.x * (TD_BLOCK * TD_QUADS) + threadIdx.x; q0 < n4; q0 += gridDim.x * (TD_BLOCK * TD_QUADS)) {
    const Trip sl = trip_slots(q0, n4);
    unsigned kb[TD_QUADS];
    float4 x0[TD_QUADS], nz[TD_QUADS], pr[TD_QUADS];
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) kb[k] = sl.in[k] ? known_bits<MASK>(m, b, n, sl.q[k] * 4u) : 0u;
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      const size_t at = off + (size_t)sl.q[k] * 4;
      x0[k] = zero, nz[k] = zero;
      if constexpr (USE_X0) x0[k] = sl.in[k] ? ld4(x_start + at) : zero;
      if constexpr (USE_Z) nz[k] = sl.in[k] ? ld4(noise + at) : zero;
      pr[k] = sl.in[k] ? ld4(out + at) : zero;
    }
    auto grad = [c](float z, float p) {
      if constexpr (L2) return (2.f * (p - z)) * c;
      else return z > p ? -c : (z < p ? c : 0.f);
    };
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      if (!sl.in[k]) continue;
      const float4 tg = obj_target4<OBJ>(x0[k], nz[k], a, s);
      float4 o;
      o.x = (kb[k] & 1u) ? 0.f : grad(tg.x, pr[k].x);
      o.y = (kb[k] & 2u) ? 0.f : grad(tg.y, pr[k].y);
      o.z = (kb[k] & 4u) ? 0.f : grad(tg.z, pr[k].z);
      o.w = (kb[k] & 8u) ? 0.f : grad(tg.w, pr[k].w);
      st4(dout + off + (size_t)sl.q[k] * 4, o);
    }
  }
}

// The one check of the geometry and the mask operands; -> MASK_* or a refusal.
int check_mask(const char* what, int batch, int64_t n, const unsigned char* frame_mask, const unsigned char* elem_mask, int frames,
               int64_t frame_elems, TrainMask& m) {
  if (batch <= 0 || batch > 65535 || n <= 0 || n % 4 != 0 || n >= ((int64_t)1 << 31))
    return lfdm_fail(LFDM_EINVAL, "%s: batch in [1, 65535] and n in (0, 2^31) with n %% 4 == 0 are needed, got batch = %d, n = %lld", what, batch, (long long)n);
  if (frame_mask && elem_mask)
    return lfdm_fail(LFDM_EINVAL, "%s: frame_mask and elem_mask exclude each other", what);
  m = TrainMask{nullptr, 0u, 0u};
  if (!frame_mask) {
    if (frames != 0 || frame_elems != 0)
      return lfdm_fail(LFDM_EINVAL, "%s: a frame split (frames = %d, frame_elems = %lld) needs frame_mask", what, frames, (long long)frame_elems);
    if (!elem_mask) return MASK_NONE;
    if (!lfdm_aligned<4>(elem_mask))
      return lfdm_fail(LFDM_EINVAL, "%s: elem_mask must be 4-byte aligned", what);
    m.mask = elem_mask;
    return MASK_ELEM;
  }
  if (frames <= 0 || frame_elems <= 0 || frame_elems % 4 != 0 || frames > n || frame_elems > n || n % ((int64_t)frames * frame_elems) != 0)
    return lfdm_fail(LFDM_EINVAL, "%s: n = %lld must be a multiple of frames * frame_elems = %d * %lld, frame_elems a multiple of 4", what, (long long)n,
                     frames, (long long)frame_elems);
  m = TrainMask{frame_mask, (unsigned)frames, (unsigned)frame_elems};
  return MASK_FRAME;
}

// f(MASK as an integral constant) for the checked form
template <class F>
void with_mask(int form, F&& f) {
  if (form == MASK_ELEM) f(std::integral_constant<int, MASK_ELEM>{});
  else if (form == MASK_FRAME) f(std::integral_constant<int, MASK_FRAME>{});
  else f(std::integral_constant<int, MASK_NONE>{});
}

template <class F>
void with_objective(int objective, F&& f) {
  if (objective == OBJ_V) f(std::integral_constant<int, OBJ_V>{});
  else if (objective == OBJ_X0) f(std::integral_constant<int, OBJ_X0>{});
  else f(std::integral_constant<int, OBJ_NOISE>{});
}

// The objective and the operands it needs (`with_r_m`: the forward's pred_x0 tables); 0 or a refusal.
int check_objective(const char* what, int objective, const float* x_start, const float* noise, const ObjTables& tab, bool with_r_m) {
  const bool ok = objective == OBJ_NOISE ? noise && (!with_r_m || (tab.r && tab.m))
                : objective == OBJ_X0    ? x_start != nullptr
                : objective == OBJ_V     ? x_start && noise && tab.a && tab.s
                                         : false;
  if (ok) return 0;
  if (objective != OBJ_NOISE && objective != OBJ_X0 && objective != OBJ_V)
    return lfdm_fail(LFDM_EINVAL, "%s: objective must be LFDM_OBJ_NOISE (0), LFDM_OBJ_X0 (1) or LFDM_OBJ_V (2), got %d", what, objective);
  return lfdm_fail(LFDM_EINVAL, "%s: objective %d lacks an operand - LFDM_OBJ_NOISE needs noise%s, LFDM_OBJ_X0 needs x_start, LFDM_OBJ_V needs "
                                "x_start, noise, a_tab and s_tab", what, objective, with_r_m ? ", r_tab and m_tab" : "");
}

}  // namespace

extern "C" int lfdm_train_qsample_f32(const float* x_start, const float* noise, const int64_t* t, const float* a_tab, const float* s_tab, int t_len,
                                      const unsigned char* frame_mask, const unsigned char* elem_mask, int frames, int64_t frame_elems,
                                      float* x_noisy, int batch, int64_t n, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x_start || !noise || !t || !a_tab || !s_tab || !x_noisy || t_len <= 0 || !lfdm_aligned16(x_start, noise, x_noisy) || !lfdm_aligned<8>(t))
    return lfdm_fail(LFDM_EINVAL, "%s", "train_qsample: x_start, noise, x_noisy (16-byte aligned), t, both tables and a table length > 0 are needed");
  TrainMask m;
  const int form = check_mask("train_qsample", batch, n, frame_mask, elem_mask, frames, frame_elems, m);
  if (form < 0) return form;
  const dim3 grid(sample_blocks(n), (unsigned)batch), block(TD_BLOCK);
  with_mask(form, [&](auto mask) {
    LFDM_LAUNCH(train_qsample_kernel<decltype(mask)::value>, grid, block, 0, stream, x_start, noise, t, a_tab, s_tab, t_len, m, x_noisy, (unsigned)n);
  });
  return lfdm_check_launch("train_qsample");
}

extern "C" size_t lfdm_masked_loss_ws_bytes(int batch, int64_t n) {
  if (batch <= 0 || n <= 0) return 0;
  return (size_t)batch * sample_blocks(n) * 2 * sizeof(unsigned long long);
}

extern "C" int lfdm_masked_loss_fwd_f32(const float* noise, const float* pred, const float* x_noisy, const int64_t* t, const float* r_tab,
                                        const float* m_tab, int t_len, const unsigned char* frame_mask, const unsigned char* elem_mask, int frames,
                                        int64_t frame_elems, int loss_type, float* loss, float* inv_count, float* pred_x0, int batch, int64_t n,
                                        void* ws, size_t ws_bytes, unsigned* ticket, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!noise || !pred || !x_noisy || !t || !r_tab || !m_tab || !loss || !inv_count || !pred_x0 || !ws || !ticket || t_len <= 0 ||
      !lfdm_aligned16(noise, pred, x_noisy, pred_x0) || !lfdm_aligned<8>(t, ws))
    return lfdm_fail(LFDM_EINVAL, "%s", "masked_loss_fwd: noise, pred, x_noisy, pred_x0 (16-byte aligned), t, both tables (length > 0), loss, inv_count, "
                                        "a workspace (8-byte aligned) and one zeroed ticket word are needed");
  if (loss_type != LFDM_LOSS_L1 && loss_type != LFDM_LOSS_L2)
    return lfdm_fail(LFDM_EINVAL, "masked_loss_fwd: loss_type must be LFDM_LOSS_L1 (0) or LFDM_LOSS_L2 (1), got %d", loss_type);
  TrainMask m;
  const int form = check_mask("masked_loss_fwd", batch, n, frame_mask, elem_mask, frames, frame_elems, m);
  if (form < 0) return form;
  if (ws_bytes < lfdm_masked_loss_ws_bytes(batch, n))
    return lfdm_fail(LFDM_EWORKSPACE, "masked_loss_fwd: workspace of %zu bytes, lfdm_masked_loss_ws_bytes asks for %zu", ws_bytes,
                     lfdm_masked_loss_ws_bytes(batch, n));
  const dim3 grid(sample_blocks(n), (unsigned)batch), block(TD_BLOCK);
  unsigned long long* part = reinterpret_cast<unsigned long long*>(ws);
  with_mask(form, [&](auto mask) {
    constexpr int M = decltype(mask)::value;
    if (loss_type == LFDM_LOSS_L2)
      LFDM_LAUNCH((masked_loss_fwd_kernel<M, true>), grid, block, 0, stream, noise, pred, x_noisy, t, r_tab, m_tab, t_len, m, loss, inv_count, pred_x0,
                  (unsigned)n, part, ticket);
    else
      LFDM_LAUNCH((masked_loss_fwd_kernel<M, false>), grid, block, 0, stream, noise, pred, x_noisy, t, r_tab, m_tab, t_len, m, loss, inv_count, pred_x0,
                  (unsigned)n, part, ticket);
  });
  return lfdm_check_launch("masked_loss_fwd");
}

extern "C" int lfdm_masked_loss_bwd_f32(const float* noise, const float* pred, const unsigned char* frame_mask, const unsigned char* elem_mask,
                                        int frames, int64_t frame_elems, int loss_type, const float* inv_count, const float* gout, float* dpred,
                                        int batch, int64_t n, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!noise || !pred || !inv_count || !gout || !dpred || !lfdm_aligned16(noise, pred, dpred))
    return lfdm_fail(LFDM_EINVAL, "%s", "masked_loss_bwd: noise, pred, dpred (16-byte aligned), inv_count and gout are needed");
  if (loss_type != LFDM_LOSS_L1 && loss_type != LFDM_LOSS_L2)
    return lfdm_fail(LFDM_EINVAL, "masked_loss_bwd: loss_type must be LFDM_LOSS_L1 (0) or LFDM_LOSS_L2 (1), got %d", loss_type);
  TrainMask m;
  const int form = check_mask("masked_loss_bwd", batch, n, frame_mask, elem_mask, frames, frame_elems, m);
  if (form < 0) return form;
  const dim3 grid(sample_blocks(n), (unsigned)batch), block(TD_BLOCK);
  with_mask(form, [&](auto mask) {
    constexpr int M = decltype(mask)::value;
    if (loss_type == LFDM_LOSS_L2)
      LFDM_LAUNCH((masked_loss_bwd_kernel<M, true>), grid, block, 0, stream, noise, pred, m, inv_count, gout, dpred, (unsigned)n);
    else
      LFDM_LAUNCH((masked_loss_bwd_kernel<M, false>), grid, block, 0, stream, noise, pred, m, inv_count, gout, dpred, (unsigned)n);
  });
  return lfdm_check_launch("masked_loss_bwd");
}

extern "C" int lfdm_objective_loss_fwd_f32(int objective, const float* x_start, const float* noise, const float* out, const float* x_noisy,
                                           const int64_t* t, const float* a_tab, const float* s_tab, const float* r_tab, const float* m_tab,
                                           const float* w_tab, int t_len, const unsigned char* frame_mask, const unsigned char* elem_mask,
                                           int frames, int64_t frame_elems, int loss_type, float* loss, float* inv_count, float* sample_loss,
                                           float* pred_x0, int batch, int64_t n, void* ws, size_t ws_bytes, unsigned* ticket,
                                           lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!out || !x_noisy || !t || !loss || !inv_count || !sample_loss || !pred_x0 || !ws || !ticket || t_len <= 0 ||
      !lfdm_aligned16(x_start, noise, out, x_noisy, pred_x0) || !lfdm_aligned<8>(t, ws))
    return lfdm_fail(LFDM_EINVAL, "%s", "objective_loss_fwd: out, x_noisy, pred_x0 (16-byte aligned, as x_start and noise where given), t, a table "
                                        "length > 0, loss, inv_count, sample_loss, a workspace (8-byte aligned) and one zeroed ticket word are needed");
  const ObjTables tab{a_tab, s_tab, r_tab, m_tab, w_tab, t_len};
  if (const int rc = check_objective("objective_loss_fwd", objective, x_start, noise, tab, true)) return rc;
  if (loss_type != LFDM_LOSS_L1 && loss_type != LFDM_LOSS_L2)
    return lfdm_fail(LFDM_EINVAL, "objective_loss_fwd: loss_type must be LFDM_LOSS_L1 (0) or LFDM_LOSS_L2 (1), got %d", loss_type);
  TrainMask m;
  const int form = check_mask("objective_loss_fwd", batch, n, frame_mask, elem_mask, frames, frame_elems, m);
  if (form < 0) return form;
  if (ws_bytes < lfdm_masked_loss_ws_bytes(batch, n))
    return lfdm_fail(LFDM_EWORKSPACE, "objective_loss_fwd: workspace of %zu bytes, lfdm_masked_loss_ws_bytes asks for %zu", ws_bytes,
                     lfdm_masked_loss_ws_bytes(batch, n));
  const dim3 grid(sample_blocks(n), (unsigned)batch), block(TD_BLOCK);
  unsigned long long* part = reinterpret_cast<unsigned long long*>(ws);
  with_objective(objective, [&](auto obj) {
    with_mask(form, [&](auto mask) {
      constexpr int O = decltype(obj)::value, M = decltype(mask)::value;
      if (loss_type == LFDM_LOSS_L2)
        LFDM_LAUNCH((objective_loss_fwd_kernel<O, M, true>), grid, block, 0, stream, x_start, noise, out, x_noisy, t, tab, m, loss, inv_count,
                    sample_loss, pred_x0, (unsigned)n, part, ticket);
      else
        LFDM_LAUNCH((objective_loss_fwd_kernel<O, M, false>), grid, block, 0, stream, x_start, noise, out, x_noisy, t, tab, m, loss, inv_count,
                    sample_loss, pred_x0, (unsigned)n, part, ticket);
    });
  });
  return lfdm_check_launch("objective_loss_fwd");
}

extern "C" int lfdm_objective_loss_bwd_f32(int objective, const float* x_start, const float* noise, const float* out, const int64_t* t,
                                           const float* a_tab, const float* s_tab, const float* w_tab, int t_len,
                                           const unsigned char* frame_mask, const unsigned char* elem_mask, int frames, int64_t frame_elems,
                                           int loss_type, const float* inv_count, const float* gout, float* dout, int batch, int64_t n,
                                           lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!out || !t || !inv_count || !gout || !dout || t_len <= 0 || !lfdm_aligned16(x_start, noise, out, dout) || !lfdm_aligned<8>(t))
    return lfdm_fail(LFDM_EINVAL, "%s", "objective_loss_bwd: out, dout (16-byte aligned, as x_start and noise where given), t, a table length > 0, "
                                        "inv_count and gout are needed");
  const ObjTables tab{a_tab, s_tab, nullptr, nullptr, w_tab, t_len};
  if (const int rc = check_objective("objective_loss_bwd", objective, x_start, noise, tab, false)) return rc;
  if (loss_type != LFDM_LOSS_L1 && loss_type != LFDM_LOSS_L2)
    return lfdm_fail(LFDM_EINVAL, "objective_loss_bwd: loss_type must be LFDM_LOSS_L1 (0) or LFDM_LOSS_L2 (1), got %d", loss_type);
  TrainMask m;
  const int form = check_mask("objective_loss_bwd", batch, n, frame_mask, elem_mask, frames, frame_elems, m);
  if (form < 0) return form;
  const dim3 grid(sample_blocks(n), (unsigned)batch), block(TD_BLOCK);
  with_objective(objective, [&](auto obj) {
    with_mask(form, [&](auto mask) {
      constexpr int O = decltype(obj)::value, M = decltype(mask)::value;
      if (loss_type == LFDM_LOSS_L2)
        LFDM_LAUNCH((objective_loss_bwd_kernel<O, M, true>), grid, block, 0, stream, x_start, noise, out, t, tab, m, inv_count, gout, dout, (unsigned)n);
      else
        LFDM_LAUNCH((objective_loss_bwd_kernel<O, M, false>), grid, block, 0, stream, x_start, noise, out, t, tab, m, inv_count, gout, dout, (unsigned)n);
    });
  });
  return lfdm_check_launch("objective_loss_bwd");
}
