// Streaming softmax attention over 65 .. 256 tokens, forward and backward (include/lfdm_hip.h, "long attention").
//
// attention.hip / train_attention.hip hold a whole sequence in one wavefront's registers or LDS tiles and stop at 64 tokens.  The kernels
// here keep only a BLOCK of the sequence resident and stream the other side from global memory in tiles of 16 tokens, flash style.  A
// (sequence, head)'s K and V are at most 256 x 32 x 4 B x 2 = 64 KB and the waves that share them are neighbours in the grid, so the
// streamed tiles come from L1 / L2.  Geometry, register layouts and arithmetic are attention_kernel's: 8 heads x 32 features, qkv rows of
// 768, out rows of 256, feature slot k = 8*lq + s (a Q / K fragment = two 16-byte loads), scale 32^-0.5 and rotary applied in registers,
// bias added vectorised when L % 4 == 0, keys >= L masked to -3e38, query rows >= L never stored, fast_exp / fast_rcp.
//
// SOFTMAX ACROSS KEY TILES: TWO SWEEPS (scheme (b) of the design note).  Sweep 1 computes S^T = K Q^T alone and takes the exact row
// maximum; sweep 2 recomputes the scores, exponentiates against the FINAL maximum, sums and accumulates P V.  Why not the online running
// maximum: its per-tile rescale factor of O lives in another lane than O (statistics: lane = query; O: lane = feature), i.e. a cross-lane
// move per tile per query tile, and the summation order of a row would depend on where its maximum sits.  Two sweeps cost 1.5x the MFMAs
// (24 instead of 16 per 16x16 tile pair) on a kernel whose MFMA pipe is far from busy, need ONE cross-lane move per query block (the
// reciprocal of the sum, through 128 bytes of LDS) and sum every row in the same fixed order as attention_kernel does.
//
// FORWARD  lfdm_attention_long_cl_f32: work unit = (sequence, head, block of 32 queries), one wavefront (= one 64-thread workgroup) each.
//   Optionally writes the row maximum and the row sum per (sequence, head, query).
// BACKWARD lfdm_attention_long_bwd_cl_f32: the two-phase flash form, P and dP recomputed from qkv, nothing but qkv saved.
//   Phase Q  - a wave owns 32 queries and sweeps the key tiles three times: (1) row maximum, (2) row sum and D_i = sum_j P_ij dP_ij
//              (= rowsum(dO o O), without needing O), (3) dS_ij = P_ij (dP_ij - D_i), dQ_i += dS_ij K_j.  Writes dq (rotary undone, 32^-0.5
//              re-applied) and the row statistics (max, 1/sum, D) for phase KV.
//   Phase KV - a wave owns (head, block of 16 keys) and walks the query tiles of its sequences: dV_j += P_ij^T dO_i, dK_j += dS_ij^T Q_i,
//              and keeps the bias gradient of its 16 key columns x L query rows in lane-private LDS words over ALL the sequences it serves (grid-stride
//              over sequences; the stride leaves (head, key block) fixed).  Writes dk (rotary undone), dv and one bias partial per wave.
//   Every output element has exactly one owner, there is no atomic anywhere, the partials are added by lfdm_sum_leading_f32 in a fixed
//   order: the result is bit-identical from run to run.
//   WORKSPACE (lfdm_attention_long_bwd_ws_bytes): row statistics 3 * nseq * 8 * LS floats (LS = L rounded up to 16; what a forward that saved
//   its statistics would hold too) + bias partials G * 8 * L * L floats with G = min(nseq, max(1, 2048 / (8 * ceil(L / 16)))) sequence
//   groups: at most 2048 waves, i.e. <= 16 groups = 32 MB at L = 256, <= 32 groups = 16 MB at L = 128 - independent of batch * hw.
//
// FOOTPRINTS (hipcc, ROCm 7.2, -O3, gfx950, the compiler's resource report): forward 96 VGPRs + 128 B of LDS = 5 waves
// per SIMD; phase Q 122 VGPRs, no LDS = 4; phase KV 160 VGPRs, no LDS = 3 without a bias, 190 VGPRs + 16 KB of LDS per wave (the bias-gradient
// tile) = 2 with one (10 waves per CU by LDS).  No spills, no AGPRs - against the one wave per SIMD on 512 VGPRs of attention_bwd_kernel.
// No inline-assembly load pipeline in this version: the other waves of the SIMD hide the streamed loads.
#include <stdlib.h>
#include "attn_core.h"
#include "../../include/lfdm_hip.h"

namespace {

constexpr int L_MIN = 65, L_MAX = 256;
constexpr int NQ = 2;                   // query tiles of 16 per wave (forward, phase Q)
constexpr int MAX_WAVES_KV = 2048;      // launch-size cap of phase KV

// f[s] = src[token t][8*lq + s] * scale (zeros for t >= L), rotated by the token's rotary factors if rot_cos: the A / B operand of a
// contraction over the 32 features for the token of lane & 15.  src points at column 0 of the head's q, k, v or dout block of row 0.
__device__ __forceinline__ void load_frag(float f[8], const float* src, int ld, int64_t row0, int64_t tstride, int t, int L, int lq,
                                          float scale, const float* rot_cos, const float* rot_sin) {
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  if (t < L) {
    const float* p = src + (row0 + (int64_t)t * tstride) * ld + 8 * lq;
    a = *reinterpret_cast<const float4*>(p);
    b = *reinterpret_cast<const float4*>(p + 4);
  }
  f[0] = a.x * scale; f[1] = a.y * scale; f[2] = a.z * scale; f[3] = a.w * scale;
  f[4] = b.x * scale; f[5] = b.y * scale; f[6] = b.z * scale; f[7] = b.w * scale;
  if (rot_cos && t < L) {
#pragma unroll
    for (int pr = 0; pr < 4; ++pr) {
      const float c = rot_cos[t * 16 + 4 * lq + pr], sn = rot_sin[t * 16 + 4 * lq + pr];
      rot_pair(f[2 * pr], f[2 * pr + 1], c, sn);
    }
  }
}

// b[hh][r] = src[token t0 + 4*lq + r][16*hh + l15] * scale (zeros for tokens >= L), rotated if rot_cos: the B operand of a contraction over
// tokens.  The rotation partner of feature d is d ^ 1 = the neighbouring lane.  Every lane executes the shuffles.
__device__ __forceinline__ void load_rows(float b[2][4], const float* src, int ld, int64_t row0, int64_t tstride, int t0, int L, int l15,
                                          int lq, float scale, const float* rot_cos, const float* rot_sin) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int t = t0 + 4 * lq + r;
    float v0 = 0.f, v1 = 0.f;
    if (t < L) {
      const float* p = src + (row0 + (int64_t)t * tstride) * ld;
      v0 = p[l15] * scale;
      v1 = p[16 + l15] * scale;
    }
    if (rot_cos) {
      const float o0 = __shfl_xor(v0, 1), o1 = __shfl_xor(v1, 1);
      const int tt = t < L ? t : 0;
      const float c0 = rot_cos[tt * 16 + (l15 >> 1)], s0 = rot_sin[tt * 16 + (l15 >> 1)];
      const float c1 = rot_cos[tt * 16 + 8 + (l15 >> 1)], s1 = rot_sin[tt * 16 + 8 + (l15 >> 1)];
      if ((l15 & 1) == 0) {          // x' = x c - y s
        v0 = v0 * c0 - o0 * s0;
        v1 = v1 * c1 - o1 * s1;
      } else {                       // y' = y c + x s
        v0 = v0 * c0 + o0 * s0;
        v1 = v1 * c1 + o1 * s1;
      }
    }
    b[0][r] = v0;
    b[1][r] = v1;
  }
}

// the gradient of a rotated row (lane = feature 16*hh + l15) taken back through the rotation: R^T
__device__ __forceinline__ float unrotate(float g, int t, int L, int hh, int l15, const float* rot_cos, const float* rot_sin) {
  if (!rot_cos) return g;
  const float go = __shfl_xor(g, 1);
  const int tt = t < L ? t : 0;
  const float c = rot_cos[tt * 16 + ((16 * hh + l15) >> 1)], sn = rot_sin[tt * 16 + ((16 * hh + l15) >> 1)];
  return (l15 & 1) == 0 ? g * c + go * sn : g * c - go * sn;      // dx = gx c + gy s ; dy = gy c - gx s
}

// Transposed scores of one (key tile, query tile): lane = query qt, registers = keys key0 + r.  Bias added, keys >= L masked to -3e38
// exactly as attention_kernel does.
__device__ __forceinline__ f32x4 scores_t(const float kf[8], const float qf[8], const float* bias, bool bias_vec, int head, int qt,
                                          int key0, int L) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 8; ++s) acc = mfma_16x16x4(kf[s], qf[s], acc);
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if (bias && qt < L && key0 < L) {
    const float* bp = bias + ((int64_t)head * L + qt) * L + key0;
    if (bias_vec) {
      const float4 b4 = *reinterpret_cast<const float4*>(bp);
      bv[0] = b4.x; bv[1] = b4.y; bv[2] = b4.z; bv[3] = b4.w;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) bv[r] = (key0 + r < L) ? bp[r] : 0.f;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = (key0 + r >= L) ? -3.0e38f : acc[r] + bv[r];
  return acc;
}

// ---------------- forward ----------------
// grid = nseq * 8 * nqb workgroups of one wavefront; unit = (seq * 8 + head) * nqb + query block.
// stats (optional): [(seq * 8 + head)][2][L] = row maximum | row sum of exp(s - max).
__global__ __launch_bounds__(64) void attention_long_kernel(const float* __restrict__ qkv, float* __restrict__ out, int batch, int frames,
                                                            int hw, int mode, const float* __restrict__ bias,
                                                            const float* __restrict__ rot_cos, const float* __restrict__ rot_sin,
                                                            float* __restrict__ stats, int nqb) {
  __shared__ float s_inv[NQ * 16];
  const int lane = threadIdx.x & 63;
  const int l15 = lane & 15, lq = lane >> 4;
  const int L = mode == 0 ? frames : hw;
  const int nkt = (L + 15) >> 4;
  const int64_t unit = blockIdx.x;
  const int64_t sh = unit / nqb;
  const int q0 = (int)(unit - sh * nqb) * (16 * NQ);
  const int64_t seq = sh / HEADS;
  const int head = (int)(sh - seq * HEADS);
  int64_t row0, tstride;
  seq_rows(seq, mode, frames, hw, row0, tstride);
  const float* qbase = qkv + head * DH;
  const float* kbase = qbase + OUT_LD;
  const float* vbase = qbase + 2 * OUT_LD;
  const bool bias_vec = bias && (L % 4 == 0) && ((((uintptr_t)bias) & 15) == 0);

  float qf[NQ][8];
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti) load_frag(qf[ti], qbase, QKV_LD, row0, tstride, q0 + 16 * ti + l15, L, lq, ATT_SCALE, rot_cos, rot_sin);

  // ---- sweep 1: exact row maxima ----
  float m[NQ];
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti) m[ti] = -3.0e38f;
  for (int tj = 0; tj < nkt; ++tj) {
    float kf[8];
    load_frag(kf, kbase, QKV_LD, row0, tstride, 16 * tj + l15, L, lq, 1.f, rot_cos, rot_sin);
#pragma unroll
    for (int ti = 0; ti < NQ; ++ti) {
      const f32x4 st = scores_t(kf, qf[ti], bias, bias_vec, head, q0 + 16 * ti + l15, 16 * tj + 4 * lq, L);
      m[ti] = fmaxf(m[ti], fmaxf(fmaxf(st[0], st[1]), fmaxf(st[2], st[3])));
    }
  }
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti) {
    m[ti] = fmaxf(m[ti], __shfl_xor(m[ti], 16));
    m[ti] = fmaxf(m[ti], __shfl_xor(m[ti], 32));
  }

  // ---- sweep 2: exp against the final maximum, row sums, O = P V (normalised at the end) ----
  float sum[NQ];
  f32x4 o[NQ][2];
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti) {
    sum[ti] = 0.f;
    o[ti][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    o[ti][1] = o[ti][0];
  }
  for (int tj = 0; tj < nkt; ++tj) {
    float kf[8], vf[2][4];
    load_frag(kf, kbase, QKV_LD, row0, tstride, 16 * tj + l15, L, lq, 1.f, rot_cos, rot_sin);
    load_rows(vf, vbase, QKV_LD, row0, tstride, 16 * tj, L, l15, lq, 1.f, nullptr, nullptr);
#pragma unroll
    for (int ti = 0; ti < NQ; ++ti) {
      const f32x4 st = scores_t(kf, qf[ti], bias, bias_vec, head, q0 + 16 * ti + l15, 16 * tj + 4 * lq, L);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = (16 * tj + 4 * lq + r) < L ? fast_exp(st[r] - m[ti]) : 0.f;
        sum[ti] += e;
        o[ti][0] = mfma_16x16x4(e, vf[0][r], o[ti][0]);
        o[ti][1] = mfma_16x16x4(e, vf[1][r], o[ti][1]);
      }
    }
  }
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti) {
    sum[ti] += __shfl_xor(sum[ti], 16);
    sum[ti] += __shfl_xor(sum[ti], 32);
    const int qt = q0 + 16 * ti + l15;
    if (lq == 0) {
      s_inv[16 * ti + l15] = fast_rcp(sum[ti]);      // one reciprocal per query
      if (stats && qt < L) {
        stats[(sh * 2 + 0) * L + qt] = m[ti];
        stats[(sh * 2 + 1) * L + qt] = sum[ti];
      }
    }
  }
  lfdm_wave_lds_sync();      // the statistics live in lane = query, O in lane = feature: the one cross-lane move of the kernel
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = q0 + 16 * ti + 4 * lq + r;
      const float inv = s_inv[16 * ti + 4 * lq + r];
      if (t < L) {
        float* dst = out + (row0 + (int64_t)t * tstride) * OUT_LD + head * DH;
        dst[l15] = o[ti][0][r] * inv;
        dst[16 + l15] = o[ti][1][r] * inv;
      }
    }
}

// ---------------- backward, phase Q ----------------
// grid as the forward.  rstat: [(seq * 8 + head)][3][LS] = row maximum | 1 / row sum | D, zeros for queries >= L.
__global__ __launch_bounds__(64) void attention_long_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                  float* __restrict__ dqkv, int batch, int frames, int hw, int mode,
                                                                  const float* __restrict__ bias, const float* __restrict__ rot_cos,
                                                                  const float* __restrict__ rot_sin, float* __restrict__ rstat, int nqb) {
  const int lane = threadIdx.x & 63;
  const int l15 = lane & 15, lq = lane >> 4;
  const int L = mode == 0 ? frames : hw;
  const int nkt = (L + 15) >> 4;
  const int LS = nkt * 16;
  const int64_t unit = blockIdx.x;
  const int64_t sh = unit / nqb;
  const int q0 = (int)(unit - sh * nqb) * (16 * NQ);
  const int64_t seq = sh / HEADS;
  const int head = (int)(sh - seq * HEADS);
  int64_t row0, tstride;
  seq_rows(seq, mode, frames, hw, row0, tstride);
  const float* qbase = qkv + head * DH;
  const float* kbase = qbase + OUT_LD;
  const float* vbase = qbase + 2 * OUT_LD;
  const float* gbase = dout + head * DH;
  const bool bias_vec = bias && (L % 4 == 0) && ((((uintptr_t)bias) & 15) == 0);

  float qf[NQ][8], gf[NQ][8];
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti) {
    load_frag(qf[ti], qbase, QKV_LD, row0, tstride, q0 + 16 * ti + l15, L, lq, ATT_SCALE, rot_cos, rot_sin);
    load_frag(gf[ti], gbase, OUT_LD, row0, tstride, q0 + 16 * ti + l15, L, lq, 1.f, nullptr, nullptr);
  }

  // ---- sweep 1: row maxima ----
  float m[NQ];
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti) m[ti] = -3.0e38f;
  for (int tj = 0; tj < nkt; ++tj) {
    float kf[8];
    load_frag(kf, kbase, QKV_LD, row0, tstride, 16 * tj + l15, L, lq, 1.f, rot_cos, rot_sin);
#pragma unroll
    for (int ti = 0; ti < NQ; ++ti) {
      const f32x4 st = scores_t(kf, qf[ti], bias, bias_vec, head, q0 + 16 * ti + l15, 16 * tj + 4 * lq, L);
      m[ti] = fmaxf(m[ti], fmaxf(fmaxf(st[0], st[1]), fmaxf(st[2], st[3])));
    }
  }
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti) {
    m[ti] = fmaxf(m[ti], __shfl_xor(m[ti], 16));
    m[ti] = fmaxf(m[ti], __shfl_xor(m[ti], 32));
  }

  // ---- sweep 2: row sums and D = sum_j P dP (dP^T = V dO^T in the scores' layout) ----
  float inv[NQ], dd[NQ];
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti) inv[ti] = dd[ti] = 0.f;
  for (int tj = 0; tj < nkt; ++tj) {
    float kf[8], vr[8];
    load_frag(kf, kbase, QKV_LD, row0, tstride, 16 * tj + l15, L, lq, 1.f, rot_cos, rot_sin);
    load_frag(vr, vbase, QKV_LD, row0, tstride, 16 * tj + l15, L, lq, 1.f, nullptr, nullptr);
#pragma unroll
    for (int ti = 0; ti < NQ; ++ti) {
      const f32x4 st = scores_t(kf, qf[ti], bias, bias_vec, head, q0 + 16 * ti + l15, 16 * tj + 4 * lq, L);
      f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 8; ++s) dp = mfma_16x16x4(vr[s], gf[ti][s], dp);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = (16 * tj + 4 * lq + r) < L ? fast_exp(st[r] - m[ti]) : 0.f;
        inv[ti] += e;
        dd[ti] += e * dp[r];
      }
    }
  }
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti) {
    inv[ti] += __shfl_xor(inv[ti], 16);
    inv[ti] += __shfl_xor(inv[ti], 32);
    dd[ti] += __shfl_xor(dd[ti], 16);
    dd[ti] += __shfl_xor(dd[ti], 32);
    inv[ti] = fast_rcp(inv[ti]);
    dd[ti] *= inv[ti];
    const int qt = q0 + 16 * ti + l15;
    if (lq == 0 && qt < LS) {
      const bool ok = qt < L;
      rstat[(sh * 3 + 0) * LS + qt] = ok ? m[ti] : 0.f;
      rstat[(sh * 3 + 1) * LS + qt] = ok ? inv[ti] : 0.f;
      rstat[(sh * 3 + 2) * LS + qt] = ok ? dd[ti] : 0.f;
    }
  }

  // ---- sweep 3: dS^T = P^T o (dP^T - D) is the A operand of dQ = dS K ----
  f32x4 dq[NQ][2];
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti) {
    dq[ti][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    dq[ti][1] = dq[ti][0];
  }
  for (int tj = 0; tj < nkt; ++tj) {
    float kf[8], vr[8], kb[2][4];
    load_frag(kf, kbase, QKV_LD, row0, tstride, 16 * tj + l15, L, lq, 1.f, rot_cos, rot_sin);
    load_frag(vr, vbase, QKV_LD, row0, tstride, 16 * tj + l15, L, lq, 1.f, nullptr, nullptr);
    load_rows(kb, kbase, QKV_LD, row0, tstride, 16 * tj, L, l15, lq, 1.f, rot_cos, rot_sin);
#pragma unroll
    for (int ti = 0; ti < NQ; ++ti) {
      const int qt = q0 + 16 * ti + l15;
      const f32x4 st = scores_t(kf, qf[ti], bias, bias_vec, head, qt, 16 * tj + 4 * lq, L);
      f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 8; ++s) dp = mfma_16x16x4(vr[s], gf[ti][s], dp);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = qt < L && (16 * tj + 4 * lq + r) < L;
        const float p = ok ? fast_exp(st[r] - m[ti]) * inv[ti] : 0.f;
        const float ds = ok ? p * (dp[r] - dd[ti]) : 0.f;
        dq[ti][0] = mfma_16x16x4(ds, kb[0][r], dq[ti][0]);
        dq[ti][1] = mfma_16x16x4(ds, kb[1][r], dq[ti][1]);
      }
    }
  }
#pragma unroll
  for (int ti = 0; ti < NQ; ++ti)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = q0 + 16 * ti + 4 * lq + r;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const float g = unrotate(dq[ti][hh][r], t, L, hh, l15, rot_cos, rot_sin);
        if (t < L) dqkv[(row0 + (int64_t)t * tstride) * QKV_LD + head * DH + 16 * hh + l15] = g * ATT_SCALE;
      }
    }
}

// ---------------- backward, phase KV ----------------
// grid = G * 8 * nkt workgroups of one wavefront: wave w = (g * 8 + head) * nkt + key block serves the sequences g, g + G, ...
// Scores here are NOT transposed: lane = key k0 + l15, registers = queries 16*i + 4*lq + r, which is the A operand layout of both
// token contractions (P^T dO and dS^T Q).  BIAS: the wave's bias-gradient tile (L queries x 16 keys, up to 64 values per lane) is kept in
// LDS words that only their own lane ever touches - lane-private scratch, no synchronisation.  (In registers, with the query loop unrolled
// for static indices, hipcc hoisted the loads of all sixteen tiles and spilled 250 VGPRs at one wave per SIMD.)
template <bool BIAS>
__global__ __launch_bounds__(64) void attention_long_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                   float* __restrict__ dqkv, int batch, int frames, int hw, int mode,
                                                                   const float* __restrict__ bias, const float* __restrict__ rot_cos,
                                                                   const float* __restrict__ rot_sin, const float* __restrict__ rstat,
                                                                   float* __restrict__ dbias_part, int groups) {
  const int lane = threadIdx.x & 63;
  const int l15 = lane & 15, lq = lane >> 4;
  const int L = mode == 0 ? frames : hw;
  const int nkt = (L + 15) >> 4;
  const int LS = nkt * 16;
  const int64_t nseq = mode == 0 ? (int64_t)batch * hw : (int64_t)batch * frames;
  const int w = blockIdx.x;
  const int kblk = w % nkt;
  const int head = (w / nkt) % HEADS;
  const int g = w / (nkt * HEADS);
  const int k0 = kblk * 16;
  const int key = k0 + l15;
  const float* qbase = qkv + head * DH;
  const float* kbase = qbase + OUT_LD;
  const float* vbase = qbase + 2 * OUT_LD;
  const float* gbase = dout + head * DH;

  __shared__ float s_db[BIAS ? (L_MAX / 16) * 4 * 64 : 64];      // [query tile][r][lane]
  if (BIAS)
    for (int i = 0; i < nkt * 4; ++i) s_db[i * 64 + lane] = 0.f;

  for (int64_t seq = g; seq < nseq; seq += groups) {
    int64_t row0, tstride;
    seq_rows(seq, mode, frames, hw, row0, tstride);
    const float* st_m = rstat + ((seq * HEADS + head) * 3) * LS;
    float kf[8], vr[8];
    load_frag(kf, kbase, QKV_LD, row0, tstride, key, L, lq, 1.f, rot_cos, rot_sin);
    load_frag(vr, vbase, QKV_LD, row0, tstride, key, L, lq, 1.f, nullptr, nullptr);
    f32x4 dk[2], dv[2];
    dk[0] = dk[1] = dv[0] = dv[1] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int i = 0; i < nkt; ++i) {
      float qf[8], gf[8], qb[2][4], gb[2][4];
      load_frag(qf, qbase, QKV_LD, row0, tstride, 16 * i + l15, L, lq, ATT_SCALE, rot_cos, rot_sin);
      load_frag(gf, gbase, OUT_LD, row0, tstride, 16 * i + l15, L, lq, 1.f, nullptr, nullptr);
      load_rows(qb, qbase, QKV_LD, row0, tstride, 16 * i, L, l15, lq, ATT_SCALE, rot_cos, rot_sin);
      load_rows(gb, gbase, OUT_LD, row0, tstride, 16 * i, L, l15, lq, 1.f, nullptr, nullptr);
      const float4 m4 = *reinterpret_cast<const float4*>(st_m + 16 * i + 4 * lq);
      const float4 i4 = *reinterpret_cast<const float4*>(st_m + LS + 16 * i + 4 * lq);
      const float4 d4 = *reinterpret_cast<const float4*>(st_m + 2 * LS + 16 * i + 4 * lq);
      const float rm[4] = {m4.x, m4.y, m4.z, m4.w}, ri[4] = {i4.x, i4.y, i4.z, i4.w}, rd[4] = {d4.x, d4.y, d4.z, d4.w};
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = s;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 16 * i + 4 * lq + r;
        if (BIAS && q < L && key < L) s[r] = bias[((int64_t)head * L + q) * L + key];
      }
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        s = mfma_16x16x4(qf[x], kf[x], s);
        dp = mfma_16x16x4(gf[x], vr[x], dp);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = (16 * i + 4 * lq + r) < L && key < L;
        const float p = ok ? fast_exp(s[r] - rm[r]) * ri[r] : 0.f;
        const float ds = ok ? p * (dp[r] - rd[r]) : 0.f;
        dv[0] = mfma_16x16x4(p, gb[0][r], dv[0]);
        dv[1] = mfma_16x16x4(p, gb[1][r], dv[1]);
        dk[0] = mfma_16x16x4(ds, qb[0][r], dk[0]);
        dk[1] = mfma_16x16x4(ds, qb[1][r], dk[1]);
        if (BIAS) s_db[(4 * i + r) * 64 + lane] += ds;
      }
    }

#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = k0 + 4 * lq + r;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const float gk = unrotate(dk[hh][r], t, L, hh, l15, rot_cos, rot_sin);
        if (t < L) {
          float* dst = dqkv + (row0 + (int64_t)t * tstride) * QKV_LD + OUT_LD + head * DH + 16 * hh + l15;
          dst[0] = gk;
          dst[OUT_LD] = dv[hh][r];
        }
      }
    }
  }

  if (BIAS) {
    // partial [g][head][query][key]: this wave owns the 16 key columns of its block
    float* dst = dbias_part + ((int64_t)g * HEADS + head) * L * L;
    for (int i = 0; i < nkt; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = 16 * i + 4 * lq + r;
        if (q < L && key < L) dst[(int64_t)q * L + key] = s_db[(4 * i + r) * 64 + lane];
      }
  }
}

int long_kv_groups(int64_t nseq, int L) {
  const int nkt = (L + 15) / 16;
  int g = MAX_WAVES_KV / (HEADS * nkt);
  if (g < 1) g = 1;
  return nseq < g ? (int)nseq : g;
}

size_t long_stat_floats(int64_t nseq, int L) { return (size_t)nseq * HEADS * 3 * (size_t)(((L + 15) / 16) * 16); }

bool long_shape_ok(int batch, int frames, int hw, int mode) {
  if (batch <= 0 || frames <= 0 || hw <= 0 || (mode != 0 && mode != 1)) return false;
  const int L = mode == 0 ? frames : hw;
  if (L < L_MIN || L > L_MAX) return false;
  const int64_t nseq = mode == 0 ? (int64_t)batch * hw : (int64_t)batch * frames;
  return nseq * HEADS * ((L + 16 * NQ - 1) / (16 * NQ)) < ((int64_t)1 << 31);      // one workgroup per (sequence, head, query block)
}

}  // namespace

extern "C" int lfdm_attention_long_cl_f32(const float* qkv, float* out, int batch, int frames, int hw, int mode, const float* bias,
                                          const float* rot_cos, const float* rot_sin, float* stats, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!qkv || !out || !long_shape_ok(batch, frames, hw, mode) || ((rot_cos == nullptr) != (rot_sin == nullptr))) {
    return lfdm_fail(LFDM_EINVAL, "attention_long: unsupported shape (sequence length must be 65 .. 256; up to 64 tokens belong to lfdm_attention_cl_f32)");
  }
  const int L = mode == 0 ? frames : hw;
  const int64_t nseq = mode == 0 ? (int64_t)batch * hw : (int64_t)batch * frames;
  const int nqb = (L + 16 * NQ - 1) / (16 * NQ);
  const dim3 grid((unsigned)(nseq * HEADS * nqb)), block(64);
  LFDM_LAUNCH(attention_long_kernel, grid, block, 0, stream, qkv, out, batch, frames, hw, mode, bias, rot_cos, rot_sin, stats, nqb);
  return lfdm_check_launch("attention_long");
}

extern "C" size_t lfdm_attention_long_bwd_ws_bytes(int batch, int frames, int hw, int mode) {
  if (!long_shape_ok(batch, frames, hw, mode)) return 0;
  const int L = mode == 0 ? frames : hw;
  const int64_t nseq = mode == 0 ? (int64_t)batch * hw : (int64_t)batch * frames;
  return (long_stat_floats(nseq, L) + (size_t)long_kv_groups(nseq, L) * HEADS * L * L) * sizeof(float);
}

extern "C" int lfdm_attention_long_bwd_cl_f32(const float* qkv, const float* dout, float* dqkv, int batch, int frames, int hw, int mode,
                                              const float* bias, const float* rot_cos, const float* rot_sin, float* dbias, void* ws,
                                              size_t ws_bytes, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!qkv || !dout || !dqkv || !long_shape_ok(batch, frames, hw, mode) || ((rot_cos == nullptr) != (rot_sin == nullptr)) ||
      ((bias == nullptr) != (dbias == nullptr))) {
    return lfdm_fail(LFDM_EINVAL, "attention_long_bwd: unsupported arguments (sequence length must be 65 .. 256; dbias iff bias)");
  }
  if (!ws || !lfdm_aligned16(ws) || ws_bytes < lfdm_attention_long_bwd_ws_bytes(batch, frames, hw, mode))
    return lfdm_fail(LFDM_EWORKSPACE, "attention_long_bwd: workspace too small or not 16-byte aligned");
  const int L = mode == 0 ? frames : hw;
  const int64_t nseq = mode == 0 ? (int64_t)batch * hw : (int64_t)batch * frames;
  const int nqb = (L + 16 * NQ - 1) / (16 * NQ), nkt = (L + 15) / 16;
  const int groups = long_kv_groups(nseq, L);
  float* rstat = (float*)ws;
  float* part = rstat + long_stat_floats(nseq, L);
  LFDM_LAUNCH(attention_long_bwd_q_kernel, dim3((unsigned)(nseq * HEADS * nqb)), dim3(64), 0, stream, qkv, dout, dqkv, batch, frames, hw,
              mode, bias, rot_cos, rot_sin, rstat, nqb);
  const dim3 grid((unsigned)(groups * HEADS * nkt)), block(64);
  if (bias) LFDM_LAUNCH((attention_long_bwd_kv_kernel<true>), grid, block, 0, stream, qkv, dout, dqkv, batch, frames, hw, mode, bias, rot_cos, rot_sin, (const float*)rstat, part, groups);
  else LFDM_LAUNCH((attention_long_bwd_kv_kernel<false>), grid, block, 0, stream, qkv, dout, dqkv, batch, frames, hw, mode, bias, rot_cos, rot_sin, (const float*)rstat, part, groups);
  const int rc = lfdm_check_launch("attention_long_bwd");
  if (rc) return rc;
  if (dbias) return lfdm_sum_leading_f32(part, dbias, (int64_t)HEADS * L * L, groups, stream_);
  return LFDM_OK;
}
