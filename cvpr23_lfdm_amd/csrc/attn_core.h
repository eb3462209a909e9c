// What the attention kernel files share (attention.hip, attention_fused.hip, attn_lowres.hip, linattn_fused.hip, attention_long.hip,
// train_attention.hip): the head geometry, the sequence -> rows map, the rotary pair rotation, the register-resident softmax attention
// of one (sequence, head) over at most 64 tokens, the LayerNorm statistics of fragment-resident rows and the host-side ladder over the
// padded sequence length.  Where two kernels compute the same quantity with different bits (the table under
// "Attention") the difference is a template parameter here: nothing in this header unifies arithmetic.
#pragma once
#include "lfdm_device.h"

constexpr int HEADS = 8;
constexpr int DH = 32;
constexpr int QKV_LD = 3 * HEADS * DH;  // 768
constexpr int OUT_LD = HEADS * DH;      // 256
constexpr float ATT_SCALE = 0.17677669529663687f;  // 32^-0.5

// Rows of sequence `seq`: token t is row row0 + t * tstride.  mode 0 (temporal): the `frames` rows of one pixel; mode 1 (spatial): the
// hw rows of one frame.
__device__ __forceinline__ void seq_rows(int64_t seq, int mode, int frames, int hw, int64_t& row0, int64_t& tstride) {
  if (mode == 0) {
    const int64_t b = seq / hw, pix = seq - b * hw;
    row0 = b * frames * hw + pix;
    tstride = hw;
  } else {
    row0 = seq * hw;
    tstride = 1;
  }
}

// Rotary embedding of one feature pair (x, y) by the angle (c, sn) = (cos, sin).  Which table entry belongs to which register pair is
// the caller's business: 4*lq + pr for fragments of 8 consecutive features, 8*fi + 2*lq + pr for MFMA accumulators.
__device__ __forceinline__ void rot_pair(float& x, float& y, float c, float sn) {
  const float x0 = x, y0 = y;
  x = x0 * c - y0 * sn;
  y = y0 * c + x0 * sn;
}

// The relative-position bias of the lane's query qt against the four keys of each register quad (key0 = 16*tj + 4*lq .. +3).
//  GUARDED   behind `if (bias && qt < L && key0 < L)`, vector or scalar by `bias_vec`: a load the compiler cannot move over its branch;
//  otherwise branch-free, for the pipelined attend_store: one aligned 16-byte load (bias_vec must hold: L % 4 == 0, 16-byte aligned
//            table) with the query and the keys CLAMPED into the table instead of guarded.  What a clamped load fetches for a key >= L
//            is masked by softmax_tile like everything else of that key; what it fetches for a query >= L lands in a score row that
//            is never stored and that no other row reads (a row of P V depends on its own row of P alone).
//            clamp_q: false where the query tile is known to be whole (every tile but the last one, see attend_store).
template <int NT, bool GUARDED>
__device__ __forceinline__ void bias_quads(f32x4 (&bq)[NT], int head, int L, int qt, int lq, const float* __restrict__ bias, bool bias_vec,
                                           bool clamp_q = true) {
#pragma unroll
  for (int tj = 0; tj < NT; ++tj) {
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    const int key0 = tj * 16 + lq * 4;
    if (!GUARDED) {
      const float* brow = bias + ((int64_t)head * L + (clamp_q && qt > L - 1 ? L - 1 : qt)) * L;
      const float4 b4 = *reinterpret_cast<const float4*>(brow + (tj == NT - 1 && key0 > L - 4 ? L - 4 : key0));
      bv[0] = b4.x; bv[1] = b4.y; bv[2] = b4.z; bv[3] = b4.w;
    } else if (bias && qt < L && key0 < L) {          // (guarded: unconditional loads of all nine fragments spill 84 registers)
      const float* bp = bias + ((int64_t)head * L + qt) * L + key0;
      if (bias_vec) {
        const float4 b4 = *reinterpret_cast<const float4*>(bp);
        bv[0] = b4.x; bv[1] = b4.y; bv[2] = b4.z; bv[3] = b4.w;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[r] = (key0 + r < L) ? bp[r] : 0.f;
      }
    }
    bq[tj] = bv;
  }
}

// Softmax over the keys of the lane's query token from the transposed scores of ONE query tile: st[tj][r] = score of key
// 16*tj + 4*lq + r, bq[tj][r] its relative-position bias (bias_quads; zeros without one).  Adds the bias, masks keys >= L, subtracts
// the row maximum and exponentiates in place; the four k-slots of a query share maximum and sum through two shuffles each.  Returns
// 1 / sum - FAST_RCP: v_rcp_f32, otherwise the IEEE division; the caller multiplies it into the probabilities.
template <int NT, bool FAST_RCP>
__device__ __forceinline__ float softmax_tile(f32x4 (&st)[NT], const f32x4 (&bq)[NT], int L, int lq) {
  float m = -3.0e38f;
#pragma unroll
  for (int tj = 0; tj < NT; ++tj) {
    const int key0 = tj * 16 + lq * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = (key0 + r >= L) ? -3.0e38f : st[tj][r] + bq[tj][r];
      st[tj][r] = v;
      m = fmaxf(m, v);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  float sum = 0.f;
#pragma unroll
  for (int tj = 0; tj < NT; ++tj)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = (tj * 16 + lq * 4 + r) < L ? fast_exp(st[tj][r] - m) : 0.f;
      st[tj][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  return FAST_RCP ? fast_rcp(sum) : 1.0f / sum;
}
// ... with the guarded bias read in front of it.  bias_vec: the four keys of a register quad are one aligned 16-byte load.
template <int NT, bool FAST_RCP>
__device__ __forceinline__ float softmax_tile(f32x4 (&st)[NT], int head, int L, int qt, int lq, const float* __restrict__ bias, bool bias_vec) {
  f32x4 bq[NT];
  bias_quads<NT, true>(bq, head, L, qt, lq, bias, bias_vec);
  return softmax_tile<NT, FAST_RCP>(st, bq, L, lq);
}

// The transposed scores of query tile ti against every key tile: NT independent chains of 8 MFMAs
template <int NT>
__device__ __forceinline__ void score_tile(f32x4 (&st)[NT], const float (&q)[8], const float (&kf)[NT][8]) {
#pragma unroll
  for (int tj = 0; tj < NT; ++tj) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = mfma_16x16x4(kf[tj][s], q[s], acc);
    st[tj] = acc;
  }
}

// O = P V of one query tile: two chains (the feature halves) of 4*NT MFMAs, keys in the order tj, r
template <int NT>
__device__ __forceinline__ void pv_tile(f32x4 (&o)[2], const f32x4 (&p)[NT], const float (&vf)[2][4 * NT]) {
  o[0] = (f32x4){0.f, 0.f, 0.f, 0.f};
  o[1] = o[0];
#pragma unroll
  for (int tj = 0; tj < NT; ++tj)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      o[0] = mfma_16x16x4(p[tj][r], vf[0][4 * tj + r], o[0]);
      o[1] = mfma_16x16x4(p[tj][r], vf[1][4 * tj + r], o[1]);
    }
}

// One token of a finished output tile: o[half][r] = token t, feature 16*half + l15 of `head`.  TO_LDS: into the workgroup's LDS tile
// [token][256] (16-byte quads XOR-swizzled by the token, see temporal_attn_fused_out_kernel) instead of global memory.
template <bool TO_LDS>
__device__ __forceinline__ void store_token(const f32x4 (&o)[2], int r, int t, int head, int l15, float* __restrict__ out, int64_t row0,
                                            int64_t tstride) {
  if (TO_LDS) {     // column c = head*32 + 16*half + l15 -> quad c >> 2, swizzled by the row
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int c = head * DH + 16 * half + l15;
      out[t * OUT_LD + ((((c >> 2) ^ (t & 15)) << 2) | (c & 3))] = o[half][r];
    }
  } else {
    float* dst = out + (row0 + t * tstride) * OUT_LD + head * DH;
    dst[l15] = o[0][r];
    dst[16 + l15] = o[1][r];
  }
}

// Cycle stamps of a probe build (attention_fused.hip, -DLFDM_TATTN_STAMP): lap(i) closes phase i.  The library's own builds pass NoProbe.
struct NoProbe {
  __device__ __forceinline__ void lap(int) {}
};

// The pipelined order of attend_store (the bias is there and read by quads): one query tile after the other - scores, softmax, P V,
// store - with the NEXT tile's scores requested in front of this tile's softmax and its bias quads behind it, under this tile's P V.
// At most two tiles of scores are live (the whole order holds all NT*NT), and a tile is straight-line code between two scheduling fences,
// in which the next tile's 8*NT score MFMAs are issued one per four vector instructions of this tile's softmax: a 16x16x4 MFMA occupies
// the matrix pipe for 32 cycles and the wave's issue for 8 of them, the softmax of a tile is about 100 vector instructions.  (Left to
// itself hipcc issues the MFMAs of a tile back to back and the softmax behind them; while every tile's stores stood behind a branch it
// could not move either.)  Every accumulator keeps its own order of operations (8 k-steps per score tile; tj, r into o[0] / o[1]; max,
// exp, sum per row): the results are the whole order's, bit for bit.
template <int NT, bool FAST_RCP, bool TO_LDS, class PROBE>
__device__ __forceinline__ void attend_tiles(const float (&qf)[NT][8], const float (&kf)[NT][8], const float (&vf)[2][4 * NT],
                                             int head, int L, int l15, int lq, const float* __restrict__ bias,
                                             float* __restrict__ out, int64_t row0, int64_t tstride, PROBE& probe) {
  f32x4 st[2][NT], bq[NT];                            // [tile parity][tj (key tile)]
  bias_quads<NT, false>(bq, head, L, l15, lq, bias, true, NT == 1);
  score_tile<NT>(st[0], qf[0], kf);
  LFDM_SCHED_FENCE();
  probe.lap(1);
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    f32x4 (&p)[NT] = st[ti & 1];
    if (ti + 1 < NT) score_tile<NT>(st[(ti + 1) & 1], qf[ti + 1], kf);
    const float inv = softmax_tile<NT, FAST_RCP>(p, bq, L, lq);
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) p[tj][r] = p[tj][r] * inv;
    if (ti + 1 < NT) {
#pragma unroll
      for (int i = 0; i < 8 * NT; ++i) {
        LFDM_SCHED_GROUP(LFDM_SG_MFMA, 1);
        LFDM_SCHED_GROUP(LFDM_SG_VALU, 4);
      }
    }
    probe.lap(2);
    if (ti + 1 < NT) bias_quads<NT, false>(bq, head, L, (ti + 1) * 16 + l15, lq, bias, true, ti + 1 == NT - 1);
    f32x4 o[2];
    pv_tile<NT>(o, p, vf);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = ti * 16 + lq * 4 + r;
      if (ti < NT - 1 || t < L) store_token<TO_LDS>(o, r, t, head, l15, out, row0, tstride);      // (only the last tile has padding)
    }
    LFDM_SCHED_FENCE();                               // tile ti+2 starts behind this tile
    probe.lap(3);
  }
}

// Attention of one (sequence, head) of L tokens, 16*(NT-1) < L <= 16*NT (lp_ladder below: every tile but the last is whole), by one
// wavefront, from operand-layout fragments: scores transposed, softmax in registers, P V, store.  Token t of the sequence is row
// row0 + t * tstride of `out`.
//  qf/kf[ti][s]: the features of token 16*ti + l15 in k-slot lq, q scaled and rotated, k rotated.  The sum over the 32 features is
//                order independent, so ANY assignment of features to (lq, s) works as long as q and k agree;
//  vf[half][4*ti + r] = v[token 16*ti + 4*lq + r][16*half + l15].
// S^T = K Q^T: lane = query token 16*ti + l15, registers = key tokens 16*tj + 4*lq + r.  In this orientation the softmax over the keys
// of a query is a reduction over the lane's registers plus two shuffles (the four k-slots), and the result is ALREADY the A operand of
// P V for the token order t(lq, s) = 16*(s>>2) + 4*lq + (s&3): no LDS.
// exp is the hardware exponential (lfdm_device.h fast_exp: the arguments are <= 0; error figures there); the probabilities are
// multiplied by ONE inverse of the row sum per query - v_rcp_f32 with FAST_RCP, one IEEE division 1.0f / sum without.
// TO_LDS: `out` is the workgroup's LDS tile (store_token above).
// PIPE: attend_tiles above; the caller guarantees a bias that bias_vec holds for.  Otherwise the WHOLE order: every score tile, then
// every softmax, then every P V.  Same bits either way; which instantiation takes which is decided by its registers.
template <int NT, bool FAST_RCP, bool PIPE = false, bool TO_LDS = false, class PROBE = NoProbe>
__device__ __forceinline__ void attend_store(const float (&qf)[NT][8], const float (&kf)[NT][8], const float (&vf)[2][4 * NT],
                                             int head, int L, int l15, int lq, const float* __restrict__ bias, bool bias_vec,
                                             float* __restrict__ out, int64_t row0, int64_t tstride, PROBE&& probe = NoProbe{}) {
  if (PIPE) return attend_tiles<NT, FAST_RCP, TO_LDS>(qf, kf, vf, head, L, l15, lq, bias, out, row0, tstride, probe);
  f32x4 st[NT][NT];                                   // [ti (query tile)][tj (key tile)]
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) score_tile<NT>(st[ti], qf[ti], kf);
  probe.lap(1);
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const float inv = softmax_tile<NT, FAST_RCP>(st[ti], head, L, ti * 16 + l15, lq, bias, bias_vec);
#pragma unroll
    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) st[ti][tj][r] = st[ti][tj][r] * inv;
  }
  probe.lap(2);
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    f32x4 o[2];
    pv_tile<NT>(o, st[ti], vf);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = ti * 16 + lq * 4 + r;
      if (t < L) store_token<TO_LDS>(o, r, t, head, l15, out, row0, tstride);
    }
  }
  probe.lap(3);
}

// Channel-LayerNorm statistics of a row whose channels are spread over the four k-slots of its token (lanes l15 + 16*lq): s1 / s2 =
// this lane's partial sum / sum of squares.  DIVIDE: mean = s1 / channels (the wide fused kernel), otherwise s1 * (1 / channels), a
// constant when `channels` is one (tattn_heads) - the two round differently.
__device__ __forceinline__ void ln_accum(const float4& v, float& s1, float& s2) {
  s1 += (v.x + v.y) + (v.z + v.w);
  s2 += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
}
template <bool DIVIDE>
__device__ __forceinline__ void ln_stats_slots4(float s1, float s2, int channels, float eps, float& mean, float& rstd) {
  s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
  s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
  mean = DIVIDE ? s1 / (float)channels : s1 * (1.0f / (float)channels);
  float var = (DIVIDE ? s2 / (float)channels : s2 * (1.0f / (float)channels)) - mean * mean;
  if (var < 0.f) var = 0.f;
  rstd = 1.0f / sqrtf(var + eps);
}

// Is the relative-position bias of L-token sequences read by 16-byte quads (the kernels' bias_vec)?  A launcher picks the pipelined
// instantiation of its kernel by this.
inline bool bias_by_quads(const float* bias, int L) { return bias && L % 4 == 0 && (((uintptr_t)bias) & 15) == 0; }

// lfdm_ladder (lfdm_device.h) over the padded length of a sequence of L <= 64 tokens
template <class F>
inline auto lp_ladder(int L, F&& f) { return lfdm_ladder<16, 32, 48, 64>(L, f); }
