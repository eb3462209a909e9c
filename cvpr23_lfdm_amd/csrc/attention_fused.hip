// PreNorm LayerNorm + to_qkv + temporal attention in ONE kernel (include/lfdm_hip.h:
// lfdm_temporal_attention_fused_cl_f32) for the two finest UNet levels (C = 64, 128):
// Residual(PreNorm(EinopsToAndFrom(Attention))) without its to_out projection,
// DM/modules/video_flow_diffusion.py:170-189,270-283,303-363.
//
// Why: at C = 64 the separate kernels are bound by the 126 MB qkv tensor - the projection takes 66 us to WRITE
// it (the GEMM itself is 26 us of MFMA) and the attention kernel 70 us to read it back.  Here qkv never exists.
// One wavefront owns one pixel's sequence (T <= 64 tokens) and walks over the 8 heads:
//  * the sequence's rows of x (T x C) are loaded ONCE, straight into MFMA operand registers: lane (token l&15,
//    k-slot l>>4) holds the C/4 consecutive channels (C/4)*slot .. of its token = float4 loads; the channel
//    LayerNorm statistics are two shuffles (the four slots of a token) and the rows are normalised in registers
//    (gamma is folded into the weights by the host);
//  * Q^T and K^T are computed TRANSPOSED (features x tokens = W_h . x^T): the accumulator layout of
//    v_mfma_f32_16x16x4 then has lane = token, registers = features 16*f + 4*slot + r, which IS a legal
//    operand layout for S = Q K^T (any feature order works if Q and K agree) - no layout change, scale and
//    rotary are applied on the accumulators (a rotation pair stays inside a lane);
//  * V = x W_v^T is computed untransposed: lane = feature, registers = tokens 16*t + 4*slot + r, exactly the
//    B operand of P V with the token order t(slot, s) = 16*(s>>2) + 4*slot + (s&3);
//  * the scores are computed TRANSPOSED too (S^T = K Q^T): lane = query token, registers = key tokens, so the softmax
//    over the keys is a register reduction + two shuffles and P^T is already the A operand of P V: no LDS at all
//    (attn_core.h attend_store; the fused kernels normalise with the IEEE division, attention_kernel with v_rcp_f32).
// Weight fragments (rows of W, contiguous over channels) come from L2 as float4.
#include <stdlib.h>

#include "attn_core.h"
#include "../../include/lfdm_hip.h"

namespace {

// Probe build (-DLFDM_TATTN_STAMP, tools/probe_tattn_phases.py; =2: every launch on the whole order of attend_store): the waves of
// temporal_attn_fused_out_kernel add up s_memtime cycles per phase and leave them in the buffer lfdm_tattn_stamp_buffer names.  A stamp
// is fenced on both sides, so the phases of a probe build do not overlap as the library's do: read its shares, not its length.
#ifdef LFDM_TATTN_STAMP
struct CycleProbe {
  long long t, acc[8];
  __device__ __forceinline__ void start() {
    for (int i = 0; i < 8; ++i) acc[i] = 0;
    t = clock64();
  }
  __device__ __forceinline__ void lap(int i) {
    LFDM_SCHED_FENCE();
    const long long now = clock64();
    acc[i] += now - t;
    t = now;
    LFDM_SCHED_FENCE();
  }
};
long long* tattn_stamps = nullptr;
#define TATTN_STAMP_PARAM , long long* stamps
#define TATTN_STAMP_ARG , tattn_stamps
#else
#define TATTN_STAMP_PARAM
#define TATTN_STAMP_ARG
#endif

// The body of one wavefront: heads [head_begin, head_begin + heads_per_block) of sequence `seq`; results to the global rows `out` or,
// with TO_LDS, to the workgroup's LDS tile `out`.
// ROT_RELOAD: the rotary factors are re-read from their (L1-resident, 2.5 KB) tables per head instead of living in 24 registers across the
// head loop - the one-launch block needs the registers (27 spills otherwise).
// WPACK: wqkv is in MFMA-operand order [q|k|v][head][feature half][quad q][lane][4] (lane (l15, lq) <- W[row 16*half + l15][C/4*lq + 4q ..]):
// every fragment load instruction then reads ONE contiguous 1 KB instead of a 16-byte piece of each of its 64 lanes' 64-byte segments
// (four times the L1 line look-ups per byte in the row-major layout).
// PIPE: the pipelined order of attend_store (attn_core.h).  TO_LDS: `out` is the workgroup's LDS tile.
// probe: lap(4) closes the prologue, lap(0) a head's projections, attend_store the rest.
template <int LP, int C, bool ROT_RELOAD = false, bool WPACK = false, bool PIPE = false, bool TO_LDS = false, class PROBE = NoProbe>
__device__ __forceinline__ void tattn_heads(const float* __restrict__ x, int ldx, int head_begin, int heads_per_block,
                                            const float* __restrict__ wqkv, float* __restrict__ out, int frames, int hw, int64_t seq,
                                            const float* __restrict__ bias, const float* __restrict__ rot_cos,
                                            const float* __restrict__ rot_sin, float eps, PROBE&& probe = NoProbe{}) {
  constexpr int NT = LP / 16;
  constexpr int CQ = C / 4;                        // channels per k-slot

  const int lane = threadIdx.x & 63;
  const int l15 = lane & 15, lq = lane >> 4;
  const int L = frames;
  const int64_t b = seq / hw, pix = seq - b * hw;
  const int64_t row0 = b * frames * hw + pix;

  // ---- the sequence's rows, normalised, as MFMA fragments: xf[ti][s] = xhat[token 16*ti + l15][CQ*lq + s] ----
  float xf[NT][CQ];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const int t = ti * 16 + l15;
    float s1 = 0.f, s2 = 0.f;
    if (t < L) {
      const float* src = x + (row0 + (int64_t)t * hw) * ldx + CQ * lq;
#pragma unroll
      for (int q = 0; q < CQ / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(src + 4 * q);
        xf[ti][4 * q] = v.x; xf[ti][4 * q + 1] = v.y; xf[ti][4 * q + 2] = v.z; xf[ti][4 * q + 3] = v.w;
        ln_accum(v, s1, s2);
      }
    } else {
#pragma unroll
      for (int s = 0; s < CQ; ++s) xf[ti][s] = 0.f;
    }
    float mean, rstd;
    ln_stats_slots4<false>(s1, s2, C, eps, mean, rstd);
    if (t < L) {
#pragma unroll
      for (int s = 0; s < CQ; ++s) xf[ti][s] = (xf[ti][s] - mean) * rstd;
    }
  }

  // rotary factors of this lane's tokens / feature pairs (head independent)
  float rc[NT][4], rs[NT][4];
  if (rot_cos && !ROT_RELOAD) {
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      const int t = ti * 16 + l15;
      const int tt = t < L ? t : 0;
#pragma unroll
      for (int fi = 0; fi < 2; ++fi)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          rc[ti][2 * fi + pr] = rot_cos[tt * 16 + 8 * fi + 2 * lq + pr];
          rs[ti][2 * fi + pr] = rot_sin[tt * 16 + 8 * fi + 2 * lq + pr];
        }
    }
  }
  const bool bias_vec = bias && (L % 4 == 0) && ((((uintptr_t)bias) & 15) == 0);
  probe.lap(4);

#pragma unroll 1
  for (int head = head_begin; head < head_begin + heads_per_block; ++head) {
    // ---- Q^T, K^T: rows = features (2 tiles of 16), cols = tokens (NT tiles) ----
    float qf[NT][8], kf[NT][8];
    {
      // four weight-row fragments (q/k x two feature tiles), all loads issued before the first MFMA; the NT token
      // tiles of a fragment are independent accumulator chains and are interleaved step by step.
      // (Round 6, measured and NOT kept: the head's 24 fragment loads as a hand-counted asm pipeline - 16 up front, the v fragments under
      //  the k projections, rotary moved behind the v projection: +1.9 ms per video, profiles/r06_n_tattn_asm_pipeline_ab.txt.  The ISA
      //  hipcc emits here already runs the loads one to two quads (12-24 MFMAs) ahead of their use; the weight stream is not what
      //  the launch waits for.)
      float wa[4][CQ];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float* wsrc = WPACK ? wqkv + ((int64_t)(((g >> 1) * HEADS + head) * 2 + (g & 1)) * (CQ / 4) * 64 + lane) * 4
                                  : wqkv + ((int64_t)((g >> 1) * OUT_LD + head * DH + 16 * (g & 1) + l15)) * C + CQ * lq;
#pragma unroll
        for (int q = 0; q < CQ / 4; ++q) {
          const float4 v = *reinterpret_cast<const float4*>(wsrc + (WPACK ? 256 * q : 4 * q));
          wa[g][4 * q] = v.x; wa[g][4 * q + 1] = v.y; wa[g][4 * q + 2] = v.z; wa[g][4 * q + 3] = v.w;
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 acc[NT];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) acc[ti] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < CQ; ++s)
#pragma unroll
          for (int ti = 0; ti < NT; ++ti) acc[ti] = mfma_16x16x4(wa[g][s], xf[ti][s], acc[ti]);
        // lane: token 16*ti + l15; acc[ti][r] = feature 16*fi + 4*lq + r
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if ((g >> 1) == 0) qf[ti][4 * (g & 1) + r] = acc[ti][r] * ATT_SCALE;
            else kf[ti][4 * (g & 1) + r] = acc[ti][r];
          }
      }
    }
    if (rot_cos) {
#pragma unroll
      for (int ti = 0; ti < NT; ++ti) {
#pragma unroll
        for (int fi = 0; fi < 2; ++fi)
#pragma unroll
          for (int pr = 0; pr < 2; ++pr) {
            float c, sn;                                                    // pair of features 16*fi + 4*lq + 2*pr (+1)
            if (ROT_RELOAD) {
              const int t = ti * 16 + l15, tt = t < L ? t : 0;
              c = rot_cos[tt * 16 + 8 * fi + 2 * lq + pr];
              sn = rot_sin[tt * 16 + 8 * fi + 2 * lq + pr];
            } else {
              c = rc[ti][2 * fi + pr];
              sn = rs[ti][2 * fi + pr];
            }
            rot_pair(qf[ti][4 * fi + 2 * pr], qf[ti][4 * fi + 2 * pr + 1], c, sn);
            rot_pair(kf[ti][4 * fi + 2 * pr], kf[ti][4 * fi + 2 * pr + 1], c, sn);
          }
      }
    }
    // ---- V: rows = tokens, cols = features; vf[half][4*ti + r] = v[token 16*ti + 4*lq + r][16*half + l15] ----
    float vf[2][4 * NT];
    {
      float wb[2][CQ];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const float* wsrc = WPACK ? wqkv + ((int64_t)((2 * HEADS + head) * 2 + half) * (CQ / 4) * 64 + lane) * 4
                                  : wqkv + ((int64_t)(2 * OUT_LD + head * DH + 16 * half + l15)) * C + CQ * lq;
#pragma unroll
        for (int q = 0; q < CQ / 4; ++q) {
          const float4 v = *reinterpret_cast<const float4*>(wsrc + (WPACK ? 256 * q : 4 * q));
          wb[half][4 * q] = v.x; wb[half][4 * q + 1] = v.y; wb[half][4 * q + 2] = v.z; wb[half][4 * q + 3] = v.w;
        }
      }
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        f32x4 acc[NT];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) acc[ti] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < CQ; ++s)
#pragma unroll
          for (int ti = 0; ti < NT; ++ti) acc[ti] = mfma_16x16x4(xf[ti][s], wb[half][s], acc[ti]);
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
          for (int r = 0; r < 4; ++r) vf[half][4 * ti + r] = acc[ti][r];
      }
    }

    probe.lap(0);
    attend_store<NT, false, PIPE, TO_LDS>(qf, kf, vf, head, L, l15, lq, bias, bias_vec, out, row0, hw, probe);
  }
}

template <int LP, int C, bool PIPE>
__global__ __launch_bounds__(64, 2) void temporal_attn_fused_kernel(const float* __restrict__ x, int ldx, int heads_per_block,
                                                                 const float* __restrict__ wqkv,   // (768, C), gamma folded
                                                                 float* __restrict__ out, int frames, int hw,
                                                                 const float* __restrict__ bias,
                                                                 const float* __restrict__ rot_cos,
                                                                 const float* __restrict__ rot_sin, float eps) {
  // grid.y splits the 8 heads over workgroups when there are few sequences (x is re-read per workgroup: 10-20 KB)
  tattn_heads<LP, C, false, false, PIPE>(x, ldx, blockIdx.y * heads_per_block, heads_per_block, wqkv, out, frames, hw, blockIdx.x, bias, rot_cos, rot_sin, eps);
}

// ... + to_out + residual in the same launch (round 4; lfdm_temporal_attention_fused_out_cl_f32): Residual(PreNorm(Attention)) complete,
// video_flow_diffusion.py:170-189, 286-363.  The separate to_out projection was a 25 us launch at 32x32 (0.67 GFLOP, 8 K chunks: all fixed
// cost) that re-read the 42 MB attention output the kernel above had just written in 64-byte pieces.  Here a workgroup of NW waves owns one
// pixel sequence: wave w runs heads [w * 8/NW, ...) exactly as above but parks its head outputs in the workgroup's LDS tile
// O[token][256] (row = 1 KB, the 16-byte quads XOR-swizzled by the token so that the unpadded tile reads conflict-free as MFMA A
// fragments), and after one barrier the waves share the projection out[t][c] = x[t][c] + sum_k O[t][k] Wout[c][k] on
// v_mfma_f32_16x16x4_f32: output tiles (16 tokens x 16 channels) dealt round-robin to the waves, A = O from LDS (one ds_read_b128 feeds
// four k-steps: k-slot lq of step (S, j) takes k = 16 S + 4 lq + j for BOTH operands), B = Wout straight from L2 in the same order.
// Both weight tensors arrive PACKED in operand order (ops.pack_tattn_weights): wqkv [3][8][2][4][64 lanes][4], wout [4 ct][16 S][64 lanes][4].
// LROWS = rows of the LDS tile (>= frames): 40 for the 40-frame videos (40 KB: four workgroups per CU), LP otherwise.
// PIPE: the pipelined attention core (attn_core.h attend_tiles); the launcher asks for it only with a bias that is read by quads.
template <int LP, int LROWS, int NW, bool PIPE>
__global__ __launch_bounds__(64 * NW, 2) void temporal_attn_fused_out_kernel(const float* __restrict__ x, int ldx,
                                                                          const float* __restrict__ wqkv, const float* __restrict__ wout,
                                                                          float* __restrict__ out, int ldo, int frames, int hw,
                                                                          const float* __restrict__ bias, const float* __restrict__ rot_cos,
                                                                          const float* __restrict__ rot_sin, float eps TATTN_STAMP_PARAM) {
  constexpr int C = 64, NT = LP / 16, CT = C / 16;
  __shared__ __attribute__((aligned(16))) float o_lds[LROWS * OUT_LD];
  const int wave = lfdm_uniform((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int L = frames;
  const int64_t seq = blockIdx.x;
#ifdef LFDM_TATTN_STAMP
  CycleProbe probe;
  probe.start();
#else
  NoProbe probe;
#endif
  tattn_heads<LP, C, (NW < 8), true, PIPE, true>(x, ldx, wave * (HEADS / NW), HEADS / NW, wqkv, o_lds, frames, hw, seq, bias, rot_cos, rot_sin, eps, probe);
  __syncthreads();
  probe.lap(5);
  const int64_t b = seq / hw, pix = seq - b * hw;
  const int64_t row0 = b * frames * hw + pix;
  // output tiles (ti, ct), ti-major, dealt to the waves
  for (int tile = wave; tile < NT * CT; tile += NW) {
    const int ti = tile / CT, ct = tile - ti * CT;
    const int t = ti * 16 + l15;                        // A rows: this lane's token
    const int tr = t < L ? t : L - 1;                   // (padded tokens read a valid row; their results are never stored)
    const float* arow = o_lds + tr * OUT_LD;
    const float* brow = wout + ((int64_t)ct * (OUT_LD / 16) * 64 + lane) * 4;      // packed [ct][S][lane][4]: one contiguous 1 KB per load
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc1 = acc;      // two chains: the 40-cycle dependent latency of 16x16x4 exceeds its 32-cycle issue
    // the tile's residual values are requested in front of its 128 MFMAs (round 6: loaded behind `if (tok < L)` at the store, they were a
    // dependent round trip at the end of every tile)
    float xr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int tok = ti * 16 + 4 * lq + r;
      xr[r] = x[(row0 + (int64_t)(tok < L ? tok : L - 1) * hw) * ldx + ct * 16 + l15];
    }
#pragma unroll 4
    for (int S = 0; S < OUT_LD / 16; S += 2) {
      const float4 a = *reinterpret_cast<const float4*>(arow + (((4 * S + lq) ^ (tr & 15)) << 2));
      const float4 a1 = *reinterpret_cast<const float4*>(arow + (((4 * S + 4 + lq) ^ (tr & 15)) << 2));
      const float4 w = *reinterpret_cast<const float4*>(brow + 256 * S);
      const float4 w1 = *reinterpret_cast<const float4*>(brow + 256 * S + 256);
      acc = mfma_16x16x4(a.x, w.x, acc);
      acc1 = mfma_16x16x4(a1.x, w1.x, acc1);
      acc = mfma_16x16x4(a.y, w.y, acc);
      acc1 = mfma_16x16x4(a1.y, w1.y, acc1);
      acc = mfma_16x16x4(a.z, w.z, acc);
      acc1 = mfma_16x16x4(a1.z, w1.z, acc1);
      acc = mfma_16x16x4(a.w, w.w, acc);
      acc1 = mfma_16x16x4(a1.w, w1.w, acc1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += acc1[r];
    // D: lane = channel ct*16 + l15, register r = token ti*16 + 4*lq + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int tok = ti * 16 + 4 * lq + r;
      if (tok < L) {
        const int64_t row = row0 + (int64_t)tok * hw;
        out[row * ldo + ct * 16 + l15] = acc[r] + xr[r];
      }
    }
  }
#ifdef LFDM_TATTN_STAMP
  probe.lap(6);
  if (stamps && lane == 0 && blockIdx.x < 256)
    for (int i = 0; i < 8; ++i) stamps[((int64_t)blockIdx.x * 8 + wave) * 8 + i] = probe.acc[i];
#endif
}

// Wide variant (C = 128, 256, ...): the channels are streamed in blocks of 64 with persistent Q^T / K^T / V
// accumulators, so the register budget does not grow with C; the sequence's rows are re-read from L1/L2 for every head
// and channel block (10-40 KB) and normalised on the fly with the token's mean / rstd computed once up front.
template <int LP, bool PIPE>
__global__ __launch_bounds__(64, 1) void temporal_attn_fused_wide_kernel(const float* __restrict__ x, int ldx, int channels,
                                                                      int heads_per_block, const float* __restrict__ wqkv,
                                                                      float* __restrict__ out, int frames, int hw,
                                                                      const float* __restrict__ bias,
                                                                      const float* __restrict__ rot_cos,
                                                                      const float* __restrict__ rot_sin, float eps) {
  constexpr int NT = LP / 16;
  const int lane = threadIdx.x & 63;
  const int l15 = lane & 15, lq = lane >> 4;
  const int L = frames;
  const int64_t seq = blockIdx.x;
  const int64_t b = seq / hw, pix = seq - b * hw;
  const int64_t row0 = b * frames * hw + pix;
  const int ncb = channels / 64;

  float mean[NT], rstd[NT];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const int t = ti * 16 + l15;
    float s1 = 0.f, s2 = 0.f;
    if (t < L) {
      const float* src = x + (row0 + (int64_t)t * hw) * ldx + 16 * lq;
      for (int cb = 0; cb < ncb; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) ln_accum(*reinterpret_cast<const float4*>(src + 64 * cb + 4 * q), s1, s2);
    }
    ln_stats_slots4<true>(s1, s2, channels, eps, mean[ti], rstd[ti]);
  }
  const bool bias_vec = bias && (L % 4 == 0) && ((((uintptr_t)bias) & 15) == 0);

  const int head_begin = blockIdx.y * heads_per_block;
#pragma unroll 1
  for (int head = head_begin; head < head_begin + heads_per_block; ++head) {
    f32x4 aq[2][NT], ak[2][NT], av[2][NT];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int ti = 0; ti < NT; ++ti) aq[g][ti] = ak[g][ti] = av[g][ti] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int cb = 0; cb < ncb; ++cb) {
      // weight-row fragments of this channel block: k-slot lq <-> channels 64*cb + 16*lq + s
      float w[6][16];
#pragma unroll
      for (int g = 0; g < 6; ++g) {
        const float* wsrc = wqkv + ((int64_t)((g >> 1) * OUT_LD + head * DH + 16 * (g & 1) + l15)) * channels + 64 * cb + 16 * lq;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v = *reinterpret_cast<const float4*>(wsrc + 4 * q);
          w[g][4 * q] = v.x; w[g][4 * q + 1] = v.y; w[g][4 * q + 2] = v.z; w[g][4 * q + 3] = v.w;
        }
      }
#pragma unroll
      for (int ti = 0; ti < NT; ++ti) {
        const int t = ti * 16 + l15;
        float xf[16];
        if (t < L) {
          const float* src = x + (row0 + (int64_t)t * hw) * ldx + 64 * cb + 16 * lq;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(src + 4 * q);
            xf[4 * q] = (v.x - mean[ti]) * rstd[ti]; xf[4 * q + 1] = (v.y - mean[ti]) * rstd[ti];
            xf[4 * q + 2] = (v.z - mean[ti]) * rstd[ti]; xf[4 * q + 3] = (v.w - mean[ti]) * rstd[ti];
          }
        } else {
#pragma unroll
          for (int s2 = 0; s2 < 16; ++s2) xf[s2] = 0.f;
        }
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
          aq[0][ti] = mfma_16x16x4(w[0][s2], xf[s2], aq[0][ti]);      // Q^T, K^T: rows = features, cols = tokens
          aq[1][ti] = mfma_16x16x4(w[1][s2], xf[s2], aq[1][ti]);
          ak[0][ti] = mfma_16x16x4(w[2][s2], xf[s2], ak[0][ti]);
          ak[1][ti] = mfma_16x16x4(w[3][s2], xf[s2], ak[1][ti]);
          av[0][ti] = mfma_16x16x4(xf[s2], w[4][s2], av[0][ti]);      // V: rows = tokens, cols = features
          av[1][ti] = mfma_16x16x4(xf[s2], w[5][s2], av[1][ti]);
        }
      }
    }
    float qf[NT][8], kf[NT][8], vf[2][4 * NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
      for (int fi = 0; fi < 2; ++fi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          qf[ti][4 * fi + r] = aq[fi][ti][r] * ATT_SCALE;
          kf[ti][4 * fi + r] = ak[fi][ti][r];
          vf[fi][4 * ti + r] = av[fi][ti][r];
        }
    if (rot_cos) {
#pragma unroll
      for (int ti = 0; ti < NT; ++ti) {
        const int t = ti * 16 + l15;
        const int tt = t < L ? t : 0;
#pragma unroll
        for (int fi = 0; fi < 2; ++fi)
#pragma unroll
          for (int pr = 0; pr < 2; ++pr) {
            const float c = rot_cos[tt * 16 + 8 * fi + 2 * lq + pr], sn = rot_sin[tt * 16 + 8 * fi + 2 * lq + pr];
            rot_pair(qf[ti][4 * fi + 2 * pr], qf[ti][4 * fi + 2 * pr + 1], c, sn);
            rot_pair(kf[ti][4 * fi + 2 * pr], kf[ti][4 * fi + 2 * pr + 1], c, sn);
          }
      }
    }
    attend_store<NT, false, PIPE>(qf, kf, vf, head, L, l15, lq, bias, bias_vec, out, row0, hw);
  }
}

int launch_fused_wide(const float* x, int ldx, int channels, const float* wqkv, float* out, int batch, int frames, int hw,
                      const float* bias, const float* rot_cos, const float* rot_sin, float eps, hipStream_t stream) {
  const int64_t nseq = (int64_t)batch * hw;
  int hpb = 8;
  while (hpb > 1 && nseq * (HEADS / hpb) < 2048) hpb >>= 1;
  const dim3 grid((unsigned)nseq, (unsigned)(HEADS / hpb)), block(64);
  lp_ladder(frames, [&](auto lp) {
    constexpr int LP = decltype(lp)::value;
    if (bias_by_quads(bias, frames))
      LFDM_LAUNCH((temporal_attn_fused_wide_kernel<LP, true>), grid, block, 0, stream, x, ldx, channels, hpb, wqkv, out, frames, hw, bias, rot_cos, rot_sin, eps);
    else
      LFDM_LAUNCH((temporal_attn_fused_wide_kernel<LP, false>), grid, block, 0, stream, x, ldx, channels, hpb, wqkv, out, frames, hw, bias, rot_cos, rot_sin, eps);
  });
  return lfdm_check_launch("temporal_attention_fused_wide");
}

template <int C>
int launch_fused(const float* x, int ldx, const float* wqkv, float* out, int batch, int frames, int hw, const float* bias,
                 const float* rot_cos, const float* rot_sin, float eps, hipStream_t stream) {
  const int64_t nseq = (int64_t)batch * hw;
  int hpb = 8;                                       // heads per workgroup: aim at >= 2048 workgroups
  while (hpb > 1 && nseq * (HEADS / hpb) < 2048) hpb >>= 1;
  if (const char* e = lfdm_knob("LFDM_TATTN_HPB")) {    // experiment knob (tools/bench_attn.py)
    const int v = atoi(e);
    if (v == 1 || v == 2 || v == 4 || v == 8) hpb = v;
  }
  const dim3 grid((unsigned)nseq, (unsigned)(HEADS / hpb)), block(64);
  lp_ladder(frames, [&](auto lp) {
    constexpr int LP = decltype(lp)::value;
    constexpr bool CAN_PIPE = LP <= 32;      // (at 48 and 64 the pipelined order spills more: profiles/attend_pipeline_ab.txt section 1)
    if (CAN_PIPE && bias_by_quads(bias, frames))
      LFDM_LAUNCH((temporal_attn_fused_kernel<LP, C, CAN_PIPE>), grid, block, 0, stream, x, ldx, hpb, wqkv, out, frames, hw, bias, rot_cos, rot_sin, eps);
    else
      LFDM_LAUNCH((temporal_attn_fused_kernel<LP, C, false>), grid, block, 0, stream, x, ldx, hpb, wqkv, out, frames, hw, bias, rot_cos, rot_sin, eps);
  });
  return lfdm_check_launch("temporal_attention_fused");
}

template <int LP, int LROWS>
int launch_fused_out_lp(const float* x, int ldx, const float* wqkv, const float* wout, float* out, int ldo, int batch, int frames, int hw,
                        const float* bias, const float* rot_cos, const float* rot_sin, float eps, hipStream_t stream) {
  const int64_t nseq = (int64_t)batch * hw;
  // waves per sequence: aim at >= 2048 wavefronts (like the kernel above), but never ONE wave per workgroup: the 40 KB tile admits four
  // workgroups per CU, i.e. one wave per SIMD (batched shapes lost 4 % to that before this floor, profiles/r04_t_other_configs.json)
  int nw = 2;
  while (nw < 8 && nseq * nw < 2048) nw <<= 1;
  if (const char* e = getenv("LFDM_TATTN_OUT_NW")) {      // experiment knob
    const int v = atoi(e);
    if (v == 1 || v == 2 || v == 4 || v == 8) nw = v;
  }
  const dim3 grid((unsigned)nseq);
  lfdm_ladder<1, 2, 4, 8>(nw, [&](auto nwc) {
    constexpr int NW = decltype(nwc)::value;
    // The pipelined attention core wherever it costs neither scratch nor a wave per SIMD (profiles/attend_pipeline_ab.txt section 1: at 64 rows
    // and four waves it spills 184 bytes instead of 168).  It reads the bias by quads: any other bias, or none, stays on the whole order.
#if defined(LFDM_TATTN_STAMP) && LFDM_TATTN_STAMP == 2
    constexpr bool CAN_PIPE = false;
#else
    constexpr bool CAN_PIPE = !(LP == 64 && NW == 4);
#endif
    if (CAN_PIPE && bias_by_quads(bias, frames))
      LFDM_LAUNCH((temporal_attn_fused_out_kernel<LP, LROWS, NW, CAN_PIPE>), grid, dim3(64 * NW), 0, stream, x, ldx, wqkv, wout, out, ldo, frames, hw, bias, rot_cos, rot_sin, eps TATTN_STAMP_ARG);
    else
      LFDM_LAUNCH((temporal_attn_fused_out_kernel<LP, LROWS, NW, false>), grid, dim3(64 * NW), 0, stream, x, ldx, wqkv, wout, out, ldo, frames, hw, bias, rot_cos, rot_sin, eps TATTN_STAMP_ARG);
  });
  return lfdm_check_launch("temporal_attention_fused_out");
}

}  // namespace

#ifdef LFDM_TATTN_STAMP
// 256 workgroups x 8 waves x 8 phases of 64-bit cycle sums (device memory), or nullptr
extern "C" void lfdm_tattn_stamp_buffer(void* p) { tattn_stamps = (long long*)p; }
#endif

extern "C" int lfdm_temporal_attention_fused_out_cl_f32(const float* x, int ldx, int channels, const float* wqkv, const float* wout,
                                                        float* out, int ldo, int batch, int frames, int hw, const float* bias,
                                                        const float* rot_cos, const float* rot_sin, float ln_eps, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !wqkv || !wout || !out || batch <= 0 || frames <= 0 || frames > 64 || hw <= 0 || channels != 64 || ldx < 64 || ldx % 4 != 0 ||
      ldo < 64 || !lfdm_aligned16(x, wqkv, wout) || ((rot_cos == nullptr) != (rot_sin == nullptr)) || out == x)
    return lfdm_fail(LFDM_EINVAL, "temporal_attention_fused_out: needs C == 64, frames <= 64, 16-byte aligned rows, out != x");
  return lp_ladder(frames, [&](auto lp) {
    constexpr int LP = decltype(lp)::value;
    if (LP == 48 && frames <= 40)      // the 40-frame videos: a 40-row LDS tile
      return launch_fused_out_lp<48, 40>(x, ldx, wqkv, wout, out, ldo, batch, frames, hw, bias, rot_cos, rot_sin, ln_eps, stream);
    return launch_fused_out_lp<LP, LP>(x, ldx, wqkv, wout, out, ldo, batch, frames, hw, bias, rot_cos, rot_sin, ln_eps, stream);
  });
}

extern "C" int lfdm_temporal_attention_fused_cl_f32(const float* x, int ldx, int channels, const float* wqkv, float* out,
                                                    int batch, int frames, int hw, const float* bias,
                                                    const float* rot_cos, const float* rot_sin, float ln_eps,
                                                    lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !wqkv || !out || batch <= 0 || frames <= 0 || frames > 64 || hw <= 0 || ldx < channels || ldx % 4 != 0 ||
      !lfdm_aligned16(x, wqkv) || ((rot_cos == nullptr) != (rot_sin == nullptr)) ||
      channels < 64 || channels % 64 != 0)
    return lfdm_fail(LFDM_EINVAL, "%s", "temporal_attention_fused: needs C % 64 == 0, frames <= 64, 16-byte aligned rows");
  if (channels == 64) return launch_fused<64>(x, ldx, wqkv, out, batch, frames, hw, bias, rot_cos, rot_sin, ln_eps, stream);
  return launch_fused_wide(x, ldx, channels, wqkv, out, batch, frames, hw, bias, rot_cos, rot_sin, ln_eps, stream);
}
