// Both sides of the fused GroupNorm statistics.  A convolution that is handed lfdm_conv_params.gn_partial leaves one (sum, sum of squares)
// pair per (row chunk, group) - gn_partial[(chunk * groups + g) * 2] - and the consumer of its output merges the chunks of a sample into
// mean / rstd.  Producers: conv_igemm.hip, conv_ksw.hip, conv_wino.hip and the two split-K reduce kernels; consumers: norm.hip
// (gn_apply_kernel), small.hip (heads_gn_kernel), conv_pw.hip (res_gn_*), train_norm.hip (the GroupNorm backward).  Every summation order
// below is part of the result: where two callers associate differently (the table under "Convolution forward") the
// difference is a template parameter, nothing here unifies arithmetic.
#pragma once
#include "norm_core.h"
#include "../../include/lfdm_hip.h"

// Most channels a GroupNorm consumer keeps per-channel tables for in LDS (gn_apply_kernel's s_a / s_b, the backward's five tables); the
// LayerNorm backward sizes its dgamma staging by it too.  One bound, forward and backward: the launchers of both refuse more.
constexpr int GN_MAX_C = 1024;

// ---- producer side ----
// one float4 of finished values into the lane's four per-column accumulators
__device__ __forceinline__ void gn_accum4(const float4& v, float (&gs)[4], float (&gq)[4]) {
  gs[0] += v.x; gs[1] += v.y; gs[2] += v.z; gs[3] += v.w;
  gq[0] += v.x * v.x; gq[1] += v.y * v.y; gq[2] += v.z * v.z; gq[3] += v.w * v.w;
}

// Column sums of a tile into LDS.  Thread = (row tid >> 3, float4 column c4 = tid & 7) in every tile epilogue, so the lanes of a wave with
// equal c4 hold the same four columns of column tile j: three xor-shuffles sum them, lanes 0..7 write s_gn[sum | sumsq][slot][col0 + column].
// slot = which of the NW row parts of the tile this wave summed.  Ends in a barrier.
template <int NW, int TN, int BN>
__device__ __forceinline__ void gn_fold_lds(const float (&gs)[TN][4], const float (&gq)[TN][4], float (&s_gn)[2][NW][BN], int slot, int col0) {
  const int lane = threadIdx.x & 63, c4 = lane & 7;
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float s = gs[j][e], q = gq[j][e];
#pragma unroll
      for (int m = 8; m <= 32; m <<= 1) {
        s += __shfl_xor(s, m);
        q += __shfl_xor(q, m);
      }
      if (lane < 8) {
        s_gn[0][slot][col0 + 32 * j + 4 * c4 + e] = s;
        s_gn[1][slot][col0 + 32 * j + 4 * c4 + e] = q;
      }
    }
  __syncthreads();
}

// ... and from LDS to the chunk's slots: thread t sums the cg columns of the tile's t-th group.  NW = 2 (the 2x2-wave kernel) adds a
// column's two row parts first, NW = 4 adds the four parts one after the other.
template <int NW, int BN>
__device__ __forceinline__ void gn_fold_groups(const lfdm_conv_params& p, const float (&s_gn)[2][NW][BN], int n0, int64_t chunk) {
  const int tid = threadIdx.x;
  const int cg = p.cout / p.gn_groups;              // channels per group
  const int gpt = BN / cg;                          // groups covered by this column tile (BN % cg == 0: host check)
  if (tid < gpt && n0 + tid * cg < p.cout) {
    float s = 0.f, q = 0.f;
    for (int c = 0; c < cg; ++c) {
      if constexpr (NW == 2) {
        s += s_gn[0][0][tid * cg + c] + s_gn[0][1][tid * cg + c];
        q += s_gn[1][0][tid * cg + c] + s_gn[1][1][tid * cg + c];
      } else {
        for (int w = 0; w < NW; ++w) {
          s += s_gn[0][w][tid * cg + c];
          q += s_gn[1][w][tid * cg + c];
        }
      }
    }
    float* dst = p.gn_partial + (chunk * p.gn_groups + (n0 / cg + tid)) * 2;
    dst[0] = s;
    dst[1] = q;
  }
}

// A group wider than the workgroup's BN columns (Winograd, 512 channels / 8 groups): the workgroup's sums are ONE of the cg / BN column
// parts of its group and go to a chunk slot of their own - chunk = tile block * parts + part; the consumer merges
// (pixels / tile rows) * parts chunks per sample (host: lfdm_conv2d_plan's tile_rows, unet.py)
template <int NW, int BN>
__device__ __forceinline__ void gn_fold_part(const lfdm_conv_params& p, const float (&s_gn)[2][NW][BN], int n0, int64_t tile_block) {
  if (threadIdx.x != 0) return;
  const int cg = p.cout / p.gn_groups;
  float s = 0.f, q = 0.f;
  for (int c = 0; c < BN; ++c)
    for (int w = 0; w < NW; ++w) {
      s += s_gn[0][w][c];
      q += s_gn[1][w][c];
    }
  const int parts = cg / BN;
  float* dst = p.gn_partial + ((tile_block * parts + (n0 % cg) / BN) * p.gn_groups + n0 / cg) * 2;
  dst[0] = s;
  dst[1] = q;
}

template <int NW, int TN, int BN>
__device__ __forceinline__ void gn_fold_tile(const lfdm_conv_params& p, const float (&gs)[TN][4], const float (&gq)[TN][4],
                                             float (&s_gn)[2][NW][BN], int slot, int col0, int n0, int64_t chunk) {
  gn_fold_lds<NW, TN, BN>(gs, gq, s_gn, slot, col0);
  gn_fold_groups<NW, BN>(p, s_gn, n0, chunk);
}

// Tail of the two split-K reduce kernels (grid (row blocks, column chunks), 256 threads) and of gn_partial_kernel (norm.hip: cw = C / 4,
// cq0 = 0): a thread always sees the same column quad (256 % cw == 0), gs / gq = its sum over that quad's values; local group t owns the
// float4 columns [t * cg4, +cg4) of the block's cw (cg4 = float4 columns per group, cw % cg4 == 0).  Writes partial[row][cq0 / cg4 + t].
__device__ __forceinline__ void splitk_gn_tail(float* partial, int64_t row, int groups, int cg4, int cw, int cq0, float (&red_s)[256],
                                               float (&red_q)[256], float gs, float gq) {
  const int tid = threadIdx.x;
  red_s[tid] = gs;
  red_q[tid] = gq;
  __syncthreads();
  const int gpb = cw / cg4;                        // groups owned by this block
  if (tid < gpb) {
    float ts = 0.f, tq = 0.f;
    for (int rep = 0; rep < 256; rep += cw)
      for (int k = 0; k < cg4; ++k) {
        ts += red_s[rep + tid * cg4 + k];
        tq += red_q[rep + tid * cg4 + k];
      }
    float* dst = partial + (row * groups + cq0 / cg4 + tid) * 2;
    dst[0] = ts;
    dst[1] = tq;
  }
}

// ---- consumer side ----
// Statistics of sample b, groups g_lo .. g_hi (inclusive), from partial[b][nchunk][groups][2]: lpg lanes (32 or 64) walk one group's
// chunks with k ascending per lane and accumulate in double, an xor-shuffle tree joins the lanes, lane 0 writes s_mean / s_rstd[g - g_lo].
// n = values per group (pixels * channels per group).  NTH threads serve NTH / lpg groups per pass; no barrier inside - the caller
// synchronises before it reads the tables.  IN_FLIGHT = 4: four chunk loads per trip and a one-load tail (the sampling-path kernels);
// 1: one load per trip (the training backward).  The per-lane order of the additions is the same, so the two give the same bits.
template <int IN_FLIGHT>
__device__ __forceinline__ void gn_merge_stats(const float* __restrict__ partial, int b, int nchunk, int groups, int g_lo, int g_hi, int nth,
                                               int lpg, double n, float eps, float* s_mean, float* s_rstd) {
  static_assert(IN_FLIGHT == 1 || IN_FLIGHT == 4, "one or four chunk loads per trip");
  const int tid = threadIdx.x;
  const int gpp = nth / lpg;          // groups per pass
  const int sub = tid & (lpg - 1);
  for (int g0 = g_lo; g0 <= g_hi; g0 += gpp) {
    const int g = g0 + tid / lpg;
    double s = 0.0, q = 0.0;
    if (g <= g_hi) {
      const float2* src = reinterpret_cast<const float2*>(partial) + ((int64_t)b * nchunk) * groups + g;
      int k = sub;
      if constexpr (IN_FLIGHT == 4) {
        for (; k + 3 * lpg < nchunk; k += 4 * lpg) {
          const float2 v0 = src[(int64_t)k * groups], v1 = src[(int64_t)(k + lpg) * groups];
          const float2 v2 = src[(int64_t)(k + 2 * lpg) * groups], v3 = src[(int64_t)(k + 3 * lpg) * groups];
          s += (double)v0.x; q += (double)v0.y;
          s += (double)v1.x; q += (double)v1.y;
          s += (double)v2.x; q += (double)v2.y;
          s += (double)v3.x; q += (double)v3.y;
        }
      }
      for (; k < nchunk; k += lpg) {
        const float2 v = src[(int64_t)k * groups];
        s += (double)v.x;
        q += (double)v.y;
      }
    }
    for (int m = lpg >> 1; m >= 1; m >>= 1) {
      s += __shfl_xor(s, m);
      q += __shfl_xor(q, m);
    }
    if (g <= g_hi && sub == 0) {
      const double mean = s / n;
      double var = q / n - mean * mean;
      if (var < 0.0) var = 0.0;
      s_mean[g - g_lo] = (float)mean;
      s_rstd[g - g_lo] = (float)(1.0 / sqrt(var + (double)eps));
    }
  }
}

// The per-channel table a consumer makes of the statistics: normalised-and-affine value = x * a + b.  Sampling-path association (rstd * gamma
// first); the training backward's channel_coeffs (train_norm.hip) forms gamma * (scale + 1) first and keeps its own.
__device__ __forceinline__ void gn_affine(float mean, float rstd, float gamma, float beta, float& a, float& b) {
  a = rstd * gamma;
  b = beta - mean * a;
}
// ... followed by the block's conditioning: (x * a + b) * sc + sh, sc = scale + 1
__device__ __forceinline__ void gn_affine_ss(float& a, float& b, float sc, float sh) {
  a = a * sc;
  b = b * sc + sh;
}
