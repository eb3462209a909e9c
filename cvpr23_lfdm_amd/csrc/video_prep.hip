// Training batches from a packed uint8 frame store (include/lfdm_hip.h: lfdm_video_prep_u8) - what
// data.FrameFolderVideos.__getitem__ does on the host per frame between the decoder and the batch tensor: data.color_jitter (PIL's
// ImageEnhance Brightness / Contrast / Color and the HSV hue shift), io_compat.resize(INTER_AREA) by an integer factor, - mean, / 255 and
// the transpose to (B, 3, T, H, W).  The arithmetic is PIL's and numpy's, restated operation by operation so that the floats are the host's:
//   prep_stats_kernel        one workgroup per (b, t): the contrast grey level of the frame after brightness (integer sums, no atomics)
//   prep_kernel<K, JITTER>   one thread per 4 adjacent output pixels: K rows of 12 K source bytes in, 16 bytes per channel plane out
//   prep_kernel<K, JITTER, true>  the same for lfae_train.FramePairs' (source, driving) pairs (lfdm_frame_pairs_prep_u8): T = 2, frame t
//                            to output t (B, 3, H, H), / 255 only, a horizontal flip per item
// Off the training step: nothing here is launched unless a loader asks for it (video_store.DevicePrep, DevicePairPrep).
#include "lfdm_device.h"
#include "../../include/lfdm_hip.h"

// PIL's blend is  in1 + alpha * (in2 - in1)  with one rounding per operation, numpy's  (x - mean) / 255  likewise: no fused multiply-adds
#pragma clang fp contract(off)

#if defined(LFDM_EMU_BUILD)
static inline float __fsub_rn(float a, float b) { return a - b; }
static inline float __fdiv_rn(float a, float b) { return a / b; }
#endif

namespace {

constexpr int kPrepBlock = 256;
constexpr int kGroup = 4;                                   // output pixels per thread: one float4 per channel plane

struct PrepArgs {
  const unsigned char* store;          // (N, S, S, 3)
  const int* frame_index;              // (B, T) rows of store
  const float* params;                 // (B, 3) brightness, contrast, saturation factors
  const int* hue_shift;                // (B)
  const int* valid;                    // (B, 4) y0, x0, h, w of the picture inside a stored frame, or null: all of it
  int* grey;                           // (B, T) contrast grey level: written by the stats launch, read by the main launch
  float* out;                          // (B, 3, T, H, H)
  float mean[3];
  int frames, S, H;
  int64_t n_groups;                    // B * T * H * H / 4
  // the pair form only (T = 2, no mean): out is source, frame 1 goes to driving, both (B, 3, H, H)
  const int* flip;                     // (B) 0 or 1: mirror the rows of both frames of the item
  float* driving;
};

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// PIL's ImagingBlend on one byte: trunc(in1 + alpha * (in2 - in1)) for alpha in [0, 1], else clamped to 0 .. 255 before the truncation
__device__ __forceinline__ int blend(int d, int x, float a) {
  const float t = (float)d + a * (float)(x - d);
  if (a >= 0.f && a <= 1.f) return (int)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// PIL's RGB -> HSV -> (hue + shift) -> RGB on one pixel.  The hue and the fraction are rounded to fp32 between fp64 expressions exactly
// where PIL's C holds them in a float variable: fp64 throughout or fp32 throughout each miss some colours by one level.
__device__ __forceinline__ void hue_rotate(int& r, int& g, int& b, int shift) {
  const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  int uh = 0, us = 0;
  const int v = maxc;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc)
      h = (float)((double)bc - (double)gc);
    else if (g == maxc)
      h = (float)(2.0 + (double)rc - (double)bc);
    else
      h = (float)(4.0 + (double)gc - (double)rc);
    const double x = (double)h / 6.0 + 1.0;           // in [0.5, 2): x - floor(x) is fmod(x, 1.0), exactly
    h = (float)(x - floor(x));
    uh = clip8((int)((double)h * 255.0));
    us = clip8((int)((double)s * 255.0));
  }
  uh = (uh + shift) & 255;
  if (us == 0) {
    r = g = b = v;
    return;
  }
  const double hh = (double)(float)uh * 6.0 / 255.0;
  const double fl = floor(hh);
  const float f = (float)(hh - fl);
  const float fs = (float)((double)(float)us / 255.0);
  const double dv = (double)v;
  const int p = clip8((int)round(dv * (1.0 - (double)fs)));
  const int q = clip8((int)round(dv * (1.0 - (double)fs * (double)f)));
  const int t = clip8((int)round(dv * (1.0 - (double)fs * (1.0 - (double)f))));
  switch ((int)fl % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

struct Jitter {
  float bf, cf, sf;
  int shift, grey;
};

__device__ __forceinline__ void jitter_pixel(int& r, int& g, int& b, const Jitter& j) {
  r = blend(0, r, j.bf);
  g = blend(0, g, j.bf);
  b = blend(0, b, j.bf);
  r = blend(j.grey, r, j.cf);
  g = blend(j.grey, g, j.cf);
  b = blend(j.grey, b, j.cf);
  const int l = luma(r, g, b);
  r = blend(l, r, j.sf);
  g = blend(l, g, j.sf);
  b = blend(l, b, j.sf);
  hue_rotate(r, g, b, j.shift);
}

__device__ __forceinline__ unsigned byte_of(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

// ---------------------------------------------------------------------------------------------------------------------------------
// ImageEnhance.Contrast's grey level of one gathered frame: int(mean(L(brightness(frame))) + 0.5) = (2 sum + n) / (2 n) in integers,
// over the n picture pixels.  A thread takes 4 pixels (three dwords) per pass; per-thread and per-wave sums fit 32 bits (S <= 4096:
// at most 255 * 2^24 / 4 per wave), the four waves are added in 64.  Integer addition: the order cannot matter.
__global__ __launch_bounds__(kPrepBlock) void prep_stats_kernel(PrepArgs a) {
  __shared__ unsigned wave_part[kPrepBlock / LFDM_WAVE];
  const int bt = blockIdx.x, b = bt / a.frames, S = a.S;
  const uint32_t* frame = reinterpret_cast<const uint32_t*>(a.store + (int64_t)a.frame_index[bt] * S * S * 3);
  const float bf = a.params[3 * b];
  int y0 = 0, x0 = 0, vh = S, vw = S;
  if (a.valid) {
    y0 = a.valid[4 * b];
    x0 = a.valid[4 * b + 1];
    vh = a.valid[4 * b + 2];
    vw = a.valid[4 * b + 3];
  }
  const int groups = S * S / kGroup, groups_per_row = S / kGroup;
  unsigned sum = 0;
  for (int gi = threadIdx.x; gi < groups; gi += kPrepBlock) {
    const int y = gi / groups_per_row, x = (gi - y * groups_per_row) * kGroup;
    if (y < y0 || y >= y0 + vh) continue;
    const uint32_t w[3] = {frame[3 * gi], frame[3 * gi + 1], frame[3 * gi + 2]};
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
      const int r = blend(0, (int)byte_of(w, 3 * j), bf), g = blend(0, (int)byte_of(w, 3 * j + 1), bf),
                bl = blend(0, (int)byte_of(w, 3 * j + 2), bf);
      if (x + j >= x0 && x + j < x0 + vw) sum += (unsigned)luma(r, g, bl);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
  if ((threadIdx.x & (LFDM_WAVE - 1)) == 0) wave_part[threadIdx.x / LFDM_WAVE] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kPrepBlock / LFDM_WAVE; ++w) total += wave_part[w];
    const unsigned long long n = (unsigned long long)vh * (unsigned long long)vw;
    a.grey[bt] = (int)((2 * total + n) / (2 * n));
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Thread q makes output pixels 4 xg .. 4 xg + 3 of row y of frame (b, t): K source rows of 4 K pixels = 3 K dwords each (S % 4 == 0, so
// every such run starts on a dword), each pixel jittered, K x K byte sums per channel, one conversion, one float4 per channel plane.
// PAIRS: where flip[b] is set the row is mirrored, out[y][x] = shrunk[y][H - 1 - x]: the thread computes group H / 4 - 1 - xg exactly as
// otherwise - the valid rectangle stays in unflipped store coordinates, so the padding moves with the picture - and stores its four
// values in reversed order.  The flag is per item: the threads of one frame all take the same side.
template <int K, bool JITTER, bool PAIRS = false>
__global__ __launch_bounds__(kPrepBlock) void prep_kernel(PrepArgs a) {
  const int64_t q = (int64_t)blockIdx.x * kPrepBlock + threadIdx.x;
  if (q >= a.n_groups) return;
  const int H = a.H, S = a.S, T = a.frames;
  const int groups_per_row = H / kGroup;
  const int64_t row = q / groups_per_row;                       // (b * T + t) * H + y
  const int xg = (int)(q - row * groups_per_row);
  const int bt = (int)(row / H), y = (int)(row - (int64_t)bt * H);
  const int b = bt / T, t = bt - b * T;
  const unsigned char* frame = a.store + (int64_t)a.frame_index[bt] * S * S * 3;
  const bool mirror = PAIRS && a.flip[b] != 0;
  const int src_xg = mirror ? groups_per_row - 1 - xg : xg;
  Jitter jit = {1.f, 1.f, 1.f, 0, 0};
  int y0 = 0, x0 = 0, vh = S, vw = S;
  if (JITTER) {
    jit.bf = a.params[3 * b];
    jit.cf = a.params[3 * b + 1];
    jit.sf = a.params[3 * b + 2];
    jit.shift = a.hue_shift[b];
    jit.grey = a.grey[bt];
    if (a.valid) {
      y0 = a.valid[4 * b];
      x0 = a.valid[4 * b + 1];
      vh = a.valid[4 * b + 2];
      vw = a.valid[4 * b + 3];
    }
  }
  int sum[kGroup][3];
#pragma unroll
  for (int j = 0; j < kGroup; ++j) sum[j][0] = sum[j][1] = sum[j][2] = 0;
  // with jitter the row loop stays rolled: 4 K inlined copies of the jitter are code enough, 4 K * K of them spill
#pragma unroll(JITTER ? 1 : K)
  for (int dy = 0; dy < K; ++dy) {
    const int sy = y * K + dy, sx = src_xg * kGroup * K;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(frame + ((int64_t)sy * S + sx) * 3);
    uint32_t w[3 * K];
#pragma unroll
    for (int i = 0; i < 3 * K; ++i) w[i] = src[i];
#pragma unroll
    for (int px = 0; px < kGroup * K; ++px) {
      int r = (int)byte_of(w, 3 * px), g = (int)byte_of(w, 3 * px + 1), bl = (int)byte_of(w, 3 * px + 2);
      if (JITTER) {
        if (sy >= y0 && sy < y0 + vh && sx + px >= x0 && sx + px < x0 + vw)
          jitter_pixel(r, g, bl, jit);
        else
          r = g = bl = 0;                                        // padding is added after the jitter on the host: it stays black
      }
      sum[px / K][0] += r;
      sum[px / K][1] += g;
      sum[px / K][2] += bl;
    }
  }
  const int64_t plane = (int64_t)H * H;
  if (PAIRS) {
    float* o = (t ? a.driving : a.out) + (int64_t)b * 3 * plane + (int64_t)y * H + xg * kGroup;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // lfae_train.FramePairs has no mean: numpy's  x / 255.0  is the one division
      const float v0 = __fdiv_rn((float)sum[0][c] / (float)(K * K), 255.0f), v1 = __fdiv_rn((float)sum[1][c] / (float)(K * K), 255.0f),
                  v2 = __fdiv_rn((float)sum[2][c] / (float)(K * K), 255.0f), v3 = __fdiv_rn((float)sum[3][c] / (float)(K * K), 255.0f);
      float4 v;
      v.x = mirror ? v3 : v0;
      v.y = mirror ? v2 : v1;
      v.z = mirror ? v1 : v2;
      v.w = mirror ? v0 : v3;
      *reinterpret_cast<float4*>(o + (int64_t)c * plane) = v;
    }
    return;
  }
  float* o = a.out + ((int64_t)b * 3 * T + t) * plane + (int64_t)y * H + xg * kGroup;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float4 v;
    // the sum is an integer below 2^12 and K * K a power of two: the quotient is exact, the two roundings are numpy's
    v.x = __fdiv_rn(__fsub_rn((float)sum[0][c] / (float)(K * K), a.mean[c]), 255.0f);
    v.y = __fdiv_rn(__fsub_rn((float)sum[1][c] / (float)(K * K), a.mean[c]), 255.0f);
    v.z = __fdiv_rn(__fsub_rn((float)sum[2][c] / (float)(K * K), a.mean[c]), 255.0f);
    v.w = __fdiv_rn(__fsub_rn((float)sum[3][c] / (float)(K * K), a.mean[c]), 255.0f);
    *reinterpret_cast<float4*>(o + (int64_t)c * T * plane) = v;
  }
}

template <int K, bool PAIRS>
void launch_prep(const PrepArgs& a, bool jitter, unsigned blocks, hipStream_t stream) {
  if (jitter)
    LFDM_LAUNCH((prep_kernel<K, true, PAIRS>), dim3(blocks), dim3(kPrepBlock), 0, stream, a);
  else
    LFDM_LAUNCH((prep_kernel<K, false, PAIRS>), dim3(blocks), dim3(kPrepBlock), 0, stream, a);
}

template <bool PAIRS>
void launch_prep_ratio(int k, const PrepArgs& a, bool jitter, unsigned blocks, hipStream_t stream) {
  if (k == 1)
    launch_prep<1, PAIRS>(a, jitter, blocks, stream);
  else if (k == 2)
    launch_prep<2, PAIRS>(a, jitter, blocks, stream);
  else
    launch_prep<4, PAIRS>(a, jitter, blocks, stream);
}

}  // namespace

extern "C" size_t lfdm_video_prep_ws_bytes(int batch, int frames) {
  if (batch < 1 || frames < 1) return 0;
  return ((size_t)batch * (size_t)frames * sizeof(int) + 15) & ~(size_t)15;
}

extern "C" int lfdm_video_prep_u8(const unsigned char* store, int64_t store_frames, const int* frame_index, const float* params,
                                  const int* hue_shift, const int* valid, const float* mean, float* out, int batch, int frames,
                                  int store_size, int image_size, int jitter, int launches, void* ws, size_t ws_bytes,
                                  lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!store || !frame_index || !mean || !out || !lfdm_aligned<4>(store) || !lfdm_aligned16(out))
    return lfdm_fail(LFDM_EINVAL, "video_prep: null store / frame_index / mean / out, or store not 4-byte / out not 16-byte aligned");
  if (batch < 1 || frames < 1 || store_frames < 1 || store_size < 4 || image_size < 4 || store_size > 4096 ||
      (int64_t)batch * frames > 0x7fffffff)
    return lfdm_fail(LFDM_EINVAL, "video_prep: batch, frames, store_frames >= 1 and 4 <= image_size <= store_size <= 4096");
  if ((store_size & 3) || (image_size & 3))
    return lfdm_fail(LFDM_EINVAL, "video_prep: store_size and image_size must be multiples of 4");
  const int k = store_size / image_size;
  if (k * image_size != store_size || (k != 1 && k != 2 && k != 4))
    return lfdm_fail(LFDM_EINVAL, "video_prep: store_size / image_size must be 1, 2 or 4");
  if (!(launches & (LFDM_PREP_STATS | LFDM_PREP_MAIN)) || (launches & ~(LFDM_PREP_STATS | LFDM_PREP_MAIN)))
    return lfdm_fail(LFDM_EINVAL, "video_prep: launches is LFDM_PREP_STATS | LFDM_PREP_MAIN or one of them");
  if (jitter && (!params || !hue_shift || !ws || !lfdm_aligned<4>(ws) || ws_bytes < lfdm_video_prep_ws_bytes(batch, frames)))
    return lfdm_fail(LFDM_EINVAL, "video_prep: jitter needs params, hue_shift and a workspace of lfdm_video_prep_ws_bytes bytes (4-byte aligned)");
  PrepArgs a;
  a.store = store;
  a.frame_index = frame_index;
  a.params = params;
  a.hue_shift = hue_shift;
  a.valid = valid;
  a.grey = (int*)ws;
  a.out = out;
  for (int c = 0; c < 3; ++c) a.mean[c] = mean[c];
  a.frames = frames;
  a.S = store_size;
  a.H = image_size;
  a.n_groups = (int64_t)batch * frames * image_size * (image_size / kGroup);
  a.flip = nullptr;
  a.driving = nullptr;
  const int64_t blocks = (a.n_groups + kPrepBlock - 1) / kPrepBlock;
  if (blocks > 0x7fffffff)
    return lfdm_fail(LFDM_EINVAL, "video_prep: the batch has more than 2^41 pixels");
  if (jitter && (launches & LFDM_PREP_STATS)) {
    LFDM_LAUNCH(prep_stats_kernel, dim3((unsigned)(batch * frames)), dim3(kPrepBlock), 0, stream, a);
    const int rc = lfdm_check_launch("video_prep (stats)");
    if (rc) return rc;
  }
  if (launches & LFDM_PREP_MAIN) {
    launch_prep_ratio<false>(k, a, jitter != 0, (unsigned)blocks, stream);
    return lfdm_check_launch("video_prep");
  }
  return 0;
}

extern "C" int lfdm_frame_pairs_prep_u8(const unsigned char* store, int64_t store_frames, const int* pair_index, const float* params,
                                        const int* hue_shift, const int* valid, const int* flip, float* source, float* driving, int batch,
                                        int store_size, int image_size, int jitter, void* ws, size_t ws_bytes, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!store || !pair_index || !flip || !source || !driving || !lfdm_aligned<4>(store) || !lfdm_aligned16(source) || !lfdm_aligned16(driving))
    return lfdm_fail(LFDM_EINVAL,
                     "frame_pairs_prep: null store / pair_index / flip / source / driving, or store not 4-byte / an output not 16-byte aligned");
  if (batch < 1 || store_frames < 1 || store_size < 4 || image_size < 4 || store_size > 4096 || (int64_t)batch * 2 > 0x7fffffff)
    return lfdm_fail(LFDM_EINVAL, "frame_pairs_prep: batch, store_frames >= 1 and 4 <= image_size <= store_size <= 4096");
  if ((store_size & 3) || (image_size & 3))
    return lfdm_fail(LFDM_EINVAL, "frame_pairs_prep: store_size and image_size must be multiples of 4");
  const int k = store_size / image_size;
  if (k * image_size != store_size || (k != 1 && k != 2 && k != 4))
    return lfdm_fail(LFDM_EINVAL, "frame_pairs_prep: store_size / image_size must be 1, 2 or 4");
  if (jitter && (!params || !hue_shift || !ws || !lfdm_aligned<4>(ws) || ws_bytes < lfdm_video_prep_ws_bytes(batch, 2)))
    return lfdm_fail(LFDM_EINVAL,
                     "frame_pairs_prep: jitter needs params, hue_shift and a workspace of lfdm_video_prep_ws_bytes(batch, 2) bytes (4-byte aligned)");
  PrepArgs a;
  a.store = store;
  a.frame_index = pair_index;
  a.params = params;
  a.hue_shift = hue_shift;
  a.valid = valid;
  a.grey = (int*)ws;
  a.out = source;
  a.mean[0] = a.mean[1] = a.mean[2] = 0.f;
  a.frames = 2;
  a.S = store_size;
  a.H = image_size;
  a.n_groups = (int64_t)batch * 2 * image_size * (image_size / kGroup);
  a.flip = flip;
  a.driving = driving;
  const int64_t blocks = (a.n_groups + kPrepBlock - 1) / kPrepBlock;
  if (blocks > 0x7fffffff)
    return lfdm_fail(LFDM_EINVAL, "frame_pairs_prep: the batch has more than 2^41 pixels");
  if (jitter) {
    LFDM_LAUNCH(prep_stats_kernel, dim3((unsigned)(batch * 2)), dim3(kPrepBlock), 0, stream, a);
    const int rc = lfdm_check_launch("frame_pairs_prep (stats)");
    if (rc) return rc;
  }
  launch_prep_ratio<true>(k, a, jitter != 0, (unsigned)blocks, stream);
  return lfdm_check_launch("frame_pairs_prep");
}
