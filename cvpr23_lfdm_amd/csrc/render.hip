// uint8 preview strips of a sampled video on the device (include/lfdm_hip.h: lfdm_flow_color_u8, lfdm_render_strip_u8) -
// what the demo scripts of the reference do on the host between `sample_one_video` and the GIF writer (misc.py:66-80 flow2fig / conf2fig,
// demo_mug.py:26-32 sample_img, :124-143 the five-panel strip), with the arithmetic of cvpr23_lfdm_amd/io_compat.py restated operation
// by operation so that the bytes are the host's:
//   flow_color_kernel   one workgroup per latent frame: flow_vis.flow_to_color(grid - identity) in fp64 -> (B*T, s, s, 3) uint8
//   strip_kernel<BPP>   the strip (B, T, S, P*S[, 3]): BPP = 3 RGB bytes per pixel, BPP = 1 one index into the 6x6x6 palette per pixel
// Both read 16 bytes per lane where the operand is fp32 video and leave through LDS, so that every global store is one whole 16-byte
// segment with lane i at base + 16 i.  Off the sampling path: nothing here is launched unless a caller asks for a rendering.
#include "lfdm_device.h"
#include "../../include/lfdm_hip.h"

// numpy evaluates  u * u + v * v,  (1 - f) * w0 / 255 + f * w1 / 255,  x + mean / 255  one rounding per operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace {

constexpr int kRenderBlock = 256;
constexpr int kGroup = 4;                                   // pixels per thread: one float4 per channel
constexpr int kTilePixels = kRenderBlock * kGroup;          // 1024 pixels per workgroup pass
constexpr int kMaxPanels = 8;

// ordered dither thresholds: the 8x8 Bayer matrix, row y & 7, column x & 7
__device__ const unsigned char kBayer8[64] = {0,  32, 8,  40, 2,  34, 10, 42, 48, 16, 56, 24, 50, 18, 58, 26, 12, 44, 4,  36, 14, 46,
                                              6,  38, 60, 28, 52, 20, 62, 30, 54, 22, 3,  35, 11, 43, 1,  33, 9,  41, 51, 19, 59, 27,
                                              49, 17, 57, 25, 15, 47, 7,  39, 13, 45, 5,  37, 63, 31, 55, 23, 61, 29, 53, 21};

// level 0 .. 5 of the 6x6x6 cube for a channel value c in 0 .. 255 under threshold b in 0 .. 63:
// floor(5 c / 255 + (b + 127 / 255) / 64), at most 5 + 63.5 / 64 < 6: no clamp
__device__ __forceinline__ unsigned cube_level(unsigned c, unsigned b) { return (c * 320u + 255u * b + 127u) / 16320u; }

// 256 threads hold `bytes_per_thread` bytes each in `stage` (thread t at t * bytes_per_thread); the workgroup stores the first
// `n_bytes` of them (a multiple of 16) to dst, 16 bytes per lane, lane i at dst + 16 i.
template <int BPT>
__device__ __forceinline__ void store_staged(const uint4* stage, unsigned char* dst, int64_t n_bytes) {
  __syncthreads();
  constexpr int kSegs = kRenderBlock * BPT / 16;
  if ((int)threadIdx.x < kSegs && (int64_t)threadIdx.x * 16 < n_bytes) reinterpret_cast<uint4*>(dst)[threadIdx.x] = stage[threadIdx.x];
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// io_compat.flow_to_color(warped - identity) per frame.  grid: (B, 2, T, s, s) planar, channel 0 = x; ident: linspace(-1, 1, s) as the
// host made it (never recomputed here: the difference must be the host's, bit for bit).  The subtraction is fp32, everything behind it
// fp64 in numpy's operation order.  The frame maximum of the radius is a wave butterfly + four LDS slots: max is exact, so the result
// does not depend on the order, and there is no atomic.
__global__ __launch_bounds__(kRenderBlock) void flow_color_kernel(const float* __restrict__ grid, int64_t batch_stride,
                                                                  const float* __restrict__ ident, unsigned char* __restrict__ out,
                                                                  int frames, int s) {
  __shared__ double wheel[55 * 3];
  __shared__ double wave_part[kRenderBlock / LFDM_WAVE];
  __shared__ uint4 stage[kRenderBlock * kGroup * 3 / 16];
  const int frame = blockIdx.x, b = frame / frames, t = frame % frames;
  const int hw = s * s;
  const float* gx = grid + (int64_t)b * batch_stride + (int64_t)t * hw;
  const float* gy = gx + (int64_t)frames * hw;
  if (threadIdx.x < 55) {      // the Middlebury wheel (io_compat._color_wheel): six ramps of floor(255 j / n), up or down, beside a fixed 255
    const int k = threadIdx.x;
    const int start[7] = {0, 15, 21, 25, 36, 49, 55}, fixed[6] = {0, 1, 1, 2, 2, 0}, ramp[6] = {1, 0, 2, 1, 0, 2};
    int seg = 0;
    while (k >= start[seg + 1]) ++seg;
    const int n = start[seg + 1] - start[seg], step = 255 * (k - start[seg]) / n;
    double w[3] = {0.0, 0.0, 0.0};
    w[fixed[seg]] = 255.0;
    w[ramp[seg]] = (double)((seg & 1) ? 255 - step : step);
    wheel[3 * k] = w[0];
    wheel[3 * k + 1] = w[1];
    wheel[3 * k + 2] = w[2];
  }
  double m = 0.0;
  for (int p = threadIdx.x; p < hw; p += kRenderBlock) {
    const float uf = gx[p] - ident[p % s], vf = gy[p] - ident[p / s];
    const double u = (double)uf, v = (double)vf;
    const double r = sqrt(u * u + v * v);
    m = r > m ? r : m;
  }
  m = wave_max(m);      // (m is never a NaN: `r > m` above lets none in)
  if ((threadIdx.x & (LFDM_WAVE - 1)) == 0) wave_part[threadIdx.x / LFDM_WAVE] = m;
  __syncthreads();
  double rad_max = wave_part[0];
#pragma unroll
  for (int w = 1; w < kRenderBlock / LFDM_WAVE; ++w) rad_max = wave_part[w] > rad_max ? wave_part[w] : rad_max;
  const double denom = rad_max + 1e-5;
  unsigned char* frame_out = out + (int64_t)frame * hw * 3;
  for (int p0 = 0; p0 < hw; p0 += kTilePixels) {
    unsigned char px[kGroup * 3];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
      const int p = p0 + (int)threadIdx.x * kGroup + j;
      unsigned char c3[3] = {0, 0, 0};
      if (p < hw) {
        const float uf = gx[p] - ident[p % s], vf = gy[p] - ident[p / s];
        const double u = (double)uf / denom, v = (double)vf / denom;
        const double rad = sqrt(u * u + v * v);
        const double fk = (atan2(-v, -u) / 3.141592653589793 + 1.0) / 2.0 * 54.0;
        const double fl = floor(fk);
        int k0 = (int)fl;
        k0 = k0 < 0 ? 0 : (k0 > 54 ? 54 : k0);          // (only a NaN flow can leave 0 .. 54; keeps the table read inside)
        const int k1 = k0 + 1 == 55 ? 0 : k0 + 1;
        const double f = fk - fl;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          double col = (1.0 - f) * wheel[3 * k0 + i] / 255.0 + f * wheel[3 * k1 + i] / 255.0;
          col = rad <= 1.0 ? 1.0 - rad * (1.0 - col) : col * 0.75;
          const double q = floor(255.0 * col);
          c3[i] = q >= 0.0 && q <= 255.0 ? (unsigned char)q : 0;      // NaN -> 0
        }
      }
      px[3 * j] = c3[0];
      px[3 * j + 1] = c3[1];
      px[3 * j + 2] = c3[2];
    }
    uint32_t* st = reinterpret_cast<uint32_t*>(stage) + 3 * threadIdx.x;
#pragma unroll
    for (int d = 0; d < 3; ++d)
      st[d] = (uint32_t)px[4 * d] | ((uint32_t)px[4 * d + 1] << 8) | ((uint32_t)px[4 * d + 2] << 16) | ((uint32_t)px[4 * d + 3] << 24);
    const int left = hw - p0;
    store_staged<kGroup * 3>(stage, frame_out + (int64_t)p0 * 3, (int64_t)(left < kTilePixels ? left : kTilePixels) * 3);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct StripArgs {
  const float* source;                 // (B, 3, S, S)
  const float* out_vid;                // (B, 3, T, S, S)
  const float* warped_vid;             // (B, 3, T, S, S)
  const unsigned char* flow_color;     // (B * T, s, s, 3): flow_color_kernel's output
  const float* conf;                   // (B, 1, T, s, s)
  unsigned char* out;                  // (B, T, S, P * S, BPP)
  double add[3];                       // mean_c / 255.0, divided in double on the host like numpy does
  int panels[kMaxPanels];
  int n_panels, frames, S, s;
  int64_t n_groups;                    // B * T * S * P * S / 4
};

// io_compat.sample_img on one value: float32(double(x) + mean / 255) -> [0, 1] -> fp32 * 255 -> truncate.  The sum is rounded to fp32
// before the product, so the two can never fuse.  NaN -> 0.
__device__ __forceinline__ unsigned img_u8(float x, double add) {
  float r = (float)((double)x + add);
  r = r < 0.f ? 0.f : r;
  r = r > 1.f ? 1.f : r;
  const float q = r * 255.f;
  return q == q ? (unsigned)(int)q : 0u;
}

// one axis of F.interpolate(mode="bilinear", align_corners=False) at the exact factor 4, output index d = 4 k + j: source coordinate
// k + (2 j - 3) / 8 clamped at 0 -> left tap i0, right tap i1 = min(i0 + 1, s - 1), weight of the right tap w1 / 8 (left: (8 - w1) / 8)
__device__ __forceinline__ void tap4(int d, int s, int& i0, int& i1, int& w1) {
  const int k = d >> 2, j = d & 3;
  if (j < 2) {
    i0 = k - 1;
    w1 = 5 + 2 * j;
    if (i0 < 0) {
      i0 = 0;
      w1 = 0;
    }
  } else {
    i0 = k;
    w1 = 2 * j - 3;
  }
  i1 = i0 + 1 < s ? i0 + 1 : s - 1;
}

// Thread q of the launch renders pixels 4 q .. 4 q + 3 of the flat output (a row of the strip is P * S pixels and S % 16 == 0, so the
// four lie in one panel row) and the workgroup's 1024 pixels leave as 192 (RGB) or 64 (indexed) 16-byte segments.
template <int BPP>
__global__ __launch_bounds__(kRenderBlock) void strip_kernel(StripArgs a) {
  __shared__ uint4 stage[kRenderBlock * kGroup * BPP / 16];
  const int64_t q = (int64_t)blockIdx.x * kRenderBlock + threadIdx.x;
  unsigned rgb[kGroup][3];
#pragma unroll
  for (int j = 0; j < kGroup; ++j) rgb[j][0] = rgb[j][1] = rgb[j][2] = 0u;
  int x_strip = 0, y = 0;
  if (q < a.n_groups) {
    const int S = a.S, s = a.s, T = a.frames;
    const int groups_per_row = a.n_panels * S / kGroup;
    const int row = (int)(q / groups_per_row);                 // (b * T + t) * S + y
    x_strip = (int)(q - (int64_t)row * groups_per_row) * kGroup;
    const int slot = x_strip / S, x = x_strip - slot * S;
    const int bt = row / S;
    y = row - bt * S;
    const int b = bt / T, t = bt - b * T;
    const int kind = a.panels[slot];
    const int64_t plane = (int64_t)S * S;
    if (kind == LFDM_PANEL_SOURCE || kind == LFDM_PANEL_OUT || kind == LFDM_PANEL_WARPED) {
      const float* base;
      int64_t cstride;
      if (kind == LFDM_PANEL_SOURCE) {
        base = a.source + (int64_t)b * 3 * plane;
        cstride = plane;
      } else {
        base = (kind == LFDM_PANEL_OUT ? a.out_vid : a.warped_vid) + ((int64_t)b * 3 * T + t) * plane;
        cstride = (int64_t)T * plane;
      }
      base += (int64_t)y * S + x;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(base + c * cstride);
        rgb[0][c] = img_u8(v.x, a.add[c]);
        rgb[1][c] = img_u8(v.y, a.add[c]);
        rgb[2][c] = img_u8(v.z, a.add[c]);
        rgb[3][c] = img_u8(v.w, a.add[c]);
      }
    } else if (kind == LFDM_PANEL_CONF) {
      // conf2fig: nearest source index floor(d * 0.25f) = d >> 2, conf * 255 in fp32, truncated, on three channels
      const float cv = a.conf[(int64_t)bt * s * s + (y >> 2) * s + (x >> 2)] * 255.f;
      const unsigned g = cv >= 0.f ? (cv <= 255.f ? (unsigned)(int)cv : 255u) : 0u;      // NaN -> 0
#pragma unroll
      for (int j = 0; j < kGroup; ++j) rgb[j][0] = rgb[j][1] = rgb[j][2] = g;
    } else {
      // _resize_hw(colour, S, S, INTER_LINEAR) on the uint8 colour image: weights in eighths per axis, so 64 * value is an integer sum;
      // rounded half to even like np.rint
      const unsigned char* img = a.flow_color + (int64_t)bt * s * s * 3;
      int y0, y1, wy;
      tap4(y, s, y0, y1, wy);
#pragma unroll
      for (int j = 0; j < kGroup; ++j) {
        int x0, x1, wx;
        tap4(x + j, s, x0, x1, wx);
        const unsigned char* p00 = img + (y0 * s + x0) * 3;
        const unsigned char* p01 = img + (y0 * s + x1) * 3;
        const unsigned char* p10 = img + (y1 * s + x0) * 3;
        const unsigned char* p11 = img + (y1 * s + x1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int v64 = (8 - wy) * ((8 - wx) * p00[c] + wx * p01[c]) + wy * ((8 - wx) * p10[c] + wx * p11[c]);
          int r = v64 >> 6;
          const int rem = v64 & 63;
          if (rem > 32 || (rem == 32 && (r & 1))) ++r;
          rgb[j][c] = (unsigned)r;
        }
      }
    }
  }
  uint32_t* st = reinterpret_cast<uint32_t*>(stage);
  if (BPP == 3) {
    unsigned char px[kGroup * 3];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
      px[3 * j] = (unsigned char)rgb[j][0];
      px[3 * j + 1] = (unsigned char)rgb[j][1];
      px[3 * j + 2] = (unsigned char)rgb[j][2];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d)
      st[3 * threadIdx.x + d] =
          (uint32_t)px[4 * d] | ((uint32_t)px[4 * d + 1] << 8) | ((uint32_t)px[4 * d + 2] << 16) | ((uint32_t)px[4 * d + 3] << 24);
  } else {
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
      const unsigned th = kBayer8[(y & 7) * 8 + ((x_strip + j) & 7)];
      const unsigned idx = 36u * cube_level(rgb[j][0], th) + 6u * cube_level(rgb[j][1], th) + cube_level(rgb[j][2], th);
      word |= idx << (8 * j);
    }
    st[threadIdx.x] = word;
  }
  const int64_t first = (int64_t)blockIdx.x * kTilePixels * BPP;
  store_staged<kGroup * BPP>(stage, a.out + first, a.n_groups * kGroup * BPP - first);
}

}  // namespace

extern "C" int lfdm_flow_color_u8(const float* grid, int64_t batch_stride, const float* ident, unsigned char* out, int batch, int frames,
                                  int s, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!grid || !ident || !out || batch < 1 || frames < 1 || s < 4 || (s & 3) || s > 4096 ||
      batch_stride < (int64_t)2 * frames * s * s || (int64_t)batch * frames > 0x7fffffff || !lfdm_aligned16(out))
    return lfdm_fail(LFDM_EINVAL, "flow_color: bad arguments (non-null grid / ident / out, out 16-byte aligned, batch, frames >= 1, s a multiple of 4, "
                   "batch_stride >= 2 * frames * s * s)");
  LFDM_LAUNCH(flow_color_kernel, dim3((unsigned)(batch * frames)), dim3(kRenderBlock), 0, stream, grid, batch_stride, ident, out, frames,
              s);
  return lfdm_check_launch("flow_color");
}

extern "C" int lfdm_render_strip_u8(const float* source, const float* out_vid, const float* warped_vid, const unsigned char* flow_color,
                                    const float* conf, const double* mean_over_255, const int* panels, int n_panels, int indexed,
                                    unsigned char* out, int batch, int frames, int S, int s, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!panels || n_panels < 1 || n_panels > kMaxPanels)
    return lfdm_fail(LFDM_EINVAL, "render_strip: the panel list is empty (1 .. 8 panels of LFDM_PANEL_*)");
  if (!out || !mean_over_255 || batch < 1 || frames < 1 || s < 4 || (s & 3) || !lfdm_aligned16(out))
    return lfdm_fail(LFDM_EINVAL, "render_strip: bad arguments (non-null out (16-byte aligned) and mean, batch, frames >= 1, s a multiple of 4)");
  if (S != 4 * s || S > 8192) {
    return lfdm_fail(LFDM_EINVAL, "render_strip: S must be 4 * s (the LFAE's factor between frame and latent; at most 8192)");
  }
  StripArgs a;
  for (int i = 0; i < kMaxPanels; ++i) a.panels[i] = 0;
  for (int i = 0; i < n_panels; ++i) {
    const int k = panels[i];
    const void* need = k == LFDM_PANEL_SOURCE ? (const void*)source : k == LFDM_PANEL_OUT ? (const void*)out_vid
                       : k == LFDM_PANEL_WARPED ? (const void*)warped_vid : k == LFDM_PANEL_FLOW ? (const void*)flow_color
                       : k == LFDM_PANEL_CONF ? (const void*)conf : nullptr;
    if (k < LFDM_PANEL_SOURCE || k > LFDM_PANEL_CONF || !need || (k <= LFDM_PANEL_WARPED && !lfdm_aligned16(need)))
      return lfdm_fail(LFDM_EINVAL, "render_strip: a panel is not one of LFDM_PANEL_*, or its operand is null (image operands 16-byte aligned)");
    a.panels[i] = k;
  }
  const int64_t rows = (int64_t)batch * frames * S;
  if (rows > 0x7fffffff)
    return lfdm_fail(LFDM_EINVAL, "render_strip: batch * frames * S exceeds 2^31 - 1");
  a.source = source;
  a.out_vid = out_vid;
  a.warped_vid = warped_vid;
  a.flow_color = flow_color;
  a.conf = conf;
  a.out = out;
  for (int c = 0; c < 3; ++c) a.add[c] = mean_over_255[c];
  a.n_panels = n_panels;
  a.frames = frames;
  a.S = S;
  a.s = s;
  a.n_groups = rows * n_panels * S / kGroup;
  const int64_t blocks = (a.n_groups + kRenderBlock - 1) / kRenderBlock;
  if (blocks > 0x7fffffff)
    return lfdm_fail(LFDM_EINVAL, "render_strip: the strip has more than 2^41 pixels");
  if (indexed)
    LFDM_LAUNCH(strip_kernel<1>, dim3((unsigned)blocks), dim3(kRenderBlock), 0, stream, a);
  else
    LFDM_LAUNCH(strip_kernel<3>, dim3((unsigned)blocks), dim3(kRenderBlock), 0, stream, a);
  return lfdm_check_launch("render_strip");
}
