// Paired, full-reference video metrics on the device (include/lfdm_hip.h: lfdm_video_metrics, lfdm_flow_metrics, lfdm_psnr_f64;
// DESIGN.md 4.6) - what a reader of the reference's test scripts needs to compare two videos (LFAE/test_flowautoenc_*.py: the L1 of
// out_loss / warp_loss) plus MSE and the SSIM of Wang et al. 2004, and the end-point / occlusion error of two latent flows:
//   video_metrics_kernel   one workgroup per (frame, channel, 16 x 32 tile of the SSIM map): halo tile of both operands in LDS as fp64,
//                          a horizontal pass of the five window moments into LDS, a vertical pass, the SSIM map, the tile's three sums
//   video_metrics_finish   one thread per (frame, metric): adds the frame's tile sums in index order and divides by the count
//   flow_metrics_kernel    one workgroup per latent frame
// Every operand is converted exactly to fp64 and every product, moment and sum is fp64.  No floating-point atomics: a tile's sum is a
// per-thread chain in a fixed order, a wave butterfly and four LDS slots; a frame's sum is the chain over its tiles.  Which thread adds
// which pixel depends only on (C, H, W), so a frame's numbers are the same bits whatever the batch around it.  Off the sampling path.
#include "lfdm_device.h"
#include "../../include/lfdm_hip.h"

// a == b must give SSIM == 1.0 exactly: 2 (mx my) and mx mx + my my are then the same number only while neither is fused into an fma
#pragma clang fp contract(off)

namespace {

constexpr int kMetricBlock = 256;
constexpr int kWin = 11;                              // the Gaussian window of Wang et al.
constexpr int kTileW = 32, kTileH = 16;               // SSIM-map pixels per workgroup
constexpr int kHaloW = kTileW + kWin - 1;             // 42
constexpr int kHaloH = kTileH + kWin - 1;             // 26
constexpr int kWaves = kMetricBlock / LFDM_WAVE;
static_assert(kWaves == 4, "block_sum_f64 (lfdm_device.h) folds the four waves of a 256-thread workgroup");

struct VideoMetricArgs {
  const float* a;                      // (B, C, T, H, W)
  const float* b;
  double* partial;                     // (B * T, C * tiles_y * tiles_x, 3)
  double add[LFDM_METRIC_MAX_CHANNELS];      // mean_c / 255.0 (unit, uint8 domains)
  double win[kWin];                    // exp(-(i - 5)^2 / (2 * 1.5^2)) normalised to sum 1, made on the host
  int channels, frames, h, w, tiles_x, tiles_y, domain;
};

// The value a metric sees.  unit: io_compat.sample_img before its scaling (render.hip img_u8 restates the same lines for the strips):
// float32(double(x) + mean / 255) clamped to [0, 1]; uint8: the byte the demo writes, trunc(float32(v * 255)), over 255 in fp64.
// A NaN stays a NaN in the raw and unit domains and is the byte 0 in the uint8 domain, as in the strips.
__device__ __forceinline__ double metric_value(float x, double add, int domain) {
  if (domain == LFDM_METRIC_RAW) return (double)x;
  float r = (float)((double)x + add);
  r = r < 0.f ? 0.f : r;
  r = r > 1.f ? 1.f : r;
  if (domain == LFDM_METRIC_UNIT) return (double)r;
  const float q = r * 255.f;
  return q == q ? (double)(int)q / 255.0 : 0.0;
}

// Tile (ty, tx) of channel c of frame (b, t) covers SSIM-map rows ty * 16 .. + 15 and columns tx * 32 .. + 31, that is input rows
// ty * 16 .. + 25 and columns tx * 32 .. + 41 (the map is the valid interior: map pixel (y, x) has its window at input (y .. y + 10,
// x .. x + 10)).  For |a - b| and (a - b)^2 every input pixel is owned by one tile: the one whose 16 x 32 corner holds it, the last tile
// of a row / column also taking the 10 pixels behind its corner - all of them inside its halo.
// LDS rows: a 32-lane half of a wave reads 32 consecutive doubles of one row in every pass (256 bytes = one bank row of ds_read_b64),
// so the passes are conflict-free at any row pitch and the tiles are stored unpadded.
__global__ __launch_bounds__(kMetricBlock) void video_metrics_kernel(VideoMetricArgs g) {
  __shared__ double ta[kHaloH * kHaloW];
  __shared__ double tb[kHaloH * kHaloW];
  __shared__ double hp[5][kHaloH * kTileW];            // E[a], E[b], E[aa], E[bb], E[ab] along x
  __shared__ double slots[3][kWaves];
  const int tiles = g.tiles_x * g.tiles_y, per_frame = g.channels * tiles;
  const int frame = (int)(blockIdx.x / (unsigned)per_frame);
  int rem = (int)(blockIdx.x - (unsigned)frame * (unsigned)per_frame);
  const int c = rem / tiles;
  rem -= c * tiles;
  const int ty = rem / g.tiles_x, tx = rem - ty * g.tiles_x;
  const int b = frame / g.frames, t = frame - b * g.frames;
  const int H = g.h, W = g.w;
  const int y0 = ty * kTileH, x0 = tx * kTileW;
  const int64_t plane = (((int64_t)b * g.channels + c) * g.frames + t) * ((int64_t)H * W) + (int64_t)y0 * W + x0;
  const float* pa = g.a + plane;
  const float* pb = g.b + plane;
  const int rows = H - y0 < kHaloH ? H - y0 : kHaloH, cols = W - x0 < kHaloW ? W - x0 : kHaloW;      // inside the frame
  const int own_h = ty == g.tiles_y - 1 ? rows : kTileH, own_w = tx == g.tiles_x - 1 ? cols : kTileW;
  const int map_h = H - (kWin - 1) - y0 < kTileH ? H - (kWin - 1) - y0 : kTileH;
  const int map_w = W - (kWin - 1) - x0 < kTileW ? W - (kWin - 1) - x0 : kTileW;
  const double add = g.add[c];
  double l1 = 0.0, mse = 0.0, ssim = 0.0;

  for (int i = threadIdx.x; i < kHaloH * kHaloW; i += kMetricBlock) {
    const int r = i / kHaloW, cx = i - r * kHaloW;
    double va = 0.0, vb = 0.0;
    if (r < rows && cx < cols) {
      va = metric_value(pa[(int64_t)r * W + cx], add, g.domain);
      vb = metric_value(pb[(int64_t)r * W + cx], add, g.domain);
      if (r < own_h && cx < own_w) {
        const double d = va - vb;
        l1 += fabs(d);
        mse += d * d;
      }
    }
    ta[i] = va;
    tb[i] = vb;
  }
  __syncthreads();

  for (int i = threadIdx.x; i < kHaloH * kTileW; i += kMetricBlock) {
    const int r = i / kTileW, x = i - r * kTileW;
    const double* ra = ta + r * kHaloW + x;
    const double* rb = tb + r * kHaloW + x;
    double ea = 0.0, eb = 0.0, eaa = 0.0, ebb = 0.0, eab = 0.0;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const double wk = g.win[k], va = ra[k], vb = rb[k];
      ea += wk * va;
      eb += wk * vb;
      eaa += wk * (va * va);
      ebb += wk * (vb * vb);
      eab += wk * (va * vb);
    }
    hp[0][i] = ea;
    hp[1][i] = eb;
    hp[2][i] = eaa;
    hp[3][i] = ebb;
    hp[4][i] = eab;
  }
  __syncthreads();

  const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;      // data range 1 in every domain
  for (int i = threadIdx.x; i < kTileH * kTileW; i += kMetricBlock) {
    const int y = i / kTileW, x = i - y * kTileW;
    if (y < map_h && x < map_w) {
      double m[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double e = 0.0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) e += g.win[k] * hp[q][(y + k) * kTileW + x];
        m[q] = e;
      }
      const double va = m[2] - m[0] * m[0], vb = m[3] - m[1] * m[1], vab = m[4] - m[0] * m[1];
      const double num = (2.0 * (m[0] * m[1]) + c1) * (2.0 * vab + c2);
      const double den = (m[0] * m[0] + m[1] * m[1] + c1) * (va + vb + c2);
      ssim += num / den;
    }
  }
  const double s0 = block_sum_f64(l1, slots[0]);
  const double s1 = block_sum_f64(mse, slots[1]);
  const double s2 = block_sum_f64(ssim, slots[2]);
  if (threadIdx.x == 0) {
    double* out = g.partial + (int64_t)blockIdx.x * 3;
    out[0] = s0;
    out[1] = s1;
    out[2] = s2;
  }
}

// out[frame][j] = (sum of the frame's tile sums, tile 0 first) / count_j
__global__ __launch_bounds__(kMetricBlock) void video_metrics_finish(const double* __restrict__ partial, double* __restrict__ out,
                                                                     int64_t n_frames, int per_frame, double n_pixels, double n_map) {
  const int64_t i = (int64_t)blockIdx.x * kMetricBlock + threadIdx.x;
  if (i >= n_frames * 3) return;
  const int64_t frame = i / 3;
  const int j = (int)(i - frame * 3);
  const double* p = partial + frame * per_frame * 3 + j;
  double s = 0.0;
  for (int k = 0; k < per_frame; ++k) s += p[(int64_t)k * 3];
  out[i] = s / (j == 2 ? n_map : n_pixels);
}

// One workgroup per latent frame: thread i adds pixels i, i + 256, ... of the frame, then the workgroup's sum as above.
__global__ __launch_bounds__(kMetricBlock) void flow_metrics_kernel(const float* __restrict__ grid_a, int64_t stride_a,
                                                                    const float* __restrict__ grid_b, int64_t stride_b,
                                                                    const float* __restrict__ conf_a, const float* __restrict__ conf_b,
                                                                    double* __restrict__ out, int frames, int s) {
  __shared__ double slots[2][kWaves];
  const int frame = blockIdx.x, b = frame / frames, t = frame - b * frames;
  const int hw = s * s;
  const float* ax = grid_a + (int64_t)b * stride_a + (int64_t)t * hw;
  const float* ay = ax + (int64_t)frames * hw;
  const float* bx = grid_b + (int64_t)b * stride_b + (int64_t)t * hw;
  const float* by = bx + (int64_t)frames * hw;
  const float* ca = conf_a ? conf_a + (int64_t)frame * hw : nullptr;
  const float* cb = conf_b ? conf_b + (int64_t)frame * hw : nullptr;
  double epe = 0.0, occ = 0.0;
  for (int p = threadIdx.x; p < hw; p += kMetricBlock) {
    const double dx = (double)ax[p] - (double)bx[p], dy = (double)ay[p] - (double)by[p];
    epe += sqrt(dx * dx + dy * dy);
    if (ca) occ += fabs((double)ca[p] - (double)cb[p]);
  }
  const double e = block_sum_f64(epe, slots[0]);
  const double o = block_sum_f64(occ, slots[1]);
  if (threadIdx.x == 0) {
    out[(int64_t)frame * 2] = e / (double)hw;
    out[(int64_t)frame * 2 + 1] = ca ? o / (double)hw : 0.0;
  }
}

__global__ __launch_bounds__(kMetricBlock) void psnr_kernel(const double* __restrict__ mse, double* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kMetricBlock + threadIdx.x;
  if (i >= n) return;
  const double m = mse[i];
  out[i] = m == 0.0 ? __builtin_huge_val() : 10.0 * log10(1.0 / m);
}

int metric_tiles(int h, int w, int* tiles_x, int* tiles_y) {
  *tiles_x = (w - (kWin - 1) + kTileW - 1) / kTileW;
  *tiles_y = (h - (kWin - 1) + kTileH - 1) / kTileH;
  return *tiles_x * *tiles_y;
}

bool video_shape_ok(int batch, int channels, int frames, int h, int w) {
  return batch >= 1 && frames >= 1 && channels >= 1 && channels <= LFDM_METRIC_MAX_CHANNELS && h >= kWin && w >= kWin && h <= 32768 &&
         w <= 32768;
}

}  // namespace

extern "C" size_t lfdm_video_metrics_ws_bytes(int batch, int channels, int frames, int h, int w) {
  if (!video_shape_ok(batch, channels, frames, h, w)) return 0;
  int tx, ty;
  const int tiles = metric_tiles(h, w, &tx, &ty);
  return (size_t)batch * frames * channels * tiles * 3 * sizeof(double);
}

extern "C" int lfdm_video_metrics(const float* a, const float* b, const double* mean_over_255, int domain, double* out, int batch,
                                  int channels, int frames, int h, int w, void* ws, size_t ws_bytes, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!a || !b || !out || !ws || !lfdm_aligned<8>(out) || !lfdm_aligned<8>(ws) || !video_shape_ok(batch, channels, frames, h, w))
    return lfdm_fail(LFDM_EINVAL, "video_metrics: bad arguments (non-null a / b / out / ws, out and ws 8-byte aligned, batch, frames >= 1, "
                   "1 <= channels <= 4, 11 <= h, w <= 32768)");
  if (domain != LFDM_METRIC_RAW && domain != LFDM_METRIC_UNIT && domain != LFDM_METRIC_UINT8)
    return lfdm_fail(LFDM_EINVAL, "video_metrics: domain is not one of LFDM_METRIC_RAW / _UNIT / _UINT8");
  if (domain != LFDM_METRIC_RAW && !mean_over_255)
    return lfdm_fail(LFDM_EINVAL, "video_metrics: the unit and uint8 domains need mean_over_255 (channels doubles)");
  VideoMetricArgs g;
  const int tiles = metric_tiles(h, w, &g.tiles_x, &g.tiles_y);
  const int64_t n_frames = (int64_t)batch * frames;
  const int64_t blocks = n_frames * channels * tiles;
  if (blocks > 0x7fffffff || n_frames * 3 > 0x7fffffff)
    return lfdm_fail(LFDM_EINVAL, "video_metrics: batch * frames * channels * tiles exceeds 2^31 - 1");
  if (ws_bytes < (size_t)blocks * 3 * sizeof(double))
    return lfdm_fail(LFDM_EINVAL, "video_metrics: workspace smaller than lfdm_video_metrics_ws_bytes");
  g.a = a;
  g.b = b;
  g.partial = (double*)ws;
  for (int c = 0; c < LFDM_METRIC_MAX_CHANNELS; ++c) g.add[c] = domain != LFDM_METRIC_RAW && c < channels ? mean_over_255[c] : 0.0;
  double wsum = 0.0;
  for (int i = 0; i < kWin; ++i) {
    const double d = (double)(i - kWin / 2);
    g.win[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    wsum += g.win[i];
  }
  for (int i = 0; i < kWin; ++i) g.win[i] /= wsum;
  g.channels = channels;
  g.frames = frames;
  g.h = h;
  g.w = w;
  g.domain = domain;
  LFDM_LAUNCH(video_metrics_kernel, dim3((unsigned)blocks), dim3(kMetricBlock), 0, stream, g);
  const int rc = lfdm_check_launch("video_metrics");
  if (rc) return rc;
  const double n_pixels = (double)channels * h * w, n_map = (double)channels * (h - (kWin - 1)) * (w - (kWin - 1));
  LFDM_LAUNCH(video_metrics_finish, dim3((unsigned)((n_frames * 3 + kMetricBlock - 1) / kMetricBlock)), dim3(kMetricBlock), 0, stream,
              (const double*)ws, out, n_frames, channels * tiles, n_pixels, n_map);
  return lfdm_check_launch("video_metrics_finish");
}

extern "C" int lfdm_flow_metrics(const float* grid_a, int64_t stride_a, const float* grid_b, int64_t stride_b, const float* conf_a,
                                 const float* conf_b, double* out, int batch, int frames, int s, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t need = (int64_t)2 * frames * s * s;
  if (!grid_a || !grid_b || !out || !lfdm_aligned<8>(out) || batch < 1 || frames < 1 || s < 1 || s > 4096 || stride_a < need ||
      stride_b < need || (int64_t)batch * frames > 0x7fffffff || (conf_a == nullptr) != (conf_b == nullptr))
    return lfdm_fail(LFDM_EINVAL, "flow_metrics: bad arguments (non-null grids and out, out 8-byte aligned, batch, frames >= 1, 1 <= s <= 4096, "
                   "batch strides >= 2 * frames * s * s, both confidences or neither)");
  LFDM_LAUNCH(flow_metrics_kernel, dim3((unsigned)(batch * frames)), dim3(kMetricBlock), 0, stream, grid_a, stride_a, grid_b, stride_b,
              conf_a, conf_b, out, frames, s);
  return lfdm_check_launch("flow_metrics");
}

extern "C" int lfdm_psnr_f64(const double* mse, double* out, int64_t n, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!mse || !out || n < 1 || (n + kMetricBlock - 1) / kMetricBlock > 0x7fffffff)
    return lfdm_fail(LFDM_EINVAL, "psnr: bad arguments (non-null mse / out, 1 <= n < 2^39)");
  LFDM_LAUNCH(psnr_kernel, dim3((unsigned)((n + kMetricBlock - 1) / kMetricBlock)), dim3(kMetricBlock), 0, stream, mse, out, n);
  return lfdm_check_launch("psnr");
}
