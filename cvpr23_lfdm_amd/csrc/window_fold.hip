// Joint sampling of a long video (include/lfdm_hip.h: lfdm_window_gather_f32, lfdm_window_fold_f32): one latent of F frames is
// denoised through W overlapping windows of T frames that go through the UNet as ONE batch.  Two launches sit between the global latent
// and that batch, inside the captured step:
//   window_gather_kernel<V>   xw[b W + w, c, t, :] = x[b, c, starts[w] + t, :]: a copy.  The T frames of a window are adjacent in x and
//                             in xw, so a (window row, channel) pair is ONE run of T * E floats.
//   window_fold_kernel<V>     out[b, c, f, :] = sum_j wgt[f, j] * ew[b W + win[f, j], c, loc[f, j], :] over the frame's count[f] <= 8
//                             contributors, ascending j, one product and one addition each (no fma): a frame with ONE contributor of
//                             weight 1.0f is the window's value bit for bit.
// V = 4: 16-byte loads and stores (E % 4 == 0, bases 16-byte aligned); V = 1: the element path, same values in the same order.
// Launch plan (both): items = floats / V, 256 threads, one item per thread and trip, min(ceil(items / 256), 1024) workgroups in a
// grid-stride loop.  Memory-bound streaming: no LDS, no atomics, no workspace, nothing that depends on launch order.
#include "lfdm_device.h"
#include "../../include/lfdm_hip.h"

// the fold's error bound counts one rounding per product and per addition
#pragma clang fp contract(off)

namespace {

constexpr int kWinBlock = 256;
constexpr int kWinGridCap = 1024;
constexpr int kFoldMax = LFDM_FOLD_MAX_CONTRIB;

template <int V> struct Vec;
template <> struct Vec<4> { typedef float4 type; };
template <> struct Vec<1> { typedef float type; };

__device__ __forceinline__ float4 scaled(float w, float4 v) { return make_float4(w * v.x, w * v.y, w * v.z, w * v.w); }
__device__ __forceinline__ float scaled(float w, float v) { return w * v; }
__device__ __forceinline__ float4 added(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float added(float a, float b) { return a + b; }

struct GatherArgs {
  const float* x;                      // (B, C, F, E)
  const int* starts;                   // (W)
  float* xw;                           // (B W, C, T, E)
  int windows, channels, total_frames, frames;
  int64_t frame_elems;                 // E
  int64_t run_items;                   // T * E / V: one (window row, channel) run
  int64_t items;                       // B W C * run_items
};

template <int V>
__global__ __launch_bounds__(kWinBlock) void window_gather_kernel(GatherArgs a) {
  typedef typename Vec<V>::type vec;
  const int64_t stride = (int64_t)gridDim.x * kWinBlock;
  for (int64_t i = (int64_t)blockIdx.x * kWinBlock + (int64_t)threadIdx.x; i < a.items; i += stride) {
    const int64_t run = i / a.run_items, q = i - run * a.run_items;
    const int c = (int)(run % a.channels);
    const int64_t bw = run / a.channels;
    const int w = (int)(bw % a.windows);
    const int64_t b = bw / a.windows;
    // the table is device memory: the entry point has checked its host copy, and the start is clamped into the latent here, so a table
    // that differs from that copy reads other frames, never outside the operand
    int s = a.starts[w];
    s = s < 0 ? 0 : (s > a.total_frames - a.frames ? a.total_frames - a.frames : s);
    const float* src = a.x + ((b * a.channels + c) * a.total_frames + s) * a.frame_elems + q * V;
    *reinterpret_cast<vec*>(a.xw + i * V) = *reinterpret_cast<const vec*>(src);
  }
}

struct FoldArgs {
  const float* ew;                     // (B W, C, T, E)
  const int* count;                    // (F)
  const int* win;                      // (F, 8)
  const int* loc;                      // (F, 8)
  const float* wgt;                    // (F, 8)
  float* out;                          // (B, C, F, E)
  int windows, channels, total_frames, frames;
  int64_t frame_elems;
  int64_t row_items;                   // E / V: one frame of one channel
  int64_t items;                       // B C F * row_items
};

template <int V>
__global__ __launch_bounds__(kWinBlock) void window_fold_kernel(FoldArgs a) {
  typedef typename Vec<V>::type vec;
  const int64_t stride = (int64_t)gridDim.x * kWinBlock;
  for (int64_t i = (int64_t)blockIdx.x * kWinBlock + (int64_t)threadIdx.x; i < a.items; i += stride) {
    const int64_t row = i / a.row_items, q = i - row * a.row_items;
    const int f = (int)(row % a.total_frames);
    const int64_t bc = row / a.total_frames;
    const int c = (int)(bc % a.channels);
    const int64_t b = bc / a.channels;
    int n = a.count[f];                 // checked by the entry point on its host copy; clamped like the indices below
    n = n < 1 ? 1 : (n > kFoldMax ? kFoldMax : n);
    vec acc;
    for (int j = 0; j < n; ++j) {
      int w = a.win[f * kFoldMax + j], t = a.loc[f * kFoldMax + j];
      w = w < 0 ? 0 : (w > a.windows - 1 ? a.windows - 1 : w);
      t = t < 0 ? 0 : (t > a.frames - 1 ? a.frames - 1 : t);
      const float* src = a.ew + (((b * a.windows + w) * a.channels + c) * a.frames + t) * a.frame_elems + q * V;
      const vec term = scaled(a.wgt[f * kFoldMax + j], *reinterpret_cast<const vec*>(src));
      acc = j == 0 ? term : added(acc, term);
    }
    *reinterpret_cast<vec*>(a.out + i * V) = acc;
  }
}

bool overlaps(const void* p, int64_t p_floats, const void* q, int64_t q_floats) {
  const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  return p0 < q0 + (uintptr_t)q_floats * sizeof(float) && q0 < p0 + (uintptr_t)p_floats * sizeof(float);
}

// the shapes both entry points share; -> 0, or the refusal
int check_shapes(const char* what, int batch, int windows, int channels, int total_frames, int frames, int64_t frame_elems) {
  if (batch < 1 || windows < 1 || channels < 1 || total_frames < 1 || frames < 1 || frame_elems < 1)
    return lfdm_fail(LFDM_EINVAL, "%s: batch, windows, channels, total_frames, frames and frame_elems must be positive", what);
  if (frames > total_frames)
    return lfdm_fail(LFDM_EINVAL, "%s: a window of %d frames does not fit a latent of %d", what, frames, total_frames);
  const int64_t limit = (int64_t)1 << 40;           // floats of either operand: far above any latent, far below an int64 overflow
  if (frame_elems > limit || (int64_t)batch * windows * channels > limit / frame_elems / frames ||
      (int64_t)batch * channels > limit / frame_elems / total_frames)
    return lfdm_fail(LFDM_EINVAL, "%s: an operand of 2^40 floats or more", what);
  return 0;
}

}  // namespace

extern "C" int lfdm_window_gather_f32(const float* x, const int* starts, const int* starts_host, float* xw, int batch, int windows,
                                      int channels, int total_frames, int frames, int64_t frame_elems, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !starts || !starts_host || !xw || !lfdm_aligned<4>(x, xw) || !lfdm_aligned<4>(starts))
    return lfdm_fail(LFDM_EINVAL, "window_gather: null x / starts / starts_host / xw, or an operand not 4-byte aligned");
  if (int rc = check_shapes("window_gather", batch, windows, channels, total_frames, frames, frame_elems)) return rc;
  for (int w = 0; w < windows; ++w)
    if (starts_host[w] < 0 || starts_host[w] > total_frames - frames)
      return lfdm_fail(LFDM_EINVAL, "window_gather: starts[%d] = %d lies outside [0, total_frames - frames = %d]", w, starts_host[w],
                       total_frames - frames);
  const int64_t in_floats = (int64_t)batch * channels * total_frames * frame_elems;
  const int64_t out_floats = (int64_t)batch * windows * channels * frames * frame_elems;
  if (overlaps(x, in_floats, xw, out_floats)) return lfdm_fail(LFDM_EINVAL, "window_gather: xw may not alias x");
  const bool wide = (frame_elems & 3) == 0 && lfdm_aligned16(x, xw);
  const int v = wide ? 4 : 1;
  GatherArgs a;
  a.x = x;
  a.starts = starts;
  a.xw = xw;
  a.windows = windows;
  a.channels = channels;
  a.total_frames = total_frames;
  a.frames = frames;
  a.frame_elems = frame_elems;
  a.run_items = (int64_t)frames * frame_elems / v;
  a.items = out_floats / v;
  const dim3 grid(lfdm_blocks(a.items, kWinBlock, kWinGridCap));
  if (wide)
    LFDM_LAUNCH((window_gather_kernel<4>), grid, dim3(kWinBlock), 0, stream, a);
  else
    LFDM_LAUNCH((window_gather_kernel<1>), grid, dim3(kWinBlock), 0, stream, a);
  return lfdm_check_launch("window_gather");
}

extern "C" int lfdm_window_fold_f32(const float* ew, const int* count, const int* win, const int* loc, const float* wgt,
                                    const int* count_host, float* out, int batch, int windows, int channels, int total_frames, int frames,
                                    int64_t frame_elems, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ew || !count || !win || !loc || !wgt || !count_host || !out || !lfdm_aligned<4>(ew, out, wgt) || !lfdm_aligned<4>(count, win, loc))
    return lfdm_fail(LFDM_EINVAL, "window_fold: null ew / count / win / loc / wgt / count_host / out, or an operand not 4-byte aligned");
  if (int rc = check_shapes("window_fold", batch, windows, channels, total_frames, frames, frame_elems)) return rc;
  for (int f = 0; f < total_frames; ++f)
    if (count_host[f] < 1 || count_host[f] > kFoldMax)
      return lfdm_fail(LFDM_EINVAL, "window_fold: count[%d] = %d: every frame needs 1 .. %d contributors", f, count_host[f], kFoldMax);
  const int64_t in_floats = (int64_t)batch * windows * channels * frames * frame_elems;
  const int64_t out_floats = (int64_t)batch * channels * total_frames * frame_elems;
  if (overlaps(ew, in_floats, out, out_floats)) return lfdm_fail(LFDM_EINVAL, "window_fold: out may not alias ew");
  const bool wide = (frame_elems & 3) == 0 && lfdm_aligned16(ew, out);
  const int v = wide ? 4 : 1;
  FoldArgs a;
  a.ew = ew;
  a.count = count;
  a.win = win;
  a.loc = loc;
  a.wgt = wgt;
  a.out = out;
  a.windows = windows;
  a.channels = channels;
  a.total_frames = total_frames;
  a.frames = frames;
  a.frame_elems = frame_elems;
  a.row_items = frame_elems / v;
  a.items = out_floats / v;
  const dim3 grid(lfdm_blocks(a.items, kWinBlock, kWinGridCap));
  if (wide)
    LFDM_LAUNCH((window_fold_kernel<4>), grid, dim3(kWinBlock), 0, stream, a);
  else
    LFDM_LAUNCH((window_fold_kernel<1>), grid, dim3(kWinBlock), 0, stream, a);
  return lfdm_check_launch("window_fold");
}
