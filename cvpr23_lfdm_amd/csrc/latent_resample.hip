// Temporal resampling of a sampled flow latent (include/lfdm_hip.h: lfdm_latent_resample_f32): every frame of a latent
// (B, C, T, H, W) is a backward warp field + occlusion map relative to the SAME source image, so a field between two sampled frames is a
// weighted mix of its neighbours.  One launch makes T' output frames from host-prepared time tables (idx[j], frac[j]):
//   resample_kernel<CUBIC, MAPS>   grid (plane chunks, T', B), one thread per 4 adjacent values of a plane and all C channels of them
//     frac == 0   the frame idx[j] itself, by selection: no arithmetic, no other frame read (a NaN elsewhere cannot reach it)
//     linear      x[i] + a * (x[i+1] - x[i])
//     cubic       Catmull-Rom over clamp(i-1), i, i+1, clamp(i+2): w0 x0 + w1 x1 + w2 x2 + w3 x3
//   MAPS (C == 3): what FlowDiffusion._maps does behind it, in the same launch - + identity on channels 0 / 1 (residual flow), and
//   conf = (ch2 + 1) * 0.5 to a second output.
// Elementwise and memory-bound: 16-byte loads, whole 16-byte stores, (idx, frac) read once per workgroup through a uniform address, no
// atomics, nothing that depends on launch order.  Off the sampling path: nothing here is launched unless a caller asks for other times.
#include "lfdm_device.h"
#include "../../include/lfdm_hip.h"

// x + identity and (x + 1) * 0.5 must be torch's single roundings; the interpolation's error bound counts one rounding per operation
#pragma clang fp contract(off)

namespace {

constexpr int kResampleBlock = 256;
constexpr int kGroup = 4;                                   // values per thread and channel: one float4

struct ResampleArgs {
  const float* latent;                 // (B, C, T, H, W)
  const int* idx;                      // (T') frame index
  const float* frac;                   // (T') position behind that frame, [0, 1)
  const float* ident_x;                // (W) or null
  const float* ident_y;                // (H) or null
  float* out;                          // (B, C, T', H, W)
  float* conf;                         // (B, 1, T', H, W) (MAPS)
  int channels, frames, out_frames, w, clamp_from;
  int groups;                          // H * W / 4
};

__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ float clamp1(float v) {
  v = v < -1.f ? -1.f : v;
  return v > 1.f ? 1.f : v;
}

template <bool CUBIC, bool MAPS>
__global__ __launch_bounds__(kResampleBlock) void resample_kernel(ResampleArgs a) {
  const int g = (int)blockIdx.x * kResampleBlock + (int)threadIdx.x;
  const int j = (int)blockIdx.y, b = (int)blockIdx.z;
  const int T = a.frames, C = a.channels;
  // the same for every thread of the workgroup.  The tables are device memory the entry point cannot check: the index is clamped into the
  // latent here, so a bad table reads a wrong frame, never outside the operand.
  int i = a.idx[j];
  i = i < 0 ? 0 : (i > T - 1 ? T - 1 : i);
  const float fr = a.frac[j];
  const bool exact = fr == 0.f;
  if (g >= a.groups) return;
  const int64_t plane = (int64_t)a.groups * kGroup;
  const int i0 = i > 0 ? i - 1 : 0, i2 = i + 1 < T ? i + 1 : T - 1, i3 = i + 2 < T ? i + 2 : T - 1;
  float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
  if (CUBIC) {
    // the four weights in fp64, rounded once each: their error stays below the products' (a handful of operations per thread)
    const double t = (double)fr;
    w0 = (float)(((2.0 - t) * t - 1.0) * t * 0.5);
    w1 = (float)(((3.0 * t - 5.0) * t * t + 2.0) * 0.5);
    w2 = (float)(((4.0 - 3.0 * t) * t + 1.0) * t * 0.5);
    w3 = (float)((t - 1.0) * t * t * 0.5);
  }
  float add_x[kGroup] = {0.f, 0.f, 0.f, 0.f}, add_y[kGroup] = {0.f, 0.f, 0.f, 0.f};
  if (MAPS && a.ident_x) {
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {          // H * W % 4 == 0 does not keep the four values in one row
      const int p = g * kGroup + k, y = p / a.w;
      add_x[k] = a.ident_x[p - y * a.w];
      add_y[k] = a.ident_y[y];
    }
  }
  const float* src = a.latent + (int64_t)b * C * T * plane + (int64_t)g * kGroup;
  float* dst = a.out + ((int64_t)b * C * a.out_frames + j) * plane + (int64_t)g * kGroup;
  for (int c = 0; c < C; ++c) {
    const float* sc = src + (int64_t)c * T * plane;
    float4 v = load4(sc + (int64_t)i * plane);
    if (!exact) {
      const float4 x2 = load4(sc + (int64_t)i2 * plane);
      if (CUBIC) {
        const float4 x0 = load4(sc + (int64_t)i0 * plane), x3 = load4(sc + (int64_t)i3 * plane);
        v.x = ((w0 * x0.x + w1 * v.x) + w2 * x2.x) + w3 * x3.x;
        v.y = ((w0 * x0.y + w1 * v.y) + w2 * x2.y) + w3 * x3.y;
        v.z = ((w0 * x0.z + w1 * v.z) + w2 * x2.z) + w3 * x3.z;
        v.w = ((w0 * x0.w + w1 * v.w) + w2 * x2.w) + w3 * x3.w;
      } else {
        v.x = v.x + fr * (x2.x - v.x);
        v.y = v.y + fr * (x2.y - v.y);
        v.z = v.z + fr * (x2.z - v.z);
        v.w = v.w + fr * (x2.w - v.w);
      }
      if (c >= a.clamp_from) {
        v.x = clamp1(v.x);
        v.y = clamp1(v.y);
        v.z = clamp1(v.z);
        v.w = clamp1(v.w);
      }
    }
    if (MAPS) {
      if (c == 2) {
        float4 cf;
        cf.x = (v.x + 1.f) * 0.5f;
        cf.y = (v.y + 1.f) * 0.5f;
        cf.z = (v.z + 1.f) * 0.5f;
        cf.w = (v.w + 1.f) * 0.5f;
        *reinterpret_cast<float4*>(a.conf + ((int64_t)b * a.out_frames + j) * plane + (int64_t)g * kGroup) = cf;
      } else if (a.ident_x) {
        const float* ad = c == 0 ? add_x : add_y;
        v.x = v.x + ad[0];
        v.y = v.y + ad[1];
        v.z = v.z + ad[2];
        v.w = v.w + ad[3];
      }
    }
    *reinterpret_cast<float4*>(dst + (int64_t)c * a.out_frames * plane) = v;
  }
}

bool overlaps(const void* p, int64_t p_floats, const void* q, int64_t q_floats) {
  const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  return p0 < q0 + (uintptr_t)q_floats * sizeof(float) && q0 < p0 + (uintptr_t)p_floats * sizeof(float);
}

}  // namespace

extern "C" int lfdm_latent_resample_f32(const float* latent, const int* idx, const float* frac, const float* ident_x, const float* ident_y,
                                        float* out, float* conf, int batch, int channels, int frames, int out_frames, int h, int w,
                                        int mode, int clamp_from, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!latent || !idx || !frac || !out || !lfdm_aligned16(latent) || !lfdm_aligned16(out) || !lfdm_aligned16(conf) ||
      !lfdm_aligned<4>(idx) || !lfdm_aligned<4>(frac))
    return lfdm_fail(LFDM_EINVAL, "latent_resample: null latent / idx / frac / out, or latent / out / conf not 16-byte aligned");
  if (mode != LFDM_RESAMPLE_LINEAR && mode != LFDM_RESAMPLE_CUBIC)
    return lfdm_fail(LFDM_EINVAL, "latent_resample: mode is LFDM_RESAMPLE_LINEAR or LFDM_RESAMPLE_CUBIC");
  if (batch < 1 || channels < 1 || frames < 1 || out_frames < 1 || h < 1 || w < 1 || batch > 65535 || out_frames > 65535 ||
      clamp_from < 0)
    return lfdm_fail(LFDM_EINVAL, "latent_resample: batch, channels, frames, out_frames, h, w >= 1, batch and out_frames <= 65535, clamp_from >= 0");
  const int64_t plane = (int64_t)h * w;
  if ((plane & 3) || plane > 0x7fffffff)
    return lfdm_fail(LFDM_EINVAL, "latent_resample: h * w must be a multiple of 4 (below 2^31)");
  const bool maps = conf != nullptr;
  if ((ident_x == nullptr) != (ident_y == nullptr) || (ident_x && !maps))
    return lfdm_fail(LFDM_EINVAL, "latent_resample: ident_x and ident_y come together, and only with conf (the maps form)");
  if (maps && channels != 3)
    return lfdm_fail(LFDM_EINVAL, "latent_resample: the maps form (conf given) needs channels == 3");
  const int64_t in_floats = (int64_t)batch * channels * frames * plane, out_floats = (int64_t)batch * channels * out_frames * plane;
  const int64_t conf_floats = (int64_t)batch * out_frames * plane;
  if (overlaps(latent, in_floats, out, out_floats) || (maps && (overlaps(latent, in_floats, conf, conf_floats) ||
                                                                overlaps(out, out_floats, conf, conf_floats))))
    return lfdm_fail(LFDM_EINVAL, "latent_resample: out / conf may not alias latent or each other");
  ResampleArgs a;
  a.latent = latent;
  a.idx = idx;
  a.frac = frac;
  a.ident_x = ident_x;
  a.ident_y = ident_y;
  a.out = out;
  a.conf = conf;
  a.channels = channels;
  a.frames = frames;
  a.out_frames = out_frames;
  a.w = w;
  a.clamp_from = clamp_from;
  a.groups = (int)(plane / kGroup);
  const dim3 grid((unsigned)((a.groups + kResampleBlock - 1) / kResampleBlock), (unsigned)out_frames, (unsigned)batch);
  const bool cubic = mode == LFDM_RESAMPLE_CUBIC;
  if (cubic && maps)
    LFDM_LAUNCH((resample_kernel<true, true>), grid, dim3(kResampleBlock), 0, stream, a);
  else if (cubic)
    LFDM_LAUNCH((resample_kernel<true, false>), grid, dim3(kResampleBlock), 0, stream, a);
  else if (maps)
    LFDM_LAUNCH((resample_kernel<false, true>), grid, dim3(kResampleBlock), 0, stream, a);
  else
    LFDM_LAUNCH((resample_kernel<false, false>), grid, dim3(kResampleBlock), 0, stream, a);
  return lfdm_check_launch("latent_resample");
}
