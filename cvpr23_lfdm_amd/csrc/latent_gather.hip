// Training latents from a flow-latent store (include/lfdm_hip.h: lfdm_latent_gather_f32): the frozen LFAE's raw outputs of
// every frame of a data set - sampling grid x, grid y, occlusion map - are computed once and kept as a flat (N, 3, h, w) fp32 or fp16
// array; a training batch is a gather of rows from it.  One launch makes the latent (B, 3, T, h, w) the diffusion denoises, by what
// FlowDiffusion._latent_of does to the LFAE's outputs:
//   gather_kernel<HALF>   grid (chunks of the 3 * h * w / 4 quads of a frame, T, B), one thread per 4 adjacent values of one plane
//     channels 0 / 1      v - ident_x[x] / v - ident_y[y] with the identity tables (residual flow), a copy without them
//     channel 2           occ * 2 - 1
// Elementwise and latency-sized: a 16-byte (fp32 store) or 8-byte (fp16 store) load and one 16-byte store per thread, the row number read
// once per workgroup through a uniform address, no atomics, no LDS, nothing that depends on launch order.
#include "lfdm_device.h"
#include "../../include/lfdm_hip.h"

// v - identity and occ * 2 - 1 must be torch's single roundings (occ * 2 is exact, so a fused form would give the same bits anyway)
#pragma clang fp contract(off)

namespace {

constexpr int kGatherBlock = 256;
constexpr int kQuad = 4;                                    // values per thread: one float4

struct alignas(8) Half4 { _Float16 v[kQuad]; };

struct GatherArgs {
  const void* store;                   // (N, 3, h, w) fp32 or fp16
  const int* frame_index;              // (B, T) rows of store
  const float* ident_x;                // (w) or null
  const float* ident_y;                // (h) or null
  float* out;                          // (B, 3, T, h, w)
  int64_t store_frames;
  int frames, w;
  int groups;                          // h * w / 4: quads of one plane
};

template <bool HALF>
__global__ __launch_bounds__(kGatherBlock) void gather_kernel(GatherArgs a) {
  const int q = (int)blockIdx.x * kGatherBlock + (int)threadIdx.x;          // quad of the frame, 0 .. 3 * groups - 1
  const int t = (int)blockIdx.y, b = (int)blockIdx.z;
  // the same for every thread of the workgroup.  The table is device memory the entry point cannot check: the row is clamped into the
  // store here, so a bad table reads a wrong frame, never outside the operand.
  int64_t row = a.frame_index[(int64_t)b * a.frames + t];
  row = row < 0 ? 0 : (row > a.store_frames - 1 ? a.store_frames - 1 : row);
  if (q >= 3 * a.groups) return;
  const int c = q / a.groups, g = q - c * a.groups;
  const int64_t plane = (int64_t)a.groups * kQuad;
  const int64_t src = row * (3 * plane) + (int64_t)q * kQuad;               // in elements of the store: 64-bit, a store passes 4 GiB
  float4 v;
  if (HALF) {
    const Half4 hv = *reinterpret_cast<const Half4*>(static_cast<const _Float16*>(a.store) + src);
    v.x = (float)hv.v[0];                                                   // fp16 -> fp32 is exact
    v.y = (float)hv.v[1];
    v.z = (float)hv.v[2];
    v.w = (float)hv.v[3];
  } else {
    v = *reinterpret_cast<const float4*>(static_cast<const float*>(a.store) + src);
  }
  if (c == 2) {
    v.x = v.x * 2.f - 1.f;
    v.y = v.y * 2.f - 1.f;
    v.z = v.z * 2.f - 1.f;
    v.w = v.w * 2.f - 1.f;
  } else if (a.ident_x) {
    float sub[kQuad];
#pragma unroll
    for (int k = 0; k < kQuad; ++k) {            // h * w % 4 == 0 does not keep the four values in one row
      const int p = g * kQuad + k, y = p / a.w;
      sub[k] = c == 0 ? a.ident_x[p - y * a.w] : a.ident_y[y];
    }
    v.x = v.x - sub[0];
    v.y = v.y - sub[1];
    v.z = v.z - sub[2];
    v.w = v.w - sub[3];
  }
  *reinterpret_cast<float4*>(a.out + (((int64_t)b * 3 + c) * a.frames + t) * plane + (int64_t)g * kQuad) = v;
}

}  // namespace

extern "C" int lfdm_latent_gather_f32(const void* store, int store_dtype, int64_t store_frames, const int* frame_index,
                                      const float* ident_x, const float* ident_y, float* out, int batch, int frames, int h, int w,
                                      lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!store || !frame_index || !out || !lfdm_aligned16(store) || !lfdm_aligned16(out) || !lfdm_aligned<4>(frame_index) ||
      !lfdm_aligned<4>(ident_x) || !lfdm_aligned<4>(ident_y))
    return lfdm_fail(LFDM_EINVAL, "latent_gather: null store / frame_index / out, or store / out not 16-byte aligned");
  if (store_dtype != LFDM_LATENT_F32 && store_dtype != LFDM_LATENT_F16)
    return lfdm_fail(LFDM_EINVAL, "latent_gather: store_dtype is LFDM_LATENT_F32 or LFDM_LATENT_F16");
  if (batch < 1 || frames < 1 || h < 1 || w < 1 || store_frames < 1 || batch > 65535 || frames > 65535)
    return lfdm_fail(LFDM_EINVAL, "latent_gather: batch, frames, h, w, store_frames >= 1, batch and frames <= 65535");
  const int64_t plane = (int64_t)h * w;
  if ((plane & 3) || 3 * plane > 0x7fffffff)
    return lfdm_fail(LFDM_EINVAL, "latent_gather: h * w must be a multiple of 4 (3 * h * w below 2^31)");
  if ((ident_x == nullptr) != (ident_y == nullptr))
    return lfdm_fail(LFDM_EINVAL, "latent_gather: ident_x and ident_y come together (both: residual flow, neither: a copy)");
  GatherArgs a;
  a.store = store;
  a.frame_index = frame_index;
  a.ident_x = ident_x;
  a.ident_y = ident_y;
  a.out = out;
  a.store_frames = store_frames;
  a.frames = frames;
  a.w = w;
  a.groups = (int)(plane / kQuad);
  const dim3 grid((unsigned)((3 * a.groups + kGatherBlock - 1) / kGatherBlock), (unsigned)frames, (unsigned)batch);
  if (store_dtype == LFDM_LATENT_F16)
    LFDM_LAUNCH((gather_kernel<true>), grid, dim3(kGatherBlock), 0, stream, a);
  else
    LFDM_LAUNCH((gather_kernel<false>), grid, dim3(kGatherBlock), 0, stream, a);
  return lfdm_check_launch("latent_gather");
}
