// Fused Adam over one flat fp32 parameter buffer (include/lfdm_hip.h: lfdm_adam_step_f32) - the
// `optimizer_diff.step()` of DM/modules/video_flow_diffusion_model.py:113-114,188 (torch.optim.Adam,
// betas (0.9, 0.99), no amsgrad).  One launch updates all 42.7 M parameters: 16 B/lane streaming reads
// of (p, g, m, v), writes of (p, m, v) - HBM-bound, 28 B per parameter.  grad_scale folds the 1/world
// of the data-parallel gradient average (RCCL all-reduce is a sum) into the same pass.
#include "lfdm_device.h"
#include "../../include/lfdm_hip.h"

namespace {

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                   float lr, float beta1, float beta2, float eps, float weight_decay,
                                                   float bias1, float bias2_sqrt, float grad_scale) {
  const float step_size = lr / bias1;
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float* pp = &pv.x;
    const float* gg = &gv.x;
    float* mm = &mv.x;
    float* vq = &vv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float grad = gg[k] * grad_scale + weight_decay * pp[k];
      mm[k] = beta1 * mm[k] + (1.f - beta1) * grad;
      vq[k] = beta2 * vq[k] + (1.f - beta2) * grad * grad;
      const float denom = sqrtf(vq[k]) / bias2_sqrt + eps;
      pp[k] = pp[k] - step_size * (mm[k] / denom);
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  // tail (n % 4)
  const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) {
    const float grad = g[t] * grad_scale + weight_decay * p[t];
    const float m1 = beta1 * m[t] + (1.f - beta1) * grad;
    const float v1 = beta2 * v[t] + (1.f - beta2) * grad * grad;
    m[t] = m1;
    v[t] = v1;
    p[t] = p[t] - step_size * (m1 / (sqrtf(v1) / bias2_sqrt + eps));
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Guarded step (opt-in: FlatAdam's ema_decay / max_grad_norm / skip_nonfinite): three launches on one stream,
//   sumsq_kernel  (only with clipping or the guard)  g -> one fp32 partial sum of squares per workgroup
//   plan_kernel   (one workgroup)                    partials -> lfdm_optim_plan: apply / clip_coef / bias corrections / EMA decay, counters
//   adam_guarded_kernel                              adam_kernel's arithmetic with the plan's scalars read from DEVICE memory (+ the EMA)
// so the host never waits for the norm.  No floating-point atomics anywhere: the partial of workgroup b is a fixed function of
// (g, n, gridDim) and the plan sums the partials in a fixed order, so every data-parallel rank - which holds the identical all-reduced
// gradient buffer - derives the identical plan and applies the identical update.
constexpr int kOptBlock = 256;               // block4_sum / block_tree_sum (lfdm_device.h) fold four waves / 256 lanes
constexpr int64_t kOptMaxBlocks = 4096;      // adam_kernel's launch geometry

inline int64_t opt_blocks(int64_t n) { return lfdm_blocks(n >> 2, kOptBlock, kOptMaxBlocks); }

// Four accumulators per thread, one per component of the 16-byte load; thread t of workgroup b adds the float4s t + 256 b + k * 256 * grid
// in order of k, so each accumulator is a chain of L = ceil((n / 4) / (256 * grid)) fused multiply-adds (+ 1 in workgroup 0's first lanes
// for the n % 4 tail).  Then (a0 + a1) + (a2 + a3), a 6-level wave butterfly and (w0 + w1) + (w2 + w3) through LDS: 8 tree levels.
__global__ __launch_bounds__(kOptBlock) void sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partials) {
  __shared__ float wave_part[kOptBlock / LFDM_WAVE];
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kOptBlock;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int64_t i = (int64_t)blockIdx.x * kOptBlock + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {      // four loads in flight; the sums stay in order of i
    const float4 x0 = g4[i], x1 = g4[i + stride], x2 = g4[i + 2 * stride], x3 = g4[i + 3 * stride];
    a0 = fmaf(x0.x, x0.x, a0); a1 = fmaf(x0.y, x0.y, a1); a2 = fmaf(x0.z, x0.z, a2); a3 = fmaf(x0.w, x0.w, a3);
    a0 = fmaf(x1.x, x1.x, a0); a1 = fmaf(x1.y, x1.y, a1); a2 = fmaf(x1.z, x1.z, a2); a3 = fmaf(x1.w, x1.w, a3);
    a0 = fmaf(x2.x, x2.x, a0); a1 = fmaf(x2.y, x2.y, a1); a2 = fmaf(x2.z, x2.z, a2); a3 = fmaf(x2.w, x2.w, a3);
    a0 = fmaf(x3.x, x3.x, a0); a1 = fmaf(x3.y, x3.y, a1); a2 = fmaf(x3.z, x3.z, a2); a3 = fmaf(x3.w, x3.w, a3);
  }
  for (; i < n4; i += stride) {
    const float4 x = g4[i];
    a0 = fmaf(x.x, x.x, a0); a1 = fmaf(x.y, x.y, a1); a2 = fmaf(x.z, x.z, a2); a3 = fmaf(x.w, x.w, a3);
  }
  const int64_t t = (n4 << 2) + threadIdx.x;           // tail (n % 4): the first lanes of workgroup 0
  if (blockIdx.x == 0 && t < n) a0 = fmaf(g[t], g[t], a0);
  const float s = block4_sum(wave_sum((a0 + a1) + (a2 + a3)), wave_part);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// include/lfdm_hip.h: lfdm_optim_plan (64 bytes, 16-byte aligned)
struct OptimPlan {
  int32_t apply, reserved0;
  float clip_coef, total_norm, bias1, bias2_sqrt, ema_decay, ema_one_minus_decay;
  int64_t applied_steps, skipped_steps;
  int32_t reserved1[4];
};
static_assert(sizeof(OptimPlan) == LFDM_OPTIM_PLAN_BYTES, "lfdm_optim_plan layout");

// One workgroup.  Thread t sums partials t, t + 256, ... in fp64, then a fixed LDS tree: a fixed order whatever the hardware does.
__global__ __launch_bounds__(kOptBlock) void plan_kernel(const float* __restrict__ partials, int n_partials, OptimPlan* __restrict__ plan,
                                                         float grad_scale, float max_grad_norm, int skip_nonfinite, float beta1, float beta2,
                                                         double ema_decay, int64_t ema_start_step) {
  __shared__ double part[kOptBlock];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += kOptBlock) s += (double)partials[i];
  part[threadIdx.x] = s;
  block_tree_sum(part);
  if (threadIdx.x != 0) return;
  const double total_norm = (double)grad_scale * sqrt(part[0]);          // 0 when no norm pass ran (n_partials == 0)
  const bool finite = total_norm == total_norm && total_norm <= 3.4028234663852886e38;      // (inf or nan: not finite)
  const int apply = (skip_nonfinite && !finite) ? 0 : 1;
  double coef = 1.0;
  if (max_grad_norm >= 0.f) {                                            // torch.nn.utils.clip_grad_norm_
    coef = (double)max_grad_norm / (total_norm + 1e-6);
    if (coef > 1.0) coef = 1.0;                                          // (a nan norm leaves a nan coefficient, as torch does)
  }
  const int64_t step = plan->applied_steps + 1;                          // the step this launch sequence applies, if it does
  // bias corrections in double, like lfdm_adam_step_f32 on the host
  const double b1 = 1.0 - pow((double)beta1, (double)step);
  const double b2 = sqrt(1.0 - pow((double)beta2, (double)step));
  const double d = (ema_decay >= 0.0 && step > ema_start_step) ? ema_decay : 0.0;      // before ema_start_step the average IS the parameters
  plan->apply = apply;
  plan->clip_coef = (float)coef;
  plan->total_norm = (float)total_norm;
  plan->bias1 = (float)b1;
  plan->bias2_sqrt = (float)b2;
  plan->ema_decay = (float)d;
  plan->ema_one_minus_decay = (float)(1.0 - d);
  if (apply) plan->applied_steps = step;
  else plan->skipped_steps = plan->skipped_steps + 1;
}

// adam_kernel with  grad = g * grad_scale * clip_coef + weight_decay * p,  ema = d * ema + (1 - d) * p_new  in the same pass (EMA:
// 36 B per parameter instead of 28), and nothing at all when the plan says skip.  g is only read: p.grad keeps the unclipped gradient.
template <bool EMA>
__global__ __launch_bounds__(kOptBlock) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                 float* __restrict__ v, float* __restrict__ ema, int64_t n, float lr,
                                                                 float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                                                 const OptimPlan* __restrict__ plan) {
  if (plan->apply == 0) return;
  const float clip_coef = plan->clip_coef, bias2_sqrt = plan->bias2_sqrt;
  const float step_size = lr / plan->bias1;
  const float d = plan->ema_decay, omd = plan->ema_one_minus_decay;
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * kOptBlock + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kOptBlock) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 ev = make_float4(0.f, 0.f, 0.f, 0.f);
    if (EMA) ev = reinterpret_cast<float4*>(ema)[i];
    float* pp = &pv.x;
    const float* gg = &gv.x;
    float* mm = &mv.x;
    float* vq = &vv.x;
    float* ee = &ev.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float grad = gg[k] * grad_scale * clip_coef + weight_decay * pp[k];
      mm[k] = beta1 * mm[k] + (1.f - beta1) * grad;
      vq[k] = beta2 * vq[k] + (1.f - beta2) * grad * grad;
      const float denom = sqrtf(vq[k]) / bias2_sqrt + eps;
      pp[k] = pp[k] - step_size * (mm[k] / denom);
      if (EMA) ee[k] = d * ee[k] + omd * pp[k];      // d = 0, omd = 1 before ema_start_step: exactly p_new
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (EMA) reinterpret_cast<float4*>(ema)[i] = ev;
  }
  // tail (n % 4)
  const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * kOptBlock + threadIdx.x;
  if (t < n) {
    const float grad = g[t] * grad_scale * clip_coef + weight_decay * p[t];
    const float m1 = beta1 * m[t] + (1.f - beta1) * grad;
    const float v1 = beta2 * v[t] + (1.f - beta2) * grad * grad;
    m[t] = m1;
    v[t] = v1;
    const float p1 = p[t] - step_size * (m1 / (sqrtf(v1) / bias2_sqrt + eps));
    p[t] = p1;
    if (EMA) ema[t] = d * ema[t] + omd * p1;
  }
}

}  // namespace

extern "C" size_t lfdm_grad_sumsq_ws_bytes(int64_t n) { return n > 0 ? (size_t)opt_blocks(n) * sizeof(float) : 0; }

extern "C" int lfdm_grad_sumsq_f32(const float* grad, int64_t n, float* partials, size_t partials_bytes, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!grad || !partials || n <= 0 || !lfdm_aligned16(grad) || !lfdm_aligned<4>(partials) ||
      partials_bytes < lfdm_grad_sumsq_ws_bytes(n))
    return lfdm_fail(LFDM_EINVAL, "grad_sumsq: bad arguments (16-byte aligned gradient, n > 0, partials of lfdm_grad_sumsq_ws_bytes(n))");
  LFDM_LAUNCH(sumsq_kernel, dim3((unsigned)opt_blocks(n)), dim3(kOptBlock), 0, stream, grad, n, partials);
  return lfdm_check_launch("grad_sumsq");
}

extern "C" int lfdm_optim_plan_f32(const float* partials, int n_partials, void* plan, size_t plan_bytes, float grad_scale,
                                   float max_grad_norm, int skip_nonfinite, float beta1, float beta2, double ema_decay,
                                   int64_t ema_start_step, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!plan || !lfdm_aligned16(plan) || plan_bytes < LFDM_OPTIM_PLAN_BYTES || n_partials < 0 || n_partials > kOptMaxBlocks ||
      (n_partials > 0 && !partials) || ema_decay > 1.0 || ema_start_step < 0)
    return lfdm_fail(LFDM_EINVAL, "optim_plan: bad arguments (16-byte aligned plan of LFDM_OPTIM_PLAN_BYTES, 0 <= n_partials <= 4096, ema_decay <= 1)");
  if (n_partials == 0 && (max_grad_norm >= 0.f || skip_nonfinite))
    return lfdm_fail(LFDM_EINVAL, "optim_plan: clipping and the non-finite guard need the partials of lfdm_grad_sumsq_f32");
  LFDM_LAUNCH(plan_kernel, dim3(1), dim3(kOptBlock), 0, stream, partials, n_partials, (OptimPlan*)plan, grad_scale, max_grad_norm,
              skip_nonfinite, beta1, beta2, ema_decay, ema_start_step);
  return lfdm_check_launch("optim_plan");
}

extern "C" int lfdm_adam_guarded_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                          float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                          const void* plan, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!param || !grad || !exp_avg || !exp_avg_sq || !plan || n <= 0 ||
      !lfdm_aligned16(param, grad, exp_avg, exp_avg_sq, ema, plan))
    return lfdm_fail(LFDM_EINVAL, "adam_guarded: bad arguments (16-byte aligned flat buffers and plan, n > 0)");
  const dim3 grid((unsigned)opt_blocks(n));
  const OptimPlan* pl = (const OptimPlan*)plan;
  if (ema)
    LFDM_LAUNCH(adam_guarded_kernel<true>, grid, dim3(kOptBlock), 0, stream, param, grad, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps,
                weight_decay, grad_scale, pl);
  else
    LFDM_LAUNCH(adam_guarded_kernel<false>, grid, dim3(kOptBlock), 0, stream, param, grad, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps,
                weight_decay, grad_scale, pl);
  return lfdm_check_launch("adam_guarded");
}

extern "C" int lfdm_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                  float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                  float grad_scale, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step < 1 ||
      !lfdm_aligned16(param, grad, exp_avg, exp_avg_sq))
    return lfdm_fail(LFDM_EINVAL, "adam: bad arguments (16-byte aligned flat buffers, step >= 1)");
  // bias corrections in double on the host, like torch.optim.Adam's scalar path
  const double b1 = 1.0 - pow((double)beta1, (double)step);
  const double b2 = sqrt(1.0 - pow((double)beta2, (double)step));
  LFDM_LAUNCH(adam_kernel, dim3(lfdm_blocks(n >> 2, 256, 4096)), dim3(256), 0, stream, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2,
              eps, weight_decay, (float)b1, (float)b2, grad_scale);
  return lfdm_check_launch("adam");
}
