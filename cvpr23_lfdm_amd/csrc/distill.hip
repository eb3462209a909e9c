// Progressive distillation (Salimans & Ho 2022; include/lfdm_hip.h: lfdm_distill_x0_f32, lfdm_distill_step_f32): the frozen
// teacher's DDIM step with a coefficient row PER SAMPLE, and the target that one student step has to reach.
//   distill_x0_kernel              x0 = c_x x - c_eps out, (c_x, c_eps) = coef[row_b][0:2] - the operand of the threshold quantile
//   distill_step_kernel<TARGET>    x0 as above (recomputed, not read back); s = thr ? max(thr[b], 1) : 1; m = clamp(x0, -s, s) / s;
//                                  v = k_x0 m [+ k_eps out] [+ k_x x] -> x_next (the teacher's step; no noise: eta = 0)
//                                  TARGET: xt = q0 v + q1 x_ref -> x_target, et = q2 x_ref + q3 xt -> eps_target, q* = tcoef[trow_b]
//                                  (the student's own row inverted on the teacher's second step, and the noise xt implies at x_ref's level)
// A coefficient that is exactly 0 skips its product, and an operand none of whose coefficients is non-zero is never loaded: it may hold NaN.
// The launch plan is train_elem_core.h's: grid (workgroups of a sample, B), one float4 per lane and load, TD_QUADS loads in flight per lane;
// the row indices and the table values are requested in front of the element loads; a row index is read on the device and clamped to its
// table.  No atomics, no tickets, no workspace, no scratch: every output element has one owner, who reads its inputs before it writes (x_next
// may therefore be x itself).
#include "train_elem_core.h"
#include "../../include/lfdm_hip.h"

// every product and sum rounded on its own: x0 is the eager fp32 expression's bits, and both builds of this file agree
#pragma clang fp contract(off)

namespace {

constexpr int COEF_COLS = 6, TCOEF_COLS = 4;

// c_x x - c_eps out without the product of a zero coefficient ("pred_x0" rows {0, -1}: -(-1 out), the bits of out)
__device__ __forceinline__ float row_x0(float x, float o, float cx, float ce) {
  if (cx == 0.f) return ce == 0.f ? 0.f : -(ce * o);
  return ce == 0.f ? cx * x : cx * x - ce * o;
}

__device__ __forceinline__ float4 row_x0_4(float4 x, float4 o, float cx, float ce) {
  return map4(x, o, [cx, ce](float xe, float oe) { return row_x0(xe, oe, cx, ce); });
}

// (x, x0 not __restrict__: nothing forbids x0 == x, each element is read by its owner before it is written)
__global__ __launch_bounds__(TD_BLOCK) void distill_x0_kernel(const float* x, const float* __restrict__ out, const float* __restrict__ coef,
                                                              const int64_t* __restrict__ row, int rows, float* x0, unsigned n) {
  const unsigned b = blockIdx.y, n4 = n >> 2;
  const size_t off = (size_t)b * n;
  const float* c = coef + (size_t)table_index(row, b, rows) * COEF_COLS;
  const float cx = c[0], ce = c[1];
  const bool use_x = cx != 0.f, use_o = ce != 0.f;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (unsigned q0 = trip_first(); q0 < n4; q0 += trip_stride()) {
    const Trip sl = trip_slots(q0, n4);
    float4 xv[TD_QUADS], ov[TD_QUADS];
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      const size_t at = off + (size_t)sl.q[k] * 4;
      xv[k] = use_x && sl.in[k] ? ld4(x + at) : zero;
      ov[k] = use_o && sl.in[k] ? ld4(out + at) : zero;
    }
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k)
      if (sl.in[k]) st4(x0 + off + (size_t)sl.q[k] * 4, row_x0_4(xv[k], ov[k], cx, ce));
  }
}

struct StepRow {
  float cx, ce, k_x0, k_eps, k_x, s;
};

__device__ __forceinline__ float step_value(float x, float o, const StepRow& r) {
  const float m = fminf(fmaxf(row_x0(x, o, r.cx, r.ce), -r.s), r.s) / r.s;
  float v = r.k_x0 * m;
  if (r.k_eps != 0.f) v += r.k_eps * o;
  if (r.k_x != 0.f) v += r.k_x * x;
  return v;
}

struct TargetOperands {
  const float* x_ref;
  const float* tcoef;
  const int64_t* trow;
  int trows;
  float *x_target, *eps_target;
};

template <bool TARGET>
__global__ __launch_bounds__(TD_BLOCK) void distill_step_kernel(const float* x, const float* __restrict__ out, const float* __restrict__ coef,
                                                                const int64_t* __restrict__ row, int rows, const float* __restrict__ thr,
                                                                float* x_next, TargetOperands tg, unsigned n) {
  const unsigned b = blockIdx.y, n4 = n >> 2;
  const size_t off = (size_t)b * n;
  const float* c = coef + (size_t)table_index(row, b, rows) * COEF_COLS;      // (column 5, the noise scale, is not read: eta = 0)
  StepRow r{c[0], c[1], c[2], c[3], c[4], 1.0f};
  float q0c = 0.f, q1c = 0.f, q2c = 0.f, q3c = 0.f;
  if constexpr (TARGET) {
    const float* q = tg.tcoef + (size_t)table_index(tg.trow, b, tg.trows) * TCOEF_COLS;
    q0c = q[0], q1c = q[1], q2c = q[2], q3c = q[3];
  }
  if (thr) r.s = fmaxf(thr[b], 1.0f);
  const bool use_x = r.cx != 0.f || r.k_x != 0.f, use_o = r.ce != 0.f || r.k_eps != 0.f;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (unsigned q0 = trip_first(); q0 < n4; q0 += trip_stride()) {
    const Trip sl = trip_slots(q0, n4);
    float4 xv[TD_QUADS], ov[TD_QUADS], rv[TD_QUADS];
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      const size_t at = off + (size_t)sl.q[k] * 4;
      xv[k] = use_x && sl.in[k] ? ld4(x + at) : zero;
      ov[k] = use_o && sl.in[k] ? ld4(out + at) : zero;
      if constexpr (TARGET) rv[k] = sl.in[k] ? ld4(tg.x_ref + at) : zero;
    }
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      if (!sl.in[k]) continue;
      const size_t at = off + (size_t)sl.q[k] * 4;
      const float4 v = make_float4(step_value(xv[k].x, ov[k].x, r), step_value(xv[k].y, ov[k].y, r), step_value(xv[k].z, ov[k].z, r),
                                   step_value(xv[k].w, ov[k].w, r));
      if (x_next) st4(x_next + at, v);
      if constexpr (TARGET) {
        const float4 xt = make_float4(q0c * v.x + q1c * rv[k].x, q0c * v.y + q1c * rv[k].y, q0c * v.z + q1c * rv[k].z, q0c * v.w + q1c * rv[k].w);
        st4(tg.x_target + at, xt);
        st4(tg.eps_target + at, make_float4(q2c * rv[k].x + q3c * xt.x, q2c * rv[k].y + q3c * xt.y, q2c * rv[k].z + q3c * xt.z,
                                            q2c * rv[k].w + q3c * xt.w));
      }
    }
  }
}

// The geometry both entries share; 0 or a refusal.
int check_rows(const char* what, int batch, int64_t n, int rows) {
  if (batch <= 0 || batch > 65535 || n <= 0 || n % 4 != 0 || n >= ((int64_t)1 << 24))
    return lfdm_fail(LFDM_EINVAL, "%s: batch in [1, 65535] and n in (0, 2^24) with n %% 4 == 0 are needed, got batch = %d, n = %lld", what, batch, (long long)n);
  if (rows <= 0) return lfdm_fail(LFDM_EINVAL, "%s: a coefficient table of rows > 0 is needed, got %d", what, rows);
  return 0;
}

}  // namespace

extern "C" int lfdm_distill_x0_f32(const float* x, const float* out, const float* coef, const int64_t* row, int rows, float* x0, int batch,
                                   int64_t n, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !out || !coef || !row || !x0 || !lfdm_aligned16(x, out, x0) || !lfdm_aligned<4>(coef) || !lfdm_aligned<8>(row))
    return lfdm_fail(LFDM_EINVAL, "%s", "distill_x0: x, out, x0 (16-byte aligned), the coefficient table and the row index (8-byte aligned) are needed");
  if (const int rc = check_rows("distill_x0", batch, n, rows)) return rc;
  if (x0 == out) return lfdm_fail(LFDM_EINVAL, "%s", "distill_x0: x0 must not alias out");
  const dim3 grid(sample_blocks(n), (unsigned)batch), block(TD_BLOCK);
  LFDM_LAUNCH(distill_x0_kernel, grid, block, 0, stream, x, out, coef, row, rows, x0, (unsigned)n);
  return lfdm_check_launch("distill_x0");
}

extern "C" int lfdm_distill_step_f32(const float* x, const float* out, const float* coef, const int64_t* row, int rows, const float* thr,
                                     float* x_next, const float* x_ref, const float* tcoef, const int64_t* trow, int trows, float* x_target,
                                     float* eps_target, int batch, int64_t n, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x || !out || !coef || !row || !lfdm_aligned16(x, out, x_next, x_ref, x_target, eps_target) || !lfdm_aligned<4>(coef, thr, tcoef) ||
      !lfdm_aligned<8>(row, trow))
    return lfdm_fail(LFDM_EINVAL, "%s", "distill_step: x, out (16-byte aligned, as x_next, x_ref, x_target and eps_target where given), the coefficient "
                                        "table and the row index (8-byte aligned, as trow where given) are needed");
  if (const int rc = check_rows("distill_step", batch, n, rows)) return rc;
  const int given = (x_ref != nullptr) + (tcoef != nullptr) + (trow != nullptr) + (x_target != nullptr) + (eps_target != nullptr);
  if (given != 0 && given != 5)
    return lfdm_fail(LFDM_EINVAL, "%s", "distill_step: x_ref, tcoef, trow, x_target and eps_target go together (all or none)");
  const bool target = given == 5;
  if (target && trows <= 0) return lfdm_fail(LFDM_EINVAL, "distill_step: a target table of trows > 0 is needed, got %d", trows);
  if (!target && trows != 0) return lfdm_fail(LFDM_EINVAL, "distill_step: trows = %d needs the target operands", trows);
  if (!target && !x_next) return lfdm_fail(LFDM_EINVAL, "%s", "distill_step: without the target operands x_next is the only output and is needed");
  if (x_next && x_next == out) return lfdm_fail(LFDM_EINVAL, "%s", "distill_step: x_next must not alias out (it may be x)");
  if (target) {
    if (x_ref == x_next || x_ref == x_target || x_ref == eps_target)
      return lfdm_fail(LFDM_EINVAL, "%s", "distill_step: x_ref must not alias an output (x_next, x_target, eps_target)");
    if (x_target == eps_target || x_target == x_next || eps_target == x_next || x_target == x || eps_target == x || x_target == out ||
        eps_target == out)
      return lfdm_fail(LFDM_EINVAL, "%s", "distill_step: x_target and eps_target must not alias each other, x_next, x or out");
  }
  const dim3 grid(sample_blocks(n), (unsigned)batch), block(TD_BLOCK);
  const TargetOperands tg{x_ref, tcoef, trow, trows, x_target, eps_target};
  if (target) LFDM_LAUNCH(distill_step_kernel<true>, grid, block, 0, stream, x, out, coef, row, rows, thr, x_next, tg, (unsigned)n);
  else LFDM_LAUNCH(distill_step_kernel<false>, grid, block, 0, stream, x, out, coef, row, rows, thr, x_next, tg, (unsigned)n);
  return lfdm_check_launch("distill_step");
}
