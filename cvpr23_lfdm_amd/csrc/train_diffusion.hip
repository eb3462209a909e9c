// The diffusion edge of the DM training step (include/lfdm_hip.h: lfdm_train_qsample_f32, lfdm_objective_loss_fwd_f32,
// lfdm_objective_loss_bwd_f32 over one lfdm_train_loss_params).  Random-mask training (RaMViD, Hoeppe et al. 2022):
// some frames or elements of x_start stay clean inside x_noisy, the loss counts the unknown elements only.
//   train_qsample_kernel<MASK>             x_noisy = known ? x_start : a[t_b] * x_start + s[t_b] * noise
//   objective_loss_fwd_kernel<OBJ,MASK,L2> S_b = sum_unknown |target - out| (or its square), N_b = the unknown count, pred_x0 (known: x_noisy)
//                                          in the same pass; the last workgroup folds the partials: inv_count[b] = 1 / max(N_b, 1),
//                                          sample_loss[b] = S_b / max(N_b, 1), loss = (1 / B) sum_b w[t_b] S_b / max(N_b, 1)
//   objective_loss_bwd_kernel<OBJ,MASK,L2> dout = -sign(target - out) * c_b (l2: 2 (out - target) in place of the sign), known: 0.f
// OBJ: the training objective (the noise, x0 or v: the table below); the masked loss of 4.12 is OBJ_NOISE without a weight table.
// MASK: 0 none, 1 one byte per frame (B, frames), 2 one byte per element (B, n) - the forms of the sampler's known operands (sampler.hip).
// All three: grid (workgroups of a sample, B), one float4 per lane and load, TD_QUADS loads in flight per lane, at most TD_CAP workgroups per
// sample (the grid-stride loop takes a second trip above TD_CAP * TD_QUADS * 256 float4 = 262 144 floats per sample).  t, the table values
// and the first mask bytes are requested in front of the element loads; t is read on the device and clamped to the table (no host read, no
// address outside the table whatever t holds).  No floating-point atomics, one owner per output element, no scratch.
// The reduction (lfdm_device.h, "In-launch hand-off between workgroups", single-writer form): a lane sums the 16 terms of one trip in fp32 (pairwise
// inside a float4, then a chain of four) and adds that to a double; lanes -> workgroup by a fixed tree of doubles in LDS; workgroup partials
// (S and N as doubles) are 8-byte agent-scope words; the workgroup that takes the last ticket folds each sample's partials in index order
// and the samples in index order, in double.  Two runs on the same inputs give the same bits.
#include "train_elem_core.h"
#include "../../include/lfdm_hip.h"

// a * x_start + s * noise and r * x_noisy - m * pred are torch's expressions: two products and one sum, each rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int MASK_NONE = 0, MASK_FRAME = 1, MASK_ELEM = 2;

struct TrainMask {
  const unsigned char* mask;         // MASK_FRAME: (B, frames); MASK_ELEM: (B, n); non-zero = known
  unsigned frames, frame_elems;      // MASK_FRAME only; frame_elems % 4 == 0: a float4 never straddles two frames
};

// the four known flags (bit k: element i + k) of the float4 at element i of sample b
template <int MASK>
__device__ __forceinline__ unsigned known_bits(const TrainMask& m, unsigned b, unsigned n, unsigned i) {
  if constexpr (MASK == MASK_FRAME) {
    return m.mask[(size_t)b * m.frames + (i / m.frame_elems) % m.frames] ? 0xFu : 0u;
  } else if constexpr (MASK == MASK_ELEM) {
    const unsigned w = *reinterpret_cast<const unsigned*>(m.mask + (size_t)b * n + i);
    return ((w & 0xFFu) ? 1u : 0u) | ((w & 0xFF00u) ? 2u : 0u) | ((w & 0xFF0000u) ? 4u : 0u) | ((w & 0xFF000000u) ? 8u : 0u);
  } else {
    return 0u;
  }
}

template <int MASK>
__global__ __launch_bounds__(TD_BLOCK) void train_qsample_kernel(const float* __restrict__ x_start, const float* __restrict__ noise,
                                                                 const int64_t* __restrict__ t, const float* __restrict__ a_tab,
                                                                 const float* __restrict__ s_tab, int t_len, TrainMask m,
                                                                 float* __restrict__ x_noisy, unsigned n) {
  const unsigned b = blockIdx.y, n4 = n >> 2;
  const size_t off = (size_t)b * n;
  const int ti = table_index(t, b, t_len);
  const float a = a_tab[ti], s = s_tab[ti];
  for (unsigned q0 = trip_first(); q0 < n4; q0 += trip_stride()) {
    const Trip sl = trip_slots(q0, n4);
    unsigned kb[TD_QUADS];
    float4 x0[TD_QUADS], z[TD_QUADS];
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) kb[k] = sl.in[k] ? known_bits<MASK>(m, b, n, sl.q[k] * 4u) : 0u;
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      x0[k] = ld4_if(sl.in[k], x_start, off + (size_t)sl.q[k] * 4);
      z[k] = ld4_if(sl.in[k], noise, off + (size_t)sl.q[k] * 4);
    }
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      if (!sl.in[k]) continue;
      st4(x_noisy + off + (size_t)sl.q[k] * 4, select4(kb[k], x0[k], map4(x0[k], z[k], [a, s](float x, float e) { return a * x + s * e; })));
    }
  }
}

static_assert(TD_BLOCK == 256, "block_tree_sum (lfdm_device.h) folds 256 lanes");

template <bool L2>
__device__ __forceinline__ float loss_term(float tg, float pr) {
  const float d = tg - pr;
  return L2 ? d * d : fabsf(d);
}

// ---- training objectives: what the denoiser's output `out` is compared with, and how x0 comes back from it
//   OBJ_NOISE  target = noise                        pred_x0 = r * x_noisy - m * out
//   OBJ_X0     target = x_start                      pred_x0 = out
//   OBJ_V      target = a * noise - s * x_start      pred_x0 = a * x_noisy - s * out      (Salimans & Ho 2022)
// The target lives in registers only.  An operand the objective does not use is never loaded (it may be null).
constexpr int OBJ_NOISE = LFDM_OBJ_NOISE, OBJ_X0 = LFDM_OBJ_X0, OBJ_V = LFDM_OBJ_V;

struct ObjTables {
  const float *a, *s, *r, *m, *w;    // w: the per-timestep loss weight, null = 1
  int len;
};

template <int OBJ>
__device__ __forceinline__ float obj_target(float x0, float z, float a, float s) {
  if constexpr (OBJ == OBJ_NOISE) return z;
  else if constexpr (OBJ == OBJ_X0) return x0;
  else return a * z - s * x0;
}

// (cx, ce): (r, m) for OBJ_NOISE, (a, s) for OBJ_V
template <int OBJ>
__device__ __forceinline__ float obj_pred_x0(float xn, float o, float cx, float ce) {
  if constexpr (OBJ == OBJ_X0) return o;
  else return cx * xn - ce * o;
}

template <int OBJ>
__device__ __forceinline__ float4 obj_target4(float4 x0, float4 z, float a, float s) {
  return map4(x0, z, [a, s](float x, float e) { return obj_target<OBJ>(x, e, a, s); });
}

template <int OBJ, int MASK, bool L2>
__global__ __launch_bounds__(TD_BLOCK) void objective_loss_fwd_kernel(const float* __restrict__ x_start, const float* __restrict__ noise,
                                                                      const float* __restrict__ out, const float* __restrict__ x_noisy,
                                                                      const int64_t* __restrict__ t, ObjTables tab, TrainMask m,
                                                                      float* __restrict__ loss, float* __restrict__ inv_count,
                                                                      float* __restrict__ sample_loss, float* __restrict__ pred_x0, unsigned n,
                                                                      unsigned long long* part, unsigned* ticket) {
  constexpr bool USE_X0 = OBJ != OBJ_NOISE, USE_Z = OBJ != OBJ_X0, USE_XN = OBJ != OBJ_X0 || MASK != MASK_NONE;
  __shared__ double s_sum[TD_BLOCK];
  __shared__ double s_cnt[TD_BLOCK];
  __shared__ unsigned s_last;
  const unsigned b = blockIdx.y, n4 = n >> 2;
  const size_t off = (size_t)b * n;
  const int ti = table_index(t, b, tab.len);
  float a = 0.f, s = 0.f, cx = 0.f, ce = 0.f;
  if constexpr (OBJ == OBJ_V) { a = tab.a[ti]; s = tab.s[ti]; cx = a; ce = s; }
  if constexpr (OBJ == OBJ_NOISE) { cx = tab.r[ti]; ce = tab.m[ti]; }
  double acc = 0.0;
  unsigned unknown = 0;
  for (unsigned q0 = trip_first(); q0 < n4; q0 += trip_stride()) {
    const Trip sl = trip_slots(q0, n4);
    unsigned kb[TD_QUADS];
    float4 x0[TD_QUADS], nz[TD_QUADS], pr[TD_QUADS], xn[TD_QUADS];
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) kb[k] = sl.in[k] ? known_bits<MASK>(m, b, n, sl.q[k] * 4u) : 0xFu;     // (outside the sample: counts as known)
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {      // (written out: ld4_if or a shared address costs the frame-mask form a wave of occupancy)
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      x0[k] = USE_X0 && sl.in[k] ? ld4(x_start + off + (size_t)sl.q[k] * 4) : zero;
      nz[k] = USE_Z && sl.in[k] ? ld4(noise + off + (size_t)sl.q[k] * 4) : zero;
      pr[k] = sl.in[k] ? ld4(out + off + (size_t)sl.q[k] * 4) : zero;
      xn[k] = USE_XN && sl.in[k] ? ld4(x_noisy + off + (size_t)sl.q[k] * 4) : zero;
    }
    float trip = 0.f;       // 16 terms: pairwise inside a float4, a chain over the four
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      const float4 e = select4(kb[k], make_float4(0.f, 0.f, 0.f, 0.f), map4(obj_target4<OBJ>(x0[k], nz[k], a, s), pr[k], loss_term<L2>));
      trip += (e.x + e.y) + (e.z + e.w);
      unknown += 4u - (unsigned)__builtin_popcount(kb[k]);
      if (!sl.in[k]) continue;
      st4(pred_x0 + off + (size_t)sl.q[k] * 4,
          select4(kb[k], xn[k], map4(xn[k], pr[k], [cx, ce](float x, float o) { return obj_pred_x0<OBJ>(x, o, cx, ce); })));
    }
    acc += (double)trip;
  }
  s_sum[threadIdx.x] = acc;
  s_cnt[threadIdx.x] = (double)unknown;
  block_tree_sum(s_sum);
  block_tree_sum(s_cnt);
  // (partials as 8-byte agent-scope words, one writer per workgroup who drains before the ticket: lfdm_device.h, "In-launch hand-off
  // between workgroups")
  const unsigned nbx = gridDim.x, nblocks = gridDim.x * gridDim.y;
  unsigned long long* part_cnt = part + (size_t)nblocks;
  if (threadIdx.x == 0) {
    lfdm_agent_store_u64(part + (size_t)b * nbx + blockIdx.x, __builtin_bit_cast(unsigned long long, s_sum[0]));
    lfdm_agent_store_u64(part_cnt + (size_t)b * nbx + blockIdx.x, __builtin_bit_cast(unsigned long long, s_cnt[0]));
    LFDM_DRAIN_STORES();
  }
  if (!lfdm_workgroup_last(ticket, nblocks, &s_last)) return;
  // the last workgroup: one lane per sample folds the sample's partials in index order and applies the weight of its timestep in double,
  // then the samples in a fixed tree
  const unsigned batch = gridDim.y;
  double mine = 0.0;
  for (unsigned bb = threadIdx.x; bb < batch; bb += TD_BLOCK) {
    double sum = 0.0, cnt = 0.0;
    for (unsigned j = 0; j < nbx; ++j) {
      sum += __builtin_bit_cast(double, lfdm_agent_load_u64(part + (size_t)bb * nbx + j));
      cnt += __builtin_bit_cast(double, lfdm_agent_load_u64(part_cnt + (size_t)bb * nbx + j));
    }
    const double inv = 1.0 / (cnt < 1.0 ? 1.0 : cnt);
    inv_count[bb] = (float)inv;
    sample_loss[bb] = (float)(sum * inv);      // unweighted
    if (tab.w) mine += (double)tab.w[table_index(t, bb, tab.len)] * sum * inv;
    else mine += sum * inv;
  }
  s_sum[threadIdx.x] = mine;
  block_tree_sum(s_sum);
  if (threadIdx.x == 0) *loss = (float)(s_sum[0] / (double)batch);
}

// dout = c_b * d term / d out, c_b = ((g * inv_count[b]) * w[t_b]) / B in fp32 in that order (null w: no product); the target is recomputed
// from x_start / noise; known: 0.f.  t is read only where a table is: OBJ_V, or with weights.
template <int OBJ, int MASK, bool L2>
__global__ __launch_bounds__(TD_BLOCK) void objective_loss_bwd_kernel(const float* __restrict__ x_start, const float* __restrict__ noise,
                                                                      const float* __restrict__ out, const int64_t* __restrict__ t,
                                                                      ObjTables tab, TrainMask m, const float* __restrict__ inv_count,
                                                                      const float* __restrict__ gout, float* __restrict__ dout, unsigned n) {
  constexpr bool USE_X0 = OBJ != OBJ_NOISE, USE_Z = OBJ != OBJ_X0;
  const unsigned b = blockIdx.y, n4 = n >> 2;
  const size_t off = (size_t)b * n;
  const int ti = OBJ == OBJ_V || tab.w ? table_index(t, b, tab.len) : 0;
  float a = 0.f, s = 0.f;
  if constexpr (OBJ == OBJ_V) { a = tab.a[ti]; s = tab.s[ti]; }
  float c = *gout * inv_count[b];
  if (tab.w) c = c * tab.w[ti];
  c = c / (float)gridDim.y;
  for (unsigned q0 = trip_first(); q0 < n4; q0 += trip_stride()) {
    const Trip sl = trip_slots(q0, n4);
    unsigned kb[TD_QUADS];
    float4 x0[TD_QUADS], nz[TD_QUADS], pr[TD_QUADS];
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) kb[k] = sl.in[k] ? known_bits<MASK>(m, b, n, sl.q[k] * 4u) : 0u;
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      x0[k] = ld4_if(USE_X0 && sl.in[k], x_start, off + (size_t)sl.q[k] * 4);
      nz[k] = ld4_if(USE_Z && sl.in[k], noise, off + (size_t)sl.q[k] * 4);
      pr[k] = ld4_if(sl.in[k], out, off + (size_t)sl.q[k] * 4);
    }
    auto grad = [c](float z, float p) {
      if constexpr (L2) return (2.f * (p - z)) * c;
      else return z > p ? -c : (z < p ? c : 0.f);
    };
#pragma unroll
    for (int k = 0; k < TD_QUADS; ++k) {
      if (!sl.in[k]) continue;
      st4(dout + off + (size_t)sl.q[k] * 4,
          select4(kb[k], make_float4(0.f, 0.f, 0.f, 0.f), map4(obj_target4<OBJ>(x0[k], nz[k], a, s), pr[k], grad)));
    }
  }
}

// The one check of the geometry and the mask operands (a null `mk`: no mask); -> MASK_* or a refusal.
int check_mask(const char* what, int batch, int64_t n, const lfdm_train_mask* mk, TrainMask& m) {
  const lfdm_train_mask none{nullptr, nullptr, 0, 0};
  const lfdm_train_mask& k = mk ? *mk : none;
  if (batch <= 0 || batch > 65535 || n <= 0 || n % 4 != 0 || n >= ((int64_t)1 << 31))
    return lfdm_fail(LFDM_EINVAL, "%s: batch in [1, 65535] and n in (0, 2^31) with n %% 4 == 0 are needed, got batch = %d, n = %lld", what, batch, (long long)n);
  if (k.frame_mask && k.elem_mask)
    return lfdm_fail(LFDM_EINVAL, "%s: frame_mask and elem_mask exclude each other", what);
  m = TrainMask{nullptr, 0u, 0u};
  if (!k.frame_mask) {
    if (k.frames != 0 || k.frame_elems != 0)
      return lfdm_fail(LFDM_EINVAL, "%s: a frame split (frames = %d, frame_elems = %lld) needs frame_mask", what, k.frames, (long long)k.frame_elems);
    if (!k.elem_mask) return MASK_NONE;
    if (!lfdm_aligned<4>(k.elem_mask))
      return lfdm_fail(LFDM_EINVAL, "%s: elem_mask must be 4-byte aligned", what);
    m.mask = k.elem_mask;
    return MASK_ELEM;
  }
  if (k.frames <= 0 || k.frame_elems <= 0 || k.frame_elems % 4 != 0 || k.frames > n || k.frame_elems > n ||
      n % ((int64_t)k.frames * k.frame_elems) != 0)
    return lfdm_fail(LFDM_EINVAL, "%s: n = %lld must be a multiple of frames * frame_elems = %d * %lld, frame_elems a multiple of 4", what, (long long)n,
                     k.frames, (long long)k.frame_elems);
  m = TrainMask{k.frame_mask, (unsigned)k.frames, (unsigned)k.frame_elems};
  return MASK_FRAME;
}

// f(MASK as an integral constant) for the checked form
template <class F>
void with_mask(int form, F&& f) {
  if (form == MASK_ELEM) f(std::integral_constant<int, MASK_ELEM>{});
  else if (form == MASK_FRAME) f(std::integral_constant<int, MASK_FRAME>{});
  else f(std::integral_constant<int, MASK_NONE>{});
}

template <class F>
void with_objective(int objective, F&& f) {
  if (objective == OBJ_V) f(std::integral_constant<int, OBJ_V>{});
  else if (objective == OBJ_X0) f(std::integral_constant<int, OBJ_X0>{});
  else f(std::integral_constant<int, OBJ_NOISE>{});
}

template <class F>
void with_loss_type(int loss_type, F&& f) {
  if (loss_type == LFDM_LOSS_L2) f(std::true_type{});
  else f(std::false_type{});
}

// Everything a loss call is refused for, in one place: pointers and alignment, the objective and the operands it needs (the forward's
// pred_x0 also r_tab and m_tab), loss_type, geometry and mask, and the forward's workspace; -> MASK_* or a refusal.
int check_loss_call(const char* what, const lfdm_train_loss_params* p, bool forward, TrainMask& m) {
  if (!p) return lfdm_fail(LFDM_EINVAL, "%s: the parameter struct is needed", what);
  const bool reads_t = forward || p->objective == OBJ_V || p->w_tab;      // (the backward reads t only where it reads a table)
  const bool common = p->out && (!reads_t || (p->t && p->t_len > 0)) && p->inv_count && lfdm_aligned16(p->x_start, p->noise, p->out) &&
                      lfdm_aligned<8>(p->t);
  if (forward) {
    if (!common || !p->x_noisy || !p->loss || !p->sample_loss || !p->pred_x0 || !p->ws || !p->ticket || !lfdm_aligned16(p->x_noisy, p->pred_x0) ||
        !lfdm_aligned<8>(p->ws))
      return lfdm_fail(LFDM_EINVAL, "%s: out, x_noisy, pred_x0 (16-byte aligned, as x_start and noise where given), t, a table length > 0, loss, "
                                    "inv_count, sample_loss, a workspace (8-byte aligned) and one zeroed ticket word are needed", what);
  } else if (!common || !p->gout || !p->dout || !lfdm_aligned16(p->dout)) {
    return lfdm_fail(LFDM_EINVAL, "%s: out, dout (16-byte aligned, as x_start and noise where given), t, a table length > 0, inv_count and gout "
                                  "are needed", what);
  }
  const int obj = p->objective;
  const bool ok = obj == OBJ_NOISE ? p->noise && (!forward || (p->r_tab && p->m_tab))
                : obj == OBJ_X0    ? p->x_start != nullptr
                : obj == OBJ_V     ? p->x_start && p->noise && p->a_tab && p->s_tab
                                   : false;
  if (!ok && obj != OBJ_NOISE && obj != OBJ_X0 && obj != OBJ_V)
    return lfdm_fail(LFDM_EINVAL, "%s: objective must be LFDM_OBJ_NOISE (0), LFDM_OBJ_X0 (1) or LFDM_OBJ_V (2), got %d", what, obj);
  if (!ok)
    return lfdm_fail(LFDM_EINVAL, "%s: objective %d lacks an operand - LFDM_OBJ_NOISE needs noise%s, LFDM_OBJ_X0 needs x_start, LFDM_OBJ_V needs "
                                  "x_start, noise, a_tab and s_tab", what, obj, forward ? ", r_tab and m_tab" : "");
  if (p->loss_type != LFDM_LOSS_L1 && p->loss_type != LFDM_LOSS_L2)
    return lfdm_fail(LFDM_EINVAL, "%s: loss_type must be LFDM_LOSS_L1 (0) or LFDM_LOSS_L2 (1), got %d", what, p->loss_type);
  const int form = check_mask(what, p->batch, p->n, &p->mask, m);
  if (form >= 0 && forward && p->ws_bytes < lfdm_masked_loss_ws_bytes(p->batch, p->n))
    return lfdm_fail(LFDM_EWORKSPACE, "%s: workspace of %zu bytes, lfdm_masked_loss_ws_bytes asks for %zu", what, p->ws_bytes,
                     lfdm_masked_loss_ws_bytes(p->batch, p->n));
  return form;
}

}  // namespace

extern "C" int lfdm_train_qsample_f32(const float* x_start, const float* noise, const int64_t* t, const float* a_tab, const float* s_tab, int t_len,
                                      const lfdm_train_mask* mask, float* x_noisy, int batch, int64_t n, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!x_start || !noise || !t || !a_tab || !s_tab || !x_noisy || t_len <= 0 || !lfdm_aligned16(x_start, noise, x_noisy) || !lfdm_aligned<8>(t))
    return lfdm_fail(LFDM_EINVAL, "%s", "train_qsample: x_start, noise, x_noisy (16-byte aligned), t, both tables and a table length > 0 are needed");
  TrainMask m;
  const int form = check_mask("train_qsample", batch, n, mask, m);
  if (form < 0) return form;
  const dim3 grid(sample_blocks(n), (unsigned)batch), block(TD_BLOCK);
  with_mask(form, [&](auto mk) {
    LFDM_LAUNCH(train_qsample_kernel<decltype(mk)::value>, grid, block, 0, stream, x_start, noise, t, a_tab, s_tab, t_len, m, x_noisy, (unsigned)n);
  });
  return lfdm_check_launch("train_qsample");
}

extern "C" size_t lfdm_masked_loss_ws_bytes(int batch, int64_t n) {
  if (batch <= 0 || n <= 0) return 0;
  return (size_t)batch * sample_blocks(n) * 2 * sizeof(unsigned long long);
}

extern "C" int lfdm_objective_loss_fwd_f32(const lfdm_train_loss_params* p, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TrainMask m;
  const int form = check_loss_call("objective_loss_fwd", p, true, m);
  if (form < 0) return form;
  const ObjTables tab{p->a_tab, p->s_tab, p->r_tab, p->m_tab, p->w_tab, p->t_len};
  const dim3 grid(sample_blocks(p->n), (unsigned)p->batch), block(TD_BLOCK);
  with_objective(p->objective, [&](auto obj) {
    with_mask(form, [&](auto mk) {
      with_loss_type(p->loss_type, [&](auto l2) {
        LFDM_LAUNCH((objective_loss_fwd_kernel<decltype(obj)::value, decltype(mk)::value, decltype(l2)::value>), grid, block, 0, stream, p->x_start,
                    p->noise, p->out, p->x_noisy, p->t, tab, m, p->loss, p->inv_count, p->sample_loss, p->pred_x0, (unsigned)p->n,
                    reinterpret_cast<unsigned long long*>(p->ws), p->ticket);
      });
    });
  });
  return lfdm_check_launch("objective_loss_fwd");
}

extern "C" int lfdm_objective_loss_bwd_f32(const lfdm_train_loss_params* p, lfdm_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TrainMask m;
  const int form = check_loss_call("objective_loss_bwd", p, false, m);
  if (form < 0) return form;
  const ObjTables tab{p->a_tab, p->s_tab, nullptr, nullptr, p->w_tab, p->t_len};
  const dim3 grid(sample_blocks(p->n), (unsigned)p->batch), block(TD_BLOCK);
  with_objective(p->objective, [&](auto obj) {
    with_mask(form, [&](auto mk) {
      with_loss_type(p->loss_type, [&](auto l2) {
        LFDM_LAUNCH((objective_loss_bwd_kernel<decltype(obj)::value, decltype(mk)::value, decltype(l2)::value>), grid, block, 0, stream, p->x_start,
                    p->noise, p->out, p->t, tab, m, p->inv_count, p->gout, p->dout, (unsigned)p->n);
      });
    });
  });
  return lfdm_check_launch("objective_loss_bwd");
}
