// Device-side helpers shared by every kernel file: wavefront-64 shuffles, the two fp32 MFMA
// shapes of gfx950 (v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32, exact f32 = fmaf chain,
// cdna_hip_programming.md section 3) and the launch macro.
//
// Two things in here rest on how gfx950 executes sc1 (write-through) stores rather than on an architectural promise: the fence-free
// hand-off between workgroups (results depend on it: see the compile-time guard at "In-launch hand-off") and the write-through stores
// of kernels' FINAL outputs (lfdm_store_f4_out: speed only - the kernel boundary orders them as it orders plain stores).
//
// LFDM_EMU_BUILD is a TEST-ONLY switch: tests/emu/ compiles these same kernel sources for x86
// against a fiber emulator so that index arithmetic can be checked against the CPU oracle in a
// container without a GPU.  The product library is built by hipcc for gfx950 only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

#if defined(LFDM_EMU_BUILD)
#include "hip_emu.h"
typedef emu_f32x16 f32x16;
typedef emu_f32x4 f32x4;
#define LFDM_LAUNCH(kern, grid, block, smem, stream, ...) \
  emu::launch(grid, block, smem, [=]() { kern(__VA_ARGS__); })
static inline f32x16 mfma_32x32x2(float a, float b, f32x16 c) { return emu_mfma_32x32x2(a, b, c); }
static inline f32x4 mfma_16x16x4(float a, float b, f32x4 c) { return emu_mfma_16x16x4(a, b, c); }
static inline f32x4 mfma_4x4x1(float a, float b, f32x4 c) { return emu_mfma_4x4x1(a, b, c); }
// bf16 operands (the opt-in Winograd K loop, conv_wino.hip): raw bits, k order.  RNE float -> bf16 as v_cvt_pk_bf16_f32 rounds
// (NaN stays a quiet NaN); the MFMA model multiplies exactly (bf16 x bf16 fits an fp32 significand) and accumulates in fp32 in k order.
struct lfdm_bf16x8 { uint16_t h[8]; };
static inline uint16_t lfdm_f32_to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float lfdm_bf16_to_f32(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static inline lfdm_bf16x8 lfdm_cvt_bf16x8(float4 a0, float4 a1) {
  const float f[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  lfdm_bf16x8 r;
  for (int i = 0; i < 8; ++i) r.h[i] = lfdm_f32_to_bf16(f[i]);
  return r;
}
static inline uint32_t lfdm_cvt_pk_bf16(float lo, float hi) { return (uint32_t)lfdm_f32_to_bf16(lo) | ((uint32_t)lfdm_f32_to_bf16(hi) << 16); }
static inline lfdm_bf16x8 lfdm_bf16x8_bits(float4 v) {
  lfdm_bf16x8 r;
  memcpy(&r, &v, 16);
  return r;
}
// v_mfma_f32_32x32x16_bf16: A[i][k] = element k & 7 of lane i + 32 (k >> 3), B[k][j] = element k & 7 of lane j + 32 (k >> 3);
// D as v_mfma_f32_32x32x2_f32.  Lane l first takes its partner l ^ 32's operands (then it holds A row / B column l & 31 whole),
// then reads every A row it needs from the lane that holds it.
static inline f32x16 mfma_32x32x16_bf16(lfdm_bf16x8 a, lfdm_bf16x8 b, f32x16 c) {
  struct Pair { lfdm_bf16x8 a, b; };
  struct Whole { lfdm_bf16x8 a[2], b[2]; };
  const unsigned lane = emu::lane_id(), h = lane >> 5;
  const Pair other = emu::wave_read_from(Pair{a, b}, lane ^ 32u);
  Whole mine;
  mine.a[h] = a;
  mine.a[1 - h] = other.a;
  mine.b[h] = b;
  mine.b[1 - h] = other.b;
  for (int r = 0; r < 16; ++r) {
    const unsigned row = (r & 3) + 8 * (r >> 2) + 4 * h;
    const Whole src = emu::wave_read_from(mine, row);
    float acc = c[r];
    for (int k = 0; k < 16; ++k)
      acc = fmaf(lfdm_bf16_to_f32(src.a[k >> 3].h[k & 7]), lfdm_bf16_to_f32(mine.b[k >> 3].h[k & 7]), acc);
    c[r] = acc;
  }
  return c;
}
#else
#include <hip/hip_runtime.h>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
#define LFDM_LAUNCH(kern, grid, block, smem, stream, ...) \
  hipLaunchKernelGGL(kern, grid, block, smem, stream, __VA_ARGS__)
// lane l: A[i = l&31][k = l>>5], B[k = l>>5][j = l&31]; D col = l&31, row = (r&3)+8*(r>>2)+4*(l>>5)
__device__ __forceinline__ f32x16 mfma_32x32x2(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// lane l: A[i = l&15][k = l>>4], B[k = l>>4][j = l&15]; D col = l&15, row = (l>>4)*4 + r
__device__ __forceinline__ f32x4 mfma_16x16x4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// 16 independent 4x4 blocks (K = 1): block b = l>>2, A_b[i] from lane 4b+i, B_b[j] from lane 4b+j; D_b[i][j] = register i
// of lane 4b+j.  Full MFMA rate with only FOUR output columns per block: the shape for skinny-N contractions.
__device__ __forceinline__ f32x4 mfma_4x4x1(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
}
// bf16 operands (the opt-in Winograd K loop, conv_wino.hip): lane l holds A[i = l&31][k = 8*(l>>5) .. +7] and B[k = 8*(l>>5) .. +7][j = l&31];
// D as v_mfma_f32_32x32x2_f32, accumulated in fp32.  The conversions are v_cvt_pk_bf16_f32 (round to nearest even on gfx950).
typedef __bf16 lfdm_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 lfdm_bf16x2 __attribute__((ext_vector_type(2)));
typedef float lfdm_f32x8 __attribute__((ext_vector_type(8)));
typedef float lfdm_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ lfdm_bf16x8 lfdm_cvt_bf16x8(float4 a0, float4 a1) {
  const lfdm_f32x8 f = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  return __builtin_convertvector(f, lfdm_bf16x8);
}
__device__ __forceinline__ uint32_t lfdm_cvt_pk_bf16(float lo, float hi) {
  const lfdm_f32x2 f = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, lfdm_bf16x2));
}
__device__ __forceinline__ lfdm_bf16x8 lfdm_bf16x8_bits(float4 v) { return __builtin_bit_cast(lfdm_bf16x8, v); }
__device__ __forceinline__ f32x16 mfma_32x32x16_bf16(lfdm_bf16x8 a, lfdm_bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
#endif

#define LFDM_WAVE 64

// compile-time loop: f(std::integral_constant<int, I>) for I = BEGIN .. END-1 (indices usable as template / asm immediates)
template <int BEGIN, int END, class F>
__device__ __forceinline__ void lfdm_static_for(F&& f) {
  if constexpr (BEGIN < END) {
    f(std::integral_constant<int, BEGIN>{});
    lfdm_static_for<BEGIN + 1, END>(f);
  }
}

// Host-side ladder: f(std::integral_constant<int, R>) for the first rung R >= v; the last rung takes everything above it.  A launch
// site names its kernel and argument list once, inside f.
template <int R, int... REST, class F>
inline auto lfdm_ladder(int v, F&& f) {
  if constexpr (sizeof...(REST) == 0) return f(std::integral_constant<int, R>{});
  else return v <= R ? f(std::integral_constant<int, R>{}) : lfdm_ladder<REST...>(v, f);
}

// Buffer-descriptor loads: an out-of-range byte offset returns zeros, which turns "is this filter tap
// inside the image" into one v_cndmask on the offset instead of a divergent branch around the load
// (branches inside the MFMA loop also made hipcc copy all accumulator registers every iteration).
#if defined(LFDM_EMU_BUILD)
struct lfdm_buf {
  const char* base;
  uint32_t bytes;
};
static inline lfdm_buf lfdm_make_buf(const void* p, uint32_t bytes) { return lfdm_buf{(const char*)p, bytes}; }
static inline float4 lfdm_buf_load_f4(lfdm_buf b, uint32_t off) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if ((uint64_t)off + 16u <= (uint64_t)b.bytes) memcpy(&v, b.base + off, 16);
  return v;
}
static inline float2 lfdm_buf_load_f2(lfdm_buf b, uint32_t off) {
  float2 v = make_float2(0.f, 0.f);
  if ((uint64_t)off + 8u <= (uint64_t)b.bytes) memcpy(&v, b.base + off, 8);
  return v;
}
#else
typedef __amdgpu_buffer_rsrc_t lfdm_buf;
typedef int lfdm_i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ lfdm_buf lfdm_make_buf(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 lfdm_buf_load_f4(lfdm_buf b, uint32_t off) {
  const lfdm_i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(b, (int)off, 0, 0);
  float4 f;
  f.x = __int_as_float(v.x);
  f.y = __int_as_float(v.y);
  f.z = __int_as_float(v.z);
  f.w = __int_as_float(v.w);
  return f;
}
typedef int lfdm_i32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 lfdm_buf_load_f2(lfdm_buf b, uint32_t off) {
  const lfdm_i32x2 v = __builtin_amdgcn_raw_buffer_load_b64(b, (int)off, 0, 0);
  return make_float2(__int_as_float(v.x), __int_as_float(v.y));
}
#endif
#define LFDM_BUF_OOB 0xFFFFFFF0u

// 16-byte WRITE-THROUGH store / L1-bypassing load through a buffer descriptor (sc1: cdna_hip_programming.md Guideline 16 form R1 - the payload of
// an in-launch hand-off between workgroups).  One 16-byte sc1 store is ONE fabric write; the same float4 as two 8-byte agent-scope atomic
// stores costs 2.7x the time per byte (MI355X_MICROARCH.md, "stores of each flavour") and an 8-byte sc1 load runs at 0.54-0.70x the
// 16-byte rate.  Ordering against the flag / ticket is the caller's: every storing wave drains (s_waitcnt vmcnt(0)) before the ticket.
#if defined(LFDM_EMU_BUILD)
static inline void lfdm_buf_store_f4_sc1(lfdm_buf b, uint32_t off, float4 v) {
  if ((uint64_t)off + 16u <= (uint64_t)b.bytes) memcpy(const_cast<char*>(b.base) + off, &v, 16);
}
static inline float4 lfdm_buf_load_f4_sc1(lfdm_buf b, uint32_t off) { return lfdm_buf_load_f4(b, off); }
#else
__device__ __forceinline__ void lfdm_buf_store_f4_sc1(lfdm_buf b, uint32_t off, float4 v) {
  lfdm_i32x4 d;
  d.x = __float_as_int(v.x); d.y = __float_as_int(v.y); d.z = __float_as_int(v.z); d.w = __float_as_int(v.w);
  __builtin_amdgcn_raw_buffer_store_b128(d, b, (int)off, 0, 16);          // aux 16 = sc1 on gfx940+
}
__device__ __forceinline__ float4 lfdm_buf_load_f4_sc1(lfdm_buf b, uint32_t off) {
  const lfdm_i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(b, (int)off, 0, 16);
  float4 f;
  f.x = __int_as_float(v.x); f.y = __int_as_float(v.y); f.z = __int_as_float(v.z); f.w = __int_as_float(v.w);
  return f;
}
#endif

// FINAL outputs written through.  A kernel's plain stores stay dirty in the producing XCD's L2 until the launch ends, and the release at
// the kernel boundary writes them back while the dependent successor waits (MI355X_MICROARCH.md, row "boundary": + B / 6 TB/s behind B dirty
// bytes).  lfdm_store_f4_out<true> stores the same 16 bytes to the same address with the sc1 policy of the slab stores above: the bytes
// leave for memory while the kernel still runs and the launch-end release finds nothing dirty.  No fence, no drain, no change to what a
// kernel boundary orders - the consumer is a LATER launch, and the boundary makes the bytes visible to it as it did for plain stores.
//   * 16-byte stores only (a narrower write-through store is one fabric write each: 2.7x the time per byte at 8 bytes, ~6x at 4);
//     epilogues that store narrower, or that cannot prove 16-byte alignment, keep their plain store.  Never `nt`.
//   * the storing thread never reads the address back in the same launch (the pointer form is an asm statement without a memory
//     clobber, so that the loads of a streaming loop may still be hoisted above it; `s_nop 1` ends it: hipcc pads nothing behind an asm
//     store and could otherwise overwrite the data registers before the store has read them - cdna_hip_programming.md 5.7).
// WHAT THIS RESTS ON: like the hand-off protocol below, on how gfx950 executes sc1 stores (written through to memory as they retire), not
// on an architectural promise; on a target where sc1 means something else the results are still right - the boundary's release is
// untouched - and only the speed argument falls.  Which kernel families use it is decided per family by measurement
// (profiles/store_through_ab.txt) and fixed at compile time: -DLFDM_ST_<FAMILY>=0 / 1 rebuilds one family with the other policy.
#ifndef LFDM_ST_GN
#define LFDM_ST_GN 1               // gn_apply_kernel (norm.hip)
#endif
#ifndef LFDM_ST_WINO
#define LFDM_ST_WINO 1             // conv_wino.hip: whole jobs, the pooled epilogue and the in-launch reducer's final store
#endif
#ifndef LFDM_ST_IGEMM
#define LFDM_ST_IGEMM 1            // conv_igemm.hip: the float4 epilogue and conv_splitk_reduce_vec_kernel
#endif
#ifndef LFDM_ST_KSW
#define LFDM_ST_KSW 0              // conv_ksw.hip: the float4 epilogue
#endif
#ifndef LFDM_ST_PW
#define LFDM_ST_PW 1               // conv_pw_kernel, all forms
#endif
#ifndef LFDM_ST_LINATTN_FUSED
#define LFDM_ST_LINATTN_FUSED 0    // linattn_fused_out2_kernel
#endif
#ifndef LFDM_ST_LINATTN_OUT
#define LFDM_ST_LINATTN_OUT 0      // linattn_output_kernel (the unfused chain of the 16x16 level)
#endif
#if defined(LFDM_EMU_BUILD)
template <bool THROUGH> static inline void lfdm_store_f4_out(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
#else
template <bool THROUGH>
__device__ __forceinline__ void lfdm_store_f4_out(float* p, float4 v) {
  if constexpr (THROUGH) {
    const f32x4 d = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(d));
  } else {
    *reinterpret_cast<float4*>(p) = v;
  }
}
#endif

// Register-operand load pipelines.  hipcc (ROCm 7.2) undoes a source-level "load group g+1, multiply group g" loop whenever the loaded
// values feed MFMAs straight from registers: the load is sunk across the back-edge to its use and every group pays the full memory
// latency (attn_lowres.hip, first version: 18.6 us for 3 us of MFMA).  The loads of such loops are therefore issued by inline asm
// (volatile: never moved or sunk) and retired by hand-counted s_waitcnt vmcnt(N) - loads return in order, N = the number of loads
// issued AFTER the ones being waited for; the waited registers are "+v" operands of the wait, so no consumer can be scheduled above
// it (cdna_hip_programming.md 5.4 rule 18, 5.7).  Only in fully unrolled straight-line code (no loop-carried asm outputs).
#if defined(LFDM_EMU_BUILD)
template <int OFF = 0> static inline void lfdm_gload_f4(f32x4& dst, const float* p) { memcpy(&dst, (const char*)p + OFF, 16); }
template <int N> static inline void lfdm_vmwait() {}
template <int N> static inline void lfdm_vmwait(f32x4&) {}
template <int N> static inline void lfdm_vmwait(f32x4&, f32x4&) {}
template <int N> static inline void lfdm_vmwait(f32x4&, f32x4&, f32x4&, f32x4&) {}
static inline void lfdm_tie(f32x4&) {}
static inline int lfdm_uniform(int v) { return v; }
#else
template <int OFF = 0>      // OFF: byte offset folded into the instruction (0 .. 4095)
__device__ __forceinline__ void lfdm_gload_f4(f32x4& dst, const float* p) {
  asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(dst) : "v"(p), "n"(OFF) : "memory");
}
template <int N> __device__ __forceinline__ void lfdm_vmwait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void lfdm_vmwait(f32x4& a) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void lfdm_vmwait(f32x4& a, f32x4& b) {
  asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void lfdm_vmwait(f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N) : "memory");
}
__device__ __forceinline__ void lfdm_tie(f32x4& a) { asm volatile("" : "+v"(a)::"memory"); }      // orders a consumer behind the preceding wait
// a value the compiler cannot prove wave-uniform (anything derived from threadIdx) made uniform for it: keeps buffer descriptors /
// scalar selects out of per-load "waterfall" loops (cdna_hip_programming.md T20)
__device__ __forceinline__ int lfdm_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
#endif

// In-launch hand-off between workgroups: every workgroup leaves a partial result (the payload) in global memory and takes a ticket; the
// workgroup that draws the last ticket reads all payloads and finishes the job in a fixed order.  The protocol as the kernels run it:
//   payload   8-byte agent-scope words, written and read ONLY through lfdm_agent_store_u64 / lfdm_agent_load_u64 (write-through sc1
//             stores, L1-bypassing sc1 loads), or the 16-byte sc1 buffer accesses above (lfdm_buf_store_f4_sc1 / lfdm_buf_load_f4_sc1,
//             conv_wino.hip).  Never plain stores or loads: those stay in one XCD's L2, and the 8 L2s are not coherent with each other.
//   drain     LFDM_DRAIN_STORES() in every thread that stored payload, after its last payload store and in front of the barrier (or, with
//             one storing thread, in front of that thread's own ticket): the stores are acknowledged at memory before the ticket moves.
//   ticket    lfdm_ticket_last by ONE thread of the workgroup, after the barrier that follows the drains (lfdm_workgroup_last: thread 0
//             and the broadcast of its answer).  A relaxed agent-scope RMW; no release / acquire fence anywhere.
//   reset     the thread that draws the last ticket stores 0 into the word before anybody reads payload: the array is zero again when
//             the launch ends, no memset between launches.
//   stream    a ticket array belongs to ONE stream: launches that share it must be ordered.
// WHAT THIS RESTS ON.  Relaxed agent-scope stores -> `s_waitcnt vmcnt(0)` -> relaxed ticket RMW -> relaxed agent-scope loads carry no
// release / acquire, so the HIP / LLVM memory model promises no happens-before between payload and ticket.  The hand-off is correct on
// gfx950 because of how that target lowers and executes it (MI355X_MICROARCH.md, "inter-workgroup visibility": sc1 stores are written
// through and acknowledged at memory before vmcnt drops; sc1 loads and atomics are served past the per-XCD L2s; observed untorn for 8-byte
// granules) - hardware behaviour validated on gfx950 / ROCm 7.2, not an architectural guarantee.  Hence the compile-time guard below (the
// library is built for gfx950 only, _build.py), the 128-byte boundary lfdm_conv2d_cl_f32 rounds the split-K slab base up to (two column tiles
// on different XCDs never share a cache line), and tests/test_ops_parity.py::test_wino_fused_reduce_stress (bit-equal to the separate
// reduce pass over many launches under load).  Another target re-validates this or puts an agent-scope release fence in front of the
// ticket and an agent-scope acquire fence behind the last one; no such fence is defined here because no kernel issues one.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(LFDM_EMU_BUILD)
#error "fence-free hand-off (lfdm_agent_store_u64 / lfdm_agent_load_u64 / lfdm_ticket_last) validated on gfx950 only: re-validate, or add agent-scope release / acquire fences around the ticket, before building for another target"
#endif
#if defined(LFDM_EMU_BUILD)
#define LFDM_DRAIN_STORES() ((void)0)
static inline unsigned lfdm_ticket_take(unsigned* c) { return __atomic_fetch_add(c, 1u, __ATOMIC_SEQ_CST); }   // workgroups run on several OS threads
static inline void lfdm_ticket_reset(unsigned* c) { __atomic_store_n(c, 0u, __ATOMIC_SEQ_CST); }
static inline void lfdm_agent_store_u64(unsigned long long* p, unsigned long long v) { __atomic_store_n(p, v, __ATOMIC_SEQ_CST); }
static inline unsigned long long lfdm_agent_load_u64(const unsigned long long* p) { return __atomic_load_n(p, __ATOMIC_SEQ_CST); }
#else
#define LFDM_DRAIN_STORES() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
__device__ __forceinline__ unsigned lfdm_ticket_take(unsigned* c) {
  return __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lfdm_ticket_reset(unsigned* c) {
  __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lfdm_agent_store_u64(unsigned long long* p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long lfdm_agent_load_u64(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif
// One thread: takes a ticket of `count`; true for the one that takes the last, which has then reset the word.
__device__ __forceinline__ bool lfdm_ticket_last(unsigned* c, unsigned count) {
  const bool last = lfdm_ticket_take(c) == count - 1;
  if (last) lfdm_ticket_reset(c);
  return last;
}
// All threads of a workgroup, behind the barrier that follows the drains: thread 0 takes the ticket, every thread gets its answer
// through the LDS word `flag`.
__device__ __forceinline__ bool lfdm_workgroup_last(unsigned* c, unsigned count, unsigned* flag) {
  if (threadIdx.x == 0) *flag = lfdm_ticket_last(c, count) ? 1u : 0u;
  __syncthreads();
  return *flag != 0u;
}

// A line the instruction scheduler moves nothing across (no instruction of its own): bounds how far ahead a software pipeline written in
// source order may be pulled - past it, hipcc requests every later stage's operands at once and pays for them in registers.
// LFDM_SCHED_GROUP(mask, n): the next n instructions of class `mask` (LFDM_SG_MFMA, LFDM_SG_VALU: vector ALU other than MFMA and
// transcendentals) of the region between two fences form a group; successive groups are issued in the order they are written.
#if defined(LFDM_EMU_BUILD)
#define LFDM_SCHED_FENCE() ((void)0)
#define LFDM_SCHED_GROUP(mask, n) ((void)0)
#else
#define LFDM_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#define LFDM_SCHED_GROUP(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0)
#endif
#define LFDM_SG_VALU 0x002
#define LFDM_SG_MFMA 0x008

// Ordering point for LDS traffic that stays INSIDE one wavefront (a wave-private LDS region written by some lanes and read by others): the
// LDS unit executes a wave's operations in order, so all that is needed is that the compiler keeps them in program order and that every
// lane has issued its writes - no workgroup barrier, the other waves of the workgroup are not involved.
#if defined(LFDM_EMU_BUILD)
static inline void lfdm_wave_lds_sync() { emu::wave_sync(); }
#else
__device__ __forceinline__ void lfdm_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

// Fixed-order folds (float or double).  Wave butterfly: x + y == y + x and max is exact, so every lane ends with the same bits.
// The fold runs in the argument's type: a double expression is reduced in double (there is no silent conversion to float), an integer
// argument does not compile.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  static_assert(std::is_floating_point<T>::value, "wave_sum: float or double");
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ float lfdm_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double lfdm_max(double a, double b) { return fmax(a, b); }
template <class T>
__device__ __forceinline__ T wave_max(T v) {
  static_assert(std::is_floating_point<T>::value, "wave_max: float or double");
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = lfdm_max(v, __shfl_xor(v, m));
  return v;
}
// The four waves of a 256-thread workgroup through the LDS slots s[4], which nobody is still reading: `v` is the wave's result (every
// lane holds it); every thread returns (w0 + w1) + (w2 + w3), or the maximum in the same pairing.
__device__ __forceinline__ float block4_sum(float v, float* s) {
  if ((threadIdx.x & (LFDM_WAVE - 1)) == 0) s[threadIdx.x / LFDM_WAVE] = v;
  __syncthreads();
  return (s[0] + s[1]) + (s[2] + s[3]);
}
__device__ __forceinline__ float block4_max(float v, float* s) {
  if ((threadIdx.x & (LFDM_WAVE - 1)) == 0) s[threadIdx.x / LFDM_WAVE] = v;
  __syncthreads();
  return fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
}
// Sums the double `v` over a 256-thread workgroup through the LDS slots s[4], which nobody is still reading: butterfly per wave, then the
// four waves' sums in wave order, ((w0 + w1) + w2) + w3.  Every thread returns the sum.
__device__ __forceinline__ double block_sum_f64(double v, double* slots) {
  v = wave_sum(v);
  if ((threadIdx.x & (LFDM_WAVE - 1)) == 0) slots[threadIdx.x / LFDM_WAVE] = v;
  __syncthreads();
  double s = slots[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) s += slots[w];
  return s;
}
// Fixed tree over the 256 doubles the lanes of a 256-thread workgroup stored in s[threadIdx.x]: the same pairs in the same order on
// every run.  The sum is s[0]; ends on a barrier.
__device__ __forceinline__ void block_tree_sum(double* s) {
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
}
// exp of a NON-POSITIVE argument (softmax terms exp(x - max), running-max rescales) on the hardware exponential: v_exp_f32(x * log2 e).
// The rounding of x * log2 e grows with |x|: against expf, 1.5 ulp on [-1, 0], 8.5 ulp on [-10, -1], ~30 ulp on [-30, -10] (checked on the
// CPU) - relative errors of 4e-6 on terms below e^-10 of their row's largest, harmless for a softmax, but NOT "within 2 ulp".  A huge
// negative argument (-3e38 - m, the first running-max rescale) overflows to -inf in the product and gives exactly 0.  fast_rcp is
// v_rcp_f32 (1 ulp): ONE reciprocal per softmax row, multiplied into the probabilities, instead of an IEEE division per element.
// The emulator build keeps expf and the division.
#if defined(LFDM_EMU_BUILD)
static inline float fast_exp(float x) { return expf(x); }
static inline float fast_rcp(float x) { return 1.0f / x; }
#else
__device__ __forceinline__ float fast_exp(float x) { return __expf(x); }
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
#endif
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float siluf_(float x) { return x / (1.0f + expf(-x)); }

// SiLU on the hardware exponential / reciprocal (v_exp_f32, v_rcp_f32: ~1 ulp each): for activations recomputed inside a consumer's
// load path (lfdm_conv_params.gn_in_*), where the IEEE division + expf expansion of siluf_ would cost more than the launch it saves
#if defined(LFDM_EMU_BUILD)
static inline float silu_fast_(float x) { return x / (1.0f + expf(-x)); }
#else
__device__ __forceinline__ float silu_fast_(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
#endif

// Tuning knobs.  Schedule constants that were found by sweeps (tile shapes, workgroup counts, thresholds) can be overridden from the
// environment ONLY in a library built with -DLFDM_TUNING_KNOBS (python -m cvpr23_lfdm_amd._build hip --knobs; tools/sweep_*.sh, tools/bench_*.py and
// the tests that force a tile shape ask the library whether it has them: lfdm_has_tuning_knobs).  The shipped build compiles every one
// of them to its default: no getenv on a launch path, no variant the parity suite does not run.
#if defined(LFDM_TUNING_KNOBS) || defined(LFDM_EMU_BUILD)
static inline const char* lfdm_knob(const char* name) { return getenv(name); }
#else
static inline const char* lfdm_knob(const char*) { return nullptr; }
#endif

// activation codes shared by the C ABI (include/lfdm_hip.h)
__device__ __forceinline__ float apply_act(float v, int act) {
  if (act == 1) return v > 0.f ? v : 0.f;
  if (act == 2) return sigmoidf_(v);
  if (act == 3) return siluf_(v);
  return v;
}

// host-side error plumbing (lfdm_capi.hip)
extern "C" void lfdm_set_error(const char* msg);
int lfdm_check_launch(const char* what);
// the one way to refuse: sets the error text (printf-style) and returns `code`
int lfdm_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// every pointer is a multiple of N bytes (a null pointer passes: optional operands)
template <unsigned N = 16, class... P>
inline bool lfdm_aligned(const P*... p) {
  return ((0 | ... | (uintptr_t)p) & (N - 1)) == 0;
}
template <class... P>
inline bool lfdm_aligned16(const P*... p) {
  return lfdm_aligned<16>(p...);
}

// workgroups of a grid-stride launch: ceil(items / per_block) clamped to [1, cap]
inline unsigned lfdm_blocks(int64_t items, int64_t per_block, int64_t cap) {
  const int64_t nb = (items + per_block - 1) / per_block;
  return (unsigned)(nb < 1 ? 1 : nb > cap ? cap : nb);
}

// Cuts a workspace into its parts, in order: the *_ws_bytes query and the launcher run the same carve function, once over a null base
// for the size and once over the caller's buffer, so the two cannot drift apart.  Every part starts where the previous one ended (the
// parts are sized in whole floats / words: no padding, today's offsets).
struct lfdm_carver {
  char* base;
  size_t bytes = 0;
  explicit lfdm_carver(void* ws) : base((char*)ws) {}
  template <class T>
  T* take(size_t count) {
    T* p = base ? (T*)(base + bytes) : nullptr;
    bytes += count * sizeof(T);
    return p;
  }
};
