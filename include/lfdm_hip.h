/* lfdm_hip.h - C ABI of liblfdm_hip.so, the MI355X (gfx950) kernels of the LFDM hot path.
 *
 * The reference (nihaomiao/CVPR23_LFDM) has no native/FFI layer: its hot path is a chain of
 * PyTorch ATen calls.  Each entry point below replaces one family of
 * those call sites; the reference file:line it stands in for is cited per function
 * (paths relative to the reference root).  The Python host side (cvpr23_lfdm_amd/) binds these
 * with ctypes - see INTEGRATION.md for the stub.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 (unless stated) owned by the caller;
 *  - "CL" = channels-last rows: a tensor (N, H, W, C) stored as N*H*W rows of C floats with a
 *    row stride `ld` >= C (so a kernel can read/write a channel slice of a wider buffer);
 *    UNet activations use N = B*T (frame-major: row = ((b*T + t)*H + y)*W + x);
 *  - "planar" = the reference layout (B, C, T, H, W) / (B, C, H, W), contiguous;
 *  - no allocation, no synchronisation, no hidden state: every call only enqueues kernels on
 *    `stream` (hipGraph-capturable); scratch memory is passed in by the caller;
 *  - return value 0 on success, negative LFDM_E* otherwise; lfdm_last_error() describes it.
 *
 * Layouts (the "Layout:" line of each entry point; tests/test_operand_layouts.py asserts them)
 *  - a row operand with a leading dimension (ld0, ldo, ldx, ss_ld, ...) is a window of a wider buffer: row r starts at base + r*ld,
 *    columns are adjacent, ld >= its column count.  The floats of a row beyond its columns ("gap columns"), and everything else
 *    outside the window, are never read into a result and never written - they may hold NaN.  An operand without a leading
 *    dimension is dense;
 *  - "any" = every 4-byte aligned pointer and every ld is taken (the library picks a scalar form where a vector form does not
 *    apply); "16 B" = the pointer must be 16-byte aligned and "ld % 4" the stride a multiple of 4 floats, LFDM_EINVAL otherwise -
 *    a refused call enqueues nothing and writes nothing;
 *  - operands must not overlap unless the line says "may alias".
 */
#ifndef LFDM_HIP_H
#define LFDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* lfdm_stream_t; /* hipStream_t */

#define LFDM_OK 0
#define LFDM_EINVAL (-1)
#define LFDM_ELAUNCH (-2)
#define LFDM_EWORKSPACE (-3)

#define LFDM_ACT_NONE 0
#define LFDM_ACT_RELU 1
#define LFDM_ACT_SIGMOID 2
#define LFDM_ACT_SILU 3
#define LFDM_ACT_GELU 4

const char* lfdm_last_error(void);
int lfdm_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Convolution as fp32-MFMA implicit GEMM (M = N*hq*wq pixels, N = cout, K = kh*kw*cin).
 * Replaces: Conv3d k=(1,3,3) Block.proj  DM/modules/video_flow_diffusion.py:199
 *           Conv3d 1x1x1 res_conv :224, final heads :495,508; Linear to_qkv/to_out :300-301;
 *           Conv2d 1x1 SpatialLinearAttention :246-247; Downsample :167; Upsample :158,160-163;
 *           init_conv fea term :410; LFAE Conv2d blocks LFAE/modules/util.py:70-150,
 *           LFAE/modules/generator.py:54 (with eval-BatchNorm folded into weight/bias).
 * Input = channel concat of src0 (c0 ch) and optional src1 (c1 ch)  -> torch.cat :580,587.
 * Tap (ky,kx) reads input pixel (qy*stride + ky - pad_y, qx*stride + kx - pad_x) of the
 * (optionally x2 nearest-upsampled) input; out pixel = (qy*out_scale + out_off_y, ...), which
 * expresses ConvTranspose3d k4 s2 p1 as four 2x2 parity convolutions.
 * weight is packed [ceil(K/32)][coutp][32] with K = kh*kw*(c0+c1) flattened tap-major then
 * channel (k = tap*cin + c), zero padded (coutp = cout rounded up to 32).
 * out = act(acc + bias + residual).
 * Optional fused GroupNorm statistics (ksplit == 1): when gn_partial != NULL the kernel also writes, per
 * output row tile, the (sum, sum of squares) of (acc + bias) per channel group:
 * gn_partial[(tile*gn_groups + g)*2 + {0,1}], tile = first_row / tile_rows (lfdm_conv2d_plan); it requires
 * gn_pixels (rows per sample) to be a multiple of the tile rows so no tile straddles two samples.
 */
typedef struct lfdm_conv_params {
  const float* src0;
  const float* src1;
  int c0, c1, ld0, ld1;
  int n_img, hi, wi;      /* physical input size */
  int hq, wq;             /* iteration grid per image */
  int stride;             /* input stride */
  int upsample;           /* 1: read the input through a virtual nearest x2 upsample */
  int pad_mode;           /* 0 zeros, 1 reflect */
  int kh, kw, pad_y, pad_x;
  const float* weight;
  int cout, coutp;
  const float* bias;      /* [cout] or NULL */
  float* out;
  int ldo, ho, wo;
  int out_scale, out_off_y, out_off_x;
  const float* residual;  /* NULL or rows indexed like out */
  int ldr;
  int act;                /* LFDM_ACT_* (NONE/RELU/SIGMOID/SILU) */
  /* split-K: 0 = let the library choose (lfdm_conv2d_plan reports the choice), >= 1 = forced.
     With a factor > 1 raw partial sums go to `partial` ([ksplit][M][coutp], size from
     lfdm_conv2d_partial_bytes) and a reduce pass applies bias/residual/act. */
  int ksplit;
  float* partial;
  float* gn_partial;      /* NULL or fused GroupNorm partial sums (see above) */
  int gn_groups, gn_pixels;
  /* Optional fused channel-LayerNorm of the INPUT rows (1x1 convolutions only; PreNorm + to_qkv,
     video_flow_diffusion.py:176-179,189 + :311 / :253): with W' = W*gamma packed as `weight` and
     ln_wsum[o] = sum_c W'[o][c], the kernel accumulates each row's mean / variance while it streams
     the row and writes rstd*(x.W' - mean*ln_wsum) - algebraically LayerNorm(x)*gamma followed by W. */
  const float* ln_wsum;
  float ln_eps;
  /* Optional in-launch split-K reduction (Winograd F(2x2) schedule with 32-column workgroups): tile_counters_len
     zero-initialised words, at least one per output tile (lfdm_conv2d_plan's tile_rows - 128 - x 32 columns).  When given, the
     workgroup that finishes a tile's last K slice sums the slabs in `partial` (slice order: bit-identical to the reduce pass) and runs the
     epilogue itself - no reduce launch; the counters are left at zero again.  NULL / too short / an unsupported geometry = separate reduce
     pass (lfdm_conv2d_plan's tile_rows says which: 16 = reduce pass).  The slabs cross workgroups as 16-byte write-through (sc1) stores / L1-bypassing
     loads through a buffer descriptor (the library rounds `partial` up to a 128-byte boundary; lfdm_conv2d_partial_bytes carries the slack):
     no scope fence.  With tile_counters the Winograd plan also splits 8..15-chunk reductions.
     BALANCED launch (round 6): with tile_counters AND a `partial` buffer of lfdm_conv2d_partial_bytes, a Winograd launch of exactly 640
     (tile, K slice) workgroups - three on half of the 256 CUs, two on the others - runs as 512 whole jobs + both halves of the other 128
     (768 workgroups: two whole + one half per CU); a halved slice adds one slab to its tile, so lfdm_conv2d_partial_bytes may be non-zero for a
     plan with ksplit = 1 and lfdm_conv2d_plan_slabs reports ksplit + the extra slabs.  The slabs are still summed in one fixed order (run-to-run
     identical results), but not the order of the plain launch: equal to it within fp32 rounding, not bit for bit.  LFDM_WINO_BALANCE=0 disables.
     GroupNorm partial sums of a fused Winograd launch whose groups are wider than 32 channels occupy cg/32 chunk slots per tile block:
     chunk = tile block * (cg / 32) + column part. */
  unsigned int* tile_counters;
  int tile_counters_len;
  /* Optional Winograd F(2x2,3x3) form of the SAME filter (3x3, stride 1, zero pad 1, even H and W, C0 % 16 == C1 % 16 == 0;
     also through the virtual nearest x2 upsample):
     U = G g G^T laid out [16 positions][Cin/16][2 halves j][coutp][2 k-slots kh][4] with reduction channel % 16 = 8 kh + 4 j + e - the
     order of the kernel's two fragment loads, each a contiguous 1 KB per 32 columns (ABI version 8; lfdm_pack_wino_weight_f32 /
     cvpr23_lfdm_amd.ops.pack_wino_weight write it; as a tensor it keeps the shape [16][Cin/16][coutp][16]).  When given and the
     geometry qualifies the library may run the 16/36-multiplication schedule (conv_wino.hip); results differ from the
     direct form by fp32 rounding only (~1e-6 relative).  LFDM_WINO=0 in the environment forces the direct form. */
  const float* weight_wino;
  /* Optional: ConvTranspose k4 s2 p1 (Upsample, video_flow_diffusion.py:158) as ONE launch of its four 2x2 parity
     convolutions.  weight = the four parity packs back to back ([4][ceil(4*cin/32)][coutp][32], parity q = 2*py + px,
     cvpr23_lfdm_amd.ops.pack_deconv_weight), kh = kw = 2, stride 1, out_scale 2, (hq, wq) = (hi, wi), (ho, wo) = 2x.
     Problem q runs with pad = (1 - py, 1 - px) and out_off = (py, px) (the pad_* / out_off_* fields are ignored);
     grid z = 4 * ksplit and the split-K slabs are [4][ksplit][M][coutp] (lfdm_conv2d_partial_bytes accounts for it). */
  int deconv4;
  /* Optional grouped convolution (Winograd schedule only, NULL src1): `groups` > 1 splits the c0 input channels and the
     cout output channels into equal groups (cout / groups a multiple of 32); weight_wino holds the groups' packs back to
     back ([groups][16][c0/groups/16][coutp/groups][16]).  Used to run the two output heads' second convolutions
     (final_conv.0.block2 / occlusion_map.0.block2, video_flow_diffusion.py:493-509) as one launch. */
  int groups;
  /* Optional (Winograd schedule only; lfdm_conv2d_cl_f32 refuses it on a geometry that would run another schedule - ask
     lfdm_conv2d_schedule first): pool2 = 1: the 2x2 average pool that follows conv -> (folded BN) -> act in DownBlock2d
     (LFAE/modules/util.py:136-150) is taken in the epilogue: out has (ho, wo) = (hq / 2, wq / 2) rows per image, one Winograd
     output tile each; needs an output activation, no residual, no fused GroupNorm statistics, no split-K. */
  int pool2;
  /* Optional Winograd F(4x4,3x3) form of the SAME filter (lfdm_pack_wino4_weight_f32: U = G g G^T as [36 positions][C0/8][coutp][8]) -
     an opt-in for BATCHED shapes: 1/4 of the direct form's multiplications (F(2x2): 4/9), fp32 error ~4e-6 of the output scale
     (F(2x2): ~1e-6).  Taken (schedule 4, conv_wino4.hip) only when weight_wino is given too and would run, one source, C0 % 8 == 0,
     H % 4 == W % 4 == 0, no groups / pool2 / fused GroupNorm statistics / forced split-K, and the launch has >= 2048 of its
     512-pixel x 32-column workgroups (LFDM_WINO4_MIN; LFDM_WINO4=0 disables): the frozen-LFAE decode of a training step, throughput
     mode - never the B = 1 sampler.  Bias / residual / activation / virtual x2 upsample as in the F(2x2) schedule. */
  const float* weight_wino4;
  /* RESERVED, must be 0 (ABI 6-11: defer_reduce - raw split-K slabs left for a GroupNorm launch that summed them; measured slower than
     conv + reduce + apply and removed in ABI 12 together with lfdm_groupnorm_splitk_*). */
  int defer_reduce;
  /* Optional (ABI version 8): the SAME 1x1 filter as `weight`, for the pointwise schedule (3) only, in MFMA-operand order
     [ceil(K/32)][coutp/32][4 u][64 lanes = 32*kh + column][4 e] <- W[k = 32g + 8u + 4kh + e][32*ct + column]
     (cvpr23_lfdm_amd.ops.pack_pw_weight): every fragment load of conv_pw_kernel then reads one contiguous 1 KB.  Ignored by the other
     schedules (they read `weight`); NULL = the pointwise kernel reads `weight` as before. */
  const float* weight_pw;
  /* RESERVED, must be NULL / 0 (ABI 8-11: gn_in_* - the INPUT's GroupNorm + SiLU applied inside the Winograd convolution's patch load;
     ~10 us slower per convolution than the launch it saved, removed in ABI 12.  The fields keep the struct layout.) */
  const float* gn_in_partial;
  int gn_in_nchunk, gn_in_groups, gn_in_pixels;
  const float* gn_in_gamma;
  const float* gn_in_beta;
  const float* gn_in_ss;
  int gn_in_ss_ld;
  float gn_in_eps;
  /* Optional (ABI version 12; pointwise schedule 3 only - ask lfdm_conv2d_schedule with the fields set: a geometry that schedule cannot take is
     refused): `residual` is the RAW output of a convolution whose GroupNorm + SiLU has not been applied: res_gn_partial != NULL -> the epilogue adds
     silu(r * A[c] + B[c]) instead of r, with A, B folded from that tensor's (sum, sum of squares) partials exactly like lfdm_groupnorm_apply_cl_f32
     does (res_gn_partial [batch * res_gn_nchunk][2 * res_gn_groups], merged in double in a fixed order; res_gn_gamma / res_gn_beta [cout]; no scale /
     shift).  This is ResnetBlock.forward's `h + res_conv(x)` (video_flow_diffusion.py:226-238) with block2's norm + act folded into the res_conv launch:
     the GroupNorm launch of every ResnetBlock that changes its channel count disappears.  Needs res_gn_pixels (pixels per sample) % 32 == 0 and
     cout % res_gn_groups == 0; out may alias residual (every thread reads the elements it writes). */
  const float* res_gn_partial;
  int res_gn_nchunk, res_gn_groups, res_gn_pixels;
  const float* res_gn_gamma;
  const float* res_gn_beta;
  float res_gn_eps;
} lfdm_conv_params;

/* Layout: src0 / src1 (ld0, ld1), out (ldo), residual (ldr), bias: any.  All 16 B with ld % 4 and cout % 4 == 0: every schedule; otherwise schedule 0
 * only (scalar epilogue / reduce pass for out, residual, bias; generic loads for src0 / src1) - ask lfdm_conv2d_schedule.  Forms that exist in the
 * float4 epilogues only are refused there: gn_partial (needs out 16 B, ldo % 4), ln_wsum (out, residual, bias 16 B, ld % 4), res_gn_*, groups, pool2,
 * lfdm_conv2d_cl_wino_bf16.  out may alias residual (same pointer and ldr == ldo) on every schedule, reduce pass and in-launch reduction:
 * each element is read by the thread that writes it.  out must not overlap src0 / src1.  partial, tile_counters, gn_partial: dense. */
int lfdm_conv2d_cl_f32(const lfdm_conv_params* p, lfdm_stream_t stream);
/* Opt-in lower-precision form of the Winograd F(2x2,3x3) schedule: runs exactly the launch lfdm_conv2d_cl_f32 would run for `p` (same plan:
 * tile_rows, ksplit, slabs, GroupNorm partial layout, tile counters - every buffer sized for p stays valid) with the transform-domain GEMM on
 * bf16 operands: V = B^T d B (fp32) and U rounded once, to nearest even, to bf16; products summed in fp32; input and output transforms,
 * bias, residual, activation, statistics and split-K sums stay fp32.  weight_wino_bf16: lfdm_pack_wino_weight_bf16 of the filter whose fp32
 * pack is p->weight_wino (or, grouped, the groups' bf16 packs back to back); 16-byte aligned.  Refused (LFDM_EINVAL) wherever
 * lfdm_conv2d_schedule(p) != 2, and for pool2. */
int lfdm_conv2d_cl_wino_bf16(const lfdm_conv_params* p, const void* weight_wino_bf16, lfdm_stream_t stream);
/* the schedule the library will use for this geometry: rows of the output tile (32 / 64 / 128 / 160) and the
 * split-K factor (the given one if p->ksplit >= 1).  Fill in gn_partial (any non-NULL value) BEFORE asking when fused
 * GroupNorm statistics are wanted: the pointwise schedule (3) has none, so the request changes the plan. */
int lfdm_conv2d_plan(const lfdm_conv_params* p, int* tile_rows, int* ksplit);
/* which schedule lfdm_conv2d_cl_f32 will run for these parameters: 0 = 2x2-wave implicit GEMM (conv_igemm), 1 = K-split
 * across waves (conv_ksw), 2 = Winograd F(2x2,3x3) (conv_wino: reads weight_wino only - `weight` is then never dereferenced, so
 * a caller that re-packs filters every step, i.e. training, can skip the direct-form pack), 3 = pointwise register-operand
 * GEMM (conv_pw: 1x1 / stride 1 projections with C % 32 == 0 - to_qkv incl. the LayerNorm fold, to_out, res_conv,
 * video_flow_diffusion.py:224,246-247,300-301 - 32-row tiles, never split-K; LFDM_PW=0 in the environment disables it), 4 = Winograd
 * F(4x4,3x3) (conv_wino4: reads weight_wino4 only; batched shapes, see lfdm_conv_params.weight_wino4), < 0 = error */
int lfdm_conv2d_schedule(const lfdm_conv_params* p);
/* bytes of `partial` needed (0 when the plan neither splits K nor balances the launch - see tile_counters) */
size_t lfdm_conv2d_partial_bytes(const lfdm_conv_params* p);
/* slabs per output tile the launch will sum when it is handed `partial`: ksplit, or more for a balanced Winograd launch (tile_counters);
 * 1 = no slabs.  (A binding that compares two plans bit for bit asks this to know whether they sum in the same order.) */
int lfdm_conv2d_plan_slabs(const lfdm_conv_params* p);

/* ------------------------------------------------------------------------------------------
 * GroupNorm(G) over (C/G, T, H, W) + optional (scale+1, shift) + SiLU, channels-last.
 * Replaces Block.forward norm/scale-shift/act: DM/modules/video_flow_diffusion.py:200-211.
 * x, out: (B, P, C) rows (P = T*H*W pixels per sample), may alias.
 * scale_shift: NULL or B rows [scale(C) | shift(C)] with row stride ss_ld (ResnetBlock.mlp output
 * chunked, :230-232).  residual: NULL or rows like x, added AFTER the activation
 * (ResnetBlock: block2(h) + x when res_conv is Identity, :237).
 * ws: caller scratch of lfdm_groupnorm_ws_bytes(B, P, C) bytes.
 */
size_t lfdm_groupnorm_ws_bytes(int batch, int pixels, int channels);
/* Layout (both entry points): x, out, residual dense rows of C floats, 16 B; out may alias x (in place), residual may alias neither.
 * scale_shift (ss_ld >= 2C): any - a column window of a wider table. */
int lfdm_groupnorm_silu_cl_f32(const float* x, float* out, int batch, int pixels, int channels,
                               int groups, const float* gamma, const float* beta,
                               const float* scale_shift, int ss_ld, const float* residual,
                               float eps, int apply_silu, void* ws, size_t ws_bytes,
                               lfdm_stream_t stream);

/* Same normalisation when the statistics were already produced by the preceding convolution
 * (lfdm_conv_params.gn_partial): partial = [batch][nchunk][groups][2] (sum, sum of squares),
 * nchunk = pixels / tile_rows (lfdm_conv2d_plan).  ws: batch*2*channels floats. */
int lfdm_groupnorm_apply_cl_f32(const float* x, float* out, int batch, int pixels, int channels,
                                int groups, const float* gamma, const float* beta,
                                const float* scale_shift, int ss_ld, const float* residual,
                                float eps, int apply_silu, const float* partial, int nchunk,
                                void* ws, size_t ws_bytes, lfdm_stream_t stream);

/* Channel LayerNorm (gamma only, biased variance): video_flow_diffusion.py:170-179. */
/* Layout: x, out dense rows, gamma: 16 B. */
int lfdm_layernorm_cl_f32(const float* x, float* out, int64_t rows, int channels,
                          const float* gamma, float eps, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Softmax attention over short sequences (L <= 64), 8 heads x 32, fp32 MFMA for QK^T / PV.
 * Replaces Attention.forward (video_flow_diffusion.py:303-363) incl. rotary (:329-331),
 * relative position bias (:339-340) and the einops re-layouts (:270-283).
 * qkv: rows of 768 floats [q(8x32) | k | v] in UNet CL row order (B*T*HW rows).
 * mode 0 (temporal): one sequence per (b, pixel), tokens = frames  (needs rot_cos/rot_sin
 *        (T,16) tables and bias (8,T,T)); mode 1 (spatial): one sequence per (b, frame),
 *        tokens = pixels (no rotary, no bias).
 * out: rows of 256 floats (heads merged), same row order.
 */
int lfdm_attention_cl_f32(const float* qkv, float* out, int batch, int frames, int hw, int mode,
                          const float* bias, const float* rot_cos, const float* rot_sin,
                          lfdm_stream_t stream);

/* Linear attention of SpatialLinearAttention.forward (video_flow_diffusion.py:249-265),
 * between the two 1x1 convolutions.  qkv rows of 768, out rows of 256; n_frames = B*T, hw tokens
 * per frame.  ws: n_frames*8*32*32 floats. */
size_t lfdm_linear_attention_ws_bytes(int n_frames);
int lfdm_linear_attention_cl_f32(const float* qkv, float* out, int n_frames, int hw,
                                 void* ws, size_t ws_bytes, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Small dense layers of the conditioning path (time_mlp :423-428, ResnetBlock.mlp :217-220).
 * y[b][n] = act_out( sum_k act_in(x[b][k]) * w[n][k] + bias[n] ),  w rows of stride ldw. */
/* Layout: x (ldx), w (ldw), y (ldy), bias: any.  batch <= 65535 (grid y); more rows are refused with LFDM_EINVAL, nothing launched. */
int lfdm_linear_small_f32(const float* x, const float* w, const float* bias, float* y,
                          int batch, int k, int n, int ldx, int ldw, int ldy, int act_in,
                          int act_out, lfdm_stream_t stream);

/* Per-step conditioning for graph replay: out[b][i] = step_table[*step_dev][i] + batch_base[b][i].
 * (The ResnetBlock.mlp input is cat(time_emb, cond), :562,:230: its Linear splits exactly into a
 * time part that depends only on the step and a cond part that depends only on the sample.) */
int lfdm_step_cond_f32(const float* step_table, const float* batch_base, const int32_t* step_dev,
                       float* out, int batch, int n, lfdm_stream_t stream);

/* SinusoidalPosEmb (:141-153): emb[b] = [sin(t*f_i) | cos(t*f_i)]; freqs[i] = exp(-ln(1e4)*i/(dim/2-1))
 * is a (dim/2) table prepared once by the host (a 1-ulp difference in exp is amplified ~1000x by
 * t, so the table is computed with the same fp32 expression the reference uses).
 * The timestep is read from DEVICE memory (int32) so a captured graph can be replayed per step. */
/* Layout: out (ldo): any. */
int lfdm_sinusoidal_f32(const int32_t* t_dev, int t_stride, const float* freqs, float* out,
                        int batch, int dim, int ldo, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Small-C_in convolution from a PLANAR input into CL output (direct, VALU):
 *   UNet init_conv's step-dependent 3-channel part (video_flow_diffusion.py:410,547) with the
 *   per-video precomputed `fea` term added (exact split of the 259-channel conv by linearity);
 *   LFAE `first` 7x7 conv (LFAE/modules/generator.py:34, BN folded).
 * x: (B, cin_total, T, H, W) planar, only channels [0, cin) are read; w: [kh*kw*cin][cout]
 * (tap-major, then channel); add_term: NULL or (B, H, W, cout) CL broadcast over T.
 */
/* Layout: x dense planar; out (ldo), bias, add_term (dense rows of cout): any (float4 epilogue when all are 16 B with ldo % 4, scalar otherwise). */
int lfdm_conv_planar_in_cl_f32(const float* x, int batch, int cin, int cin_total, int frames,
                               int h, int w, const float* wgt, int kh, int kw, int cout,
                               const float* bias, const float* add_term, float* out, int ldo,
                               int act, lfdm_stream_t stream);

/* Output heads: the two 1x1x1 convs (video_flow_diffusion.py:495,508,588) from CL features to the
 * PLANAR 3-channel prediction (B, 3, T, H, W): ch 0,1 from y_flow (w_flow (2,C)), ch 2 from y_occ.
 * ld = row stride (floats) of both feature tensors: the two heads' ResnetBlocks run as one 2C-channel block, their outputs
 * are the two column halves of one (rows, 2C) buffer. */
/* Layout (the three heads forms): y_flow / y_occ resp. y (ld), x0 (ld0), x1 (ld1): 16 B, ld % 4, C % 4; out dense planar. */
int lfdm_heads_cl_to_planar_f32(const float* y_flow, const float* y_occ, int channels, int ld,
                                const float* w_flow, const float* b_flow, const float* w_occ,
                                const float* b_occ, float* out, int batch, int frames, int hw,
                                lfdm_stream_t stream);
/* The same heads with the ResnetBlocks' res_conv folded in (ABI version 8): the blocks end in h + res_conv(cat(x0, x1))
 * (video_flow_diffusion.py:224,236) and the heads are linear, so W1 (h + Wres [x0|x1] + bres) + b1 = W1 h + (W1 Wres)[x0|x1] + (W1 bres + b1):
 * y_flow / y_occ are the blocks' outputs WITHOUT the res_conv term, w_extra (3, c0 + c1) the composed matrices (rows: flow x, flow y,
 * occlusion), b_flow / b_occ already include W1 bres.  Replaces a 1x1 convolution launch by three more dot products per pixel. */
int lfdm_heads_res_cl_to_planar_f32(const float* y_flow, const float* y_occ, int channels, int ld, const float* w_flow,
                                    const float* b_flow, const float* w_occ, const float* b_occ, const float* x0, int ld0, int c0,
                                    const float* x1, int ld1, int c1, const float* w_extra, float* out, int batch, int frames,
                                    int hw, lfdm_stream_t stream);
/* ... with the block's LAST GroupNorm folded in (ABI version 12): y (rows, >= 2*channels) is the RAW output of the merged heads block's second
 * convolution, columns [flow C | occlusion C]; every value is read as silu(y * A[c] + B[c]) with A, B folded from that tensor's (sum, sum of squares)
 * partials exactly like lfdm_groupnorm_apply_cl_f32 does (partial [batch * nchunk][2 * groups], merged in double in a fixed order; gamma / beta
 * [2*channels]; no scale / shift) - the GroupNorm launch between the convolution and the heads, and the 21 MB it wrote and the heads read back at
 * 40 frames of 32x32, disappear.  Otherwise as lfdm_heads_res_cl_to_planar_f32 (w_flow (2, C), w_occ (1, C), b_* incl. the folded res_conv bias,
 * w_extra (3, c0 + c1)).  video_flow_diffusion.py:199-212 (Block.forward's norm + act), :493-509, :583-586. */
int lfdm_heads_gn_res_cl_to_planar_f32(const float* y, int ld, int channels, const float* partial, int nchunk, int groups,
                                       const float* gamma, const float* beta, float eps, const float* w_flow, const float* b_flow,
                                       const float* w_occ, const float* b_occ, const float* x0, int ld0, int c0, const float* x1, int ld1,
                                       int c1, const float* w_extra, float* out, int batch, int frames, int hw, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sampler step (GaussianDiffusion.ddim_sample :791-827 / p_sample :737-746): predict x0
 * (:697-701), dynamic threshold = per-sample 0.9-quantile of |x0| with linear interpolation,
 * clamp and divide (:805-818), then the update.  Coefficients come from a device table indexed
 * by a device step counter, so the whole step can be replayed from a hipGraph:
 *   x0 = c_x*x - c_eps*eps;  s = max(1, quantile(|x0|) per sample);  m = clamp(x0, -s, s) / s
 *   DDIM / DDPM:  coef[step] = { c_x, c_eps, k_x0, k_eps, k_x, k_noise }:  x <- k_x0*m + k_eps*eps + k_x*x + k_noise*noise
 *   multistep:    coef[step] = { c_x, c_eps, k_x, k_m, k_prev, unused }:   x <- k_x*x + k_m*m + k_prev*hist;  hist <- m
 * (c_x = sqrt_recip_alphas_cumprod, c_eps = sqrt_recipm1_alphas_cumprod; multistep = DPM-Solver++, Lu et al. 2022, "2M" and its first-order
 * form, on the THRESHOLDED data prediction).  A coefficient that is exactly 0 skips its operand.
 * One entry point, one parameter struct (ABI version 13; it replaces the nine positional lfdm_sampler_step_*_f32 forms of ABI 12 - migration
 * table in INTEGRATION.md).  Which of the update kernel's instantiations runs follows from the fields that are set; the launch sequence
 * (histogram clear for batch > 2, x0 pass, two select passes, update) is the same for all of them.
 * Refusals (LFDM_EINVAL, nothing is enqueued): a null required operand or n outside (0, 2^24); exactly one of seeds / window; seeds with
 * noise; seeds with multistep (the multistep update draws nothing); in `known`: some but not all of known / known_noise / a mask / level,
 * both masks (they exclude each other), elem_mask with frames or frame_elems set, a frame split that does not divide n.
 */
/* Known content for the replacement method (per element 4.11): the final store of x is replaced, where a byte mask marks it, by
 *   x[b, i] <- a * known[b, i] + s * known_noise[b, i],   (a, s) = level[2 * (step + 1)]
 * It is a select, never a blend: known / known_noise at unmarked positions are never read into a result and may be NaN or uninitialised.  x0, the
 * threshold (over the whole sample), x0_out, hist and the step counter are exactly what the unconditioned step computes.
 * All zero = no conditioning.  Otherwise known, known_noise, level and exactly ONE of the masks. */
typedef struct lfdm_known_operands {
  const float* known;               /* dense (B, n) */
  const float* known_noise;         /* dense (B, n) */
  const unsigned char* frame_mask;  /* frame form: dense (B, frames) bytes, non-zero = frame (i / frame_elems) % frames of sample b is known */
  const unsigned char* elem_mask;   /* element form: dense (B, n) bytes, non-zero = element i of sample b is known (any subset: a region, a channel, a pixel) */
  const float* level;               /* dense (steps + 1, 2) on the device: row 0 = the level of x_T, row i + 1 = (a, s) after step i; indexed by the
                                       step counter like coef, read before it is advanced.  Not an operand of lfdm_known_blend_f32 (leave NULL) */
  int frames;                       /* frame form only (0 with elem_mask): n must be a multiple of frames * frame_elems */
  int64_t frame_elems;              /* frame form only: elements per frame (planar (C, T, S, S): S * S) */
} lfdm_known_operands;
typedef struct lfdm_sampler_step_params {
  float* x;                /* dense planar (B, n), n = 3*T*S*S; in/out */
  const float* eps;        /* dense (B, n): the model's prediction */
  const float* noise;      /* dense (B, n) or NULL (no noise term); must be NULL with seeds; ignored with multistep */
  float* hist;             /* multistep only, dense (B, n), in/out: m of the previous step on entry, m of this step on return (each element is
                              read, then written, by one thread; it must not alias x, eps or x0_out).  A first-order row (k_prev == 0: the first and
                              the last step of a video) may be handed UNINITIALISED memory, NaNs included */
  const uint64_t* seeds;   /* counter-based step noise, with window or not at all: `batch` 64-bit words on the device.  The noise term
                              is computed inside the update kernel, noise[b, i] = z of (seeds[b], counter (i >> 2, *step_dev, 2, *window)), element
                              i & 3 of its quad - bit for bit what lfdm_philox_normal_f32 writes for stream_id 2, step = *step_dev */
  const uint32_t* window;  /* one 32-bit word on the device: the window number (0 for one video); one captured graph serves every seed and window */
  float* x0_out;           /* NULL or dense (B, n): receives m */
  int batch;
  int64_t n;               /* elements per sample, 0 < n < 2^24 */
  const float* coef;       /* dense (steps, 6) on the device, rows as above */
  int32_t* step_dev;       /* the device step counter: row index of coef and level */
  float quantile;          /* in [0, 1]; negative = the static branch of the reference (use_dynamic_thres=False: x0.clamp(-1, 1), :729-732) */
  int advance;             /* != 0: the step increments *step_dev at its end */
  void* ws;                /* lfdm_sampler_ws_bytes, and it MUST have been cleared once by lfdm_sampler_ws_init: the step relies on histograms and an
                              end-of-step ticket word that every step leaves zeroed for the next one.  A workspace that was never initialised gives
                              wrong dynamic thresholds and a step counter that never advances - and no error code: the library cannot look into
                              device memory without a synchronisation.  One workspace may serve every form of the step */
  size_t ws_bytes;
  int multistep;           /* != 0: the multistep update (hist required); seeds is refused */
  lfdm_known_operands known;
} lfdm_sampler_step_params;
size_t lfdm_sampler_ws_bytes(int batch, int64_t n);
/* once per workspace, before its first lfdm_sampler_step_f32: clears the histograms and the end-of-step ticket (every step leaves
 * them cleared again: its last workgroup does the housekeeping, incl. the step-counter increment) */
int lfdm_sampler_ws_init(void* ws, size_t ws_bytes, int batch, int64_t n, lfdm_stream_t stream);
/* Layout: every operand dense, as stated at its field.  The struct is read during the call only. */
int lfdm_sampler_step_f32(const lfdm_sampler_step_params* p, lfdm_stream_t stream);
/* the known select with host scalars, for x_T (once per video, outside the replayed step): x <- a * known + s * known_noise where the mask of
 * `k` marks it (with an all-set elem_mask: everywhere, the entry of a schedule on a given latent).  k->level is not an operand. */
/* Layout: x dense (B, n), the operands of k as stated at its fields.  x must not alias known or known_noise. */
int lfdm_known_blend_f32(float* x, const lfdm_known_operands* k, float a, float s, int batch, int64_t n, lfdm_stream_t stream);
/* Counter-based noise (additive, ABI version unchanged; DESIGN.md 4.10, csrc/lfdm_philox.h): every normal is a pure function of
 * (video seed, window, stream, step, element).  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85,
 * ten rounds) with key = (seed & 0xffffffff, seed >> 32) and counter = (i >> 2, step, stream_id, window) gives four words r0..r3 for the quad
 * of element i of one video's flat latent; u(r) = ((r >> 8) + 0.5) * 2^-24 in fp32 arithmetic;  R(r) = sqrt(-2 ln u(r));
 *   z[4q] = R(r0) cos(2 pi u(r1)), z[4q+1] = R(r0) sin(2 pi u(r1)), z[4q+2] = R(r2) cos(2 pi u(r3)), z[4q+3] = R(r2) sin(2 pi u(r3)),  |z| <= 5.89.
 * stream_id: 0 = x_T, 1 = known-frame noise, 2 = step noise.  step: the sampler step index (0 for the two per-video draws).  window: 0 for one
 * video, the window number in a long video.  seeds: `batch` unsigned 64-bit words ON THE DEVICE.  0 < n < 2^24, row_stride >= n.
 * lfdm_philox_normal_f32 writes z, lfdm_philox_bits_u32 the raw words (out[b * row_stride + i] = r_{i & 3} of quad i >> 2; for tests). */
/* Layout: out is `batch` rows of n adjacent values, row b at out + b * row_stride (any row_stride >= n, any 4-byte aligned base: rows whose
 * base is 16-byte aligned are stored in 16-byte words, other rows and the ragged last quad element by element); nothing outside the rows is
 * written.  seeds dense. */
int lfdm_philox_normal_f32(float* out, const uint64_t* seeds, int batch, int64_t n, int64_t row_stride, unsigned stream_id, unsigned step,
                           unsigned window, lfdm_stream_t stream);
/* Layout: as lfdm_philox_normal_f32. */
int lfdm_philox_bits_u32(uint32_t* out, const uint64_t* seeds, int batch, int64_t n, int64_t row_stride, unsigned stream_id, unsigned step,
                         unsigned window, lfdm_stream_t stream);
/* classifier-free guidance combine of Unet3D.forward_with_cond_scale (:525-526):
 * out = null_eps + (cond_eps - null_eps) * scale   (out may alias an input) */
/* Layout: dense, any; out may alias cond_eps or null_eps. */
int lfdm_cfg_combine_f32(const float* cond_eps, const float* null_eps, float scale, float* out,
                         int64_t n, lfdm_stream_t stream);
/* The guidance combine with the rescale of Lin et al. 2024 (additive, ABI version unchanged):
 *   g = null_eps + (cond_eps - null_eps) * scale  (the bits of lfdm_cfg_combine_f32),   out = g * (phi * std(cond_eps) / std(g) + 1 - phi)
 * with both standard deviations per sample over its n elements, unbiased (n - 1), summed and formed in double; the factor is rounded to fp32
 * once and is 1 where std(g) == 0.  phi in [0, 1]; phi = 0 gives lfdm_cfg_combine_f32's bits.  factor_out: NULL or `batch` floats, the factor
 * of each sample.  ws: lfdm_cfg_rescale_ws_bytes(batch, n) bytes, 8-byte aligned, written and read by this call only (no state between
 * calls).  Two launches, no atomics: the same bits on every run, and a sample's bits do not depend on the batch around it.  Refused with
 * LFDM_EINVAL, nothing touched: n < 2, batch <= 0 (or > 65535), a null pointer, phi outside [0, 1], a workspace that is too small. */
size_t lfdm_cfg_rescale_ws_bytes(int batch, int64_t n);
/* Layout: cond_eps, null_eps and out dense (batch, n), any 4-byte aligned base (a sample whose bases are 16-byte aligned moves in 16-byte
 * words, any other element by element - the same bits); out may alias cond_eps or null_eps; factor_out dense (batch). */
int lfdm_cfg_combine_rescale_f32(const float* cond_eps, const float* null_eps, float scale, float phi, float* out, float* factor_out,
                                 int batch, int64_t n, void* ws, size_t ws_bytes, lfdm_stream_t stream);
/* stand-alone |x| quantile (torch.quantile semantics, :722-726) for tests: q_out[b] */
int lfdm_abs_quantile_f32(const float* x, int batch, int64_t n, float quantile, float* q_out,
                          void* ws, size_t ws_bytes, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * LFAE warp: Generator.deform_input + apply_optical (LFAE/modules/generator.py:59-88):
 * bilinear resize of the low-res sampling grid / occlusion map to the feature resolution
 * (F.interpolate align_corners=False, :65,:80) fused with grid_sample (bilinear, zeros,
 * align_corners=False, :67) and the occlusion blend out = w*occ + prev*(1-occ) (:82-84).
 * flow_x/flow_y/occ: low-res maps addressed as  base[b*sb + t*st + y*fw + x]  so the planar
 * DM prediction (B,3,T,S,S) is read in place (occ_scale/occ_bias map it to [0,1]: 0.5/0.5 for
 * the raw prediction, 1/0 for a ready occlusion map; occ may be NULL = no masking).
 */
typedef struct lfdm_warp_params {
  const float* src;      /* CL (B, H, W, C) rows (ld_src) or planar (B, C, H, W) */
  const float* prev;     /* NULL or rows (B*T, H, W, C) (ld_prev) / planar like out */
  float* out;            /* CL (B*T, H, W, C) rows (ld_out) or planar (B, C, T, H, W) */
  int batch, frames, h, w, c;
  int ld_src, ld_prev, ld_out;
  const float* flow_x;
  const float* flow_y;
  const float* occ;
  int fh, fw;            /* low-res map size */
  int64_t fsb, fst;      /* batch / frame strides (floats) of the maps */
  float occ_scale, occ_bias;
  int prev_is_cl;        /* planar kernel only: prev given as CL rows (ld_prev) */
} lfdm_warp_params;

/* Layout: warp_cl: src (ld_src), prev (ld_prev), out (ld_out): 16 B, ld % 4, C % 4.  warp_planar: src, out dense planar (src any: the plane kernel
 * stages 16 B planes with float4 and others with scalar loads), prev as CL rows (ld_prev): any.  flow_x / flow_y / occ: any (fsb, fst in floats). */
int lfdm_warp_cl_f32(const lfdm_warp_params* p, lfdm_stream_t stream);
int lfdm_warp_planar_f32(const lfdm_warp_params* p, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Element-wise / layout helpers of the LFAE decode path.
 * affine_act: y = act(x*a[c] + b[c])  (eval BatchNorm + ReLU of ResBlock2d, util.py:84-90)
 * avgpool2:   2x2 average pool (DownBlock2d, util.py:124)
 */
/* Layout: affine_act: x (ldx), out (ldo), a, b: 16 B, ld % 4, C % 4; out may alias x.  avgpool2: x, out dense, 16 B.  planar_to_cl: out (ldo) any.
 * cl_to_planar: x (ldx) any.  Both transposes: n_img <= 65535 (grid z) and C <= 65535 * 32 (grid y); more is refused with LFDM_EINVAL,
 * nothing launched. */
int lfdm_affine_act_cl_f32(const float* x, float* out, int64_t rows, int channels, int ldx,
                           int ldo, const float* a, const float* b, int act,
                           lfdm_stream_t stream);
int lfdm_avgpool2_cl_f32(const float* x, float* out, int n_img, int h, int w, int channels,
                         lfdm_stream_t stream);
int lfdm_planar_to_cl_f32(const float* x, float* out, int n_img, int channels, int hw, int ldo,
                          lfdm_stream_t stream);
int lfdm_cl_to_planar_f32(const float* x, float* out, int n_img, int channels, int hw, int ldx,
                          lfdm_stream_t stream);

/* PreNorm LayerNorm + to_qkv + temporal Attention (without to_out) in one launch, for C % 64 == 0:
 * video_flow_diffusion.py:170-189 (LayerNorm, PreNorm), :270-283 (einops re-layout), :303-361 (Attention incl.
 * rotary :329-331 and relative position bias :339-340).  x: CL rows (B*T*HW, C) stride ldx; wqkv: the to_qkv weight
 * (768, C) row-major with the LayerNorm gamma folded in (w[n][c] * gamma[c]); out: rows of 256 (heads merged).
 * The 768-wide qkv tensor is never materialised. */
/* Layout: x (ldx), wqkv: 16 B, ldx % 4; out dense rows of 256; bias any (float4 loads when 16 B and frames % 4 == 0, scalar otherwise). */
int lfdm_temporal_attention_fused_cl_f32(const float* x, int ldx, int channels, const float* wqkv, float* out,
                                         int batch, int frames, int hw, const float* bias,
                                         const float* rot_cos, const float* rot_sin, float ln_eps,
                                         lfdm_stream_t stream);
/* The same block COMPLETE in one launch (ABI version 8): out = x + to_out(attention(LayerNorm(x))) - Residual(PreNorm(EinopsToAndFrom(
 * Attention))), video_flow_diffusion.py:170-189, 270-283, 286-363 incl. to_out (:301, no bias) and the residual add (:165).  Both weights
 * in MFMA-operand order, lane = 16 * lq + l15 (cvpr23_lfdm_amd.ops.pack_tattn_weights):
 *   wqkv [3 = q|k|v][8 heads][2 feature halves][4 quads][64 lanes][4]  <-  (W_qkv * gamma)[which*256 + head*32 + 16*half + l15][16*lq + 4*quad + e]
 *   wout [4 column tiles][16 steps S][64 lanes][4]                      <-  W_out[16*ct + l15][16*S + 4*lq + e]
 * out (rows, C) with row stride ldo, out != x.  C == 64 only (the finest UNet levels). */
/* Layout: x (ldx), wqkv, wout: 16 B, ldx % 4; out (ldo): any, out != x; bias as above. */
int lfdm_temporal_attention_fused_out_cl_f32(const float* x, int ldx, int channels, const float* wqkv, const float* wout, float* out,
                                             int ldo, int batch, int frames, int hw, const float* bias, const float* rot_cos,
                                             const float* rot_sin, float ln_eps, lfdm_stream_t stream);

/* PreNorm LayerNorm + to_qkv (1x1 conv, no bias) + SpatialLinearAttention core (without to_out) for C == 64:
 * video_flow_diffusion.py:170-189, :249-263.  x: CL rows (n_frames*hw, C) stride ldx; wqkv (768, C) row-major with the
 * LayerNorm gamma folded in; out rows of 256.  qkv is never materialised (every pass recomputes its projection). 
 * wqkv (ABI version 8): the LayerNorm-folded (768, 64) weight in MFMA-operand order [3 = q|k|v][8 heads][8 quads][64 lanes = 32*kh + l31][4]
 * <- W[which*256 + head*32 + l31][32*kh + 4*quad + e] (cvpr23_lfdm_amd.ops.pack_linattn_weights): every fragment load = one contiguous 1 KB. */
/* Layout: x (ldx), wqkv: 16 B, ldx % 4; out dense rows of 256. */
size_t lfdm_linear_attention_fused_ws_bytes(int n_frames, int hw);
int lfdm_linear_attention_fused_cl_f32(const float* x, int ldx, int channels, const float* wqkv, float* out,
                                       int n_frames, int hw, float ln_eps, void* ws, size_t ws_bytes,
                                       lfdm_stream_t stream);
/* ... and the WHOLE block Residual(PreNorm(SpatialLinearAttention)) at C == 64 (ABI version 12; video_flow_diffusion.py:170-189, :240-265 incl. to_out,
 * its bias and the residual add): out[row][c] = x[row][c] + bias_out[c] + sum_k attention(LayerNorm(x))[row][k] Wout[c][k], rows of 64 with stride ldo,
 * out != x.  The 256-column attention output is never written: the merge pass folds to_out into the context (Mt_h = Wout_h ctx_h^T, 64 x 32 per
 * (frame, head)) and the output pass multiplies the softmaxed q accumulator by it (one launch and 84 MB of traffic less than
 * lfdm_linear_attention_fused_cl_f32 + a 1x1 convolution at 40 frames of 32x32).  wout: the
 * (64, 256) to_out weight in MFMA-operand order [8 heads][2 row blocks][4 quads][64 lanes = 32*kh + c_local][4] <- Wout[32*cb + c_local][32*h + 8*quad + 4*kh + e]
 * (cvpr23_lfdm_amd.ops.pack_linattn_out_weight); bias_out (64,) or NULL; same workspace as above. */
/* Layout: x (ldx), out (ldo), wqkv, wout, bias_out: 16 B, ld % 4; out != x. */
int lfdm_linear_attention_fused_out_cl_f32(const float* x, int ldx, int channels, const float* wqkv, const float* wout, const float* bias_out,
                                           float* out, int ldo, int n_frames, int hw, float ln_eps, void* ws, size_t ws_bytes,
                                           lfdm_stream_t stream);

/* The same two blocks - PreNorm LayerNorm + to_qkv + attention core, without to_out - as ONE launch for the low-resolution levels
 * (C % 64 == 0 channels, a few hundred to a few thousand rows), where separate projection / reduce / core launches sit at their
 * launch latency: one workgroup per (frame, head) resp. (sequence, head) projects its rows with the head's 96 filter rows (fp32
 * MFMA, K split over the wavefronts), keeps q | k | v in LDS and writes the head's 32 output columns.
 * wqkv: (768, C) row-major with the LayerNorm gamma folded in; wsum[o] = sum_c wqkv[o][c] (768 floats: the algebraic LayerNorm fold
 * y = rstd * (x.W' - mean * wsum)); out: rows of 256.
 * lfdm_linear_attention_lowres_cl_f32: SpatialLinearAttention (video_flow_diffusion.py:240-265), hw <= 64 or 192 < hw <= 256 pixels
 * per frame.  lfdm_attention_lowres_cl_f32: Attention (:286-363); mode 0 = over the frames of a pixel (rot_cos / rot_sin (T,16), bias
 * (8,T,T) as in lfdm_attention_cl_f32), mode 1 = over the pixels of a frame (mid block); at most 64 tokens per sequence. */
/* Layout (both): x (ldx), wqkv, out (dense rows of 256): 16 B, ldx % 4. */
int lfdm_linear_attention_lowres_cl_f32(const float* x, int ldx, int channels, const float* wqkv, const float* wsum, float* out,
                                        int n_frames, int hw, float ln_eps, lfdm_stream_t stream);
int lfdm_attention_lowres_cl_f32(const float* x, int ldx, int channels, const float* wqkv, const float* wsum, float* out, int batch,
                                 int frames, int hw, int mode, const float* bias, const float* rot_cos, const float* rot_sin,
                                 float ln_eps, lfdm_stream_t stream);

/* Winograd F(2x2,3x3) filter transform U = G g G^T into the operand layout of lfdm_conv_params.weight_wino:
 * out[16][cin/16][coutp][16] (zero for output channels >= cout).  w: 3x3 filters of the reference layout
 * (Cout, Cin, 3, 3) (video_flow_diffusion.py:197 Block.proj / LFAE util.py:73-76 ResBlock2d); element (o, i, a, b) at
 * w[o*ld_o + i*9 + a*3 + b], so a channel slice [lo, hi) of the input axis is w + lo*9 with ld_o = Cin_total*9.
 * dgrad != 0 builds the filters of the data-gradient convolution instead (roles of the channel axes exchanged, taps
 * flipped): the result convolves dY (cout channels) into dX (cin channels); then cout % 16 == 0 is required and
 * coutp >= cin.  dgrad == 0 requires cin % 16 == 0 and coutp >= cout; coutp % 32 == 0. */
/* Layout (the four Winograd packers, the per-job ld_o of lfdm_pack_wino_weights_multi_f32 included): w (ld_o >= cin*9 floats between output channels): any -
 * an input-channel slice of a wider filter is read where it lies, nothing of the filter outside the slice is read; out dense (bf16: 16 B). */
int lfdm_pack_wino_weight_f32(const float* w, int ld_o, int cout, int cin, int coutp, int dgrad, float* out,
                              lfdm_stream_t stream);
/* the F(4x4,3x3) filters of lfdm_conv_params.weight_wino4: out[36][cin/8][coutp][8] (zero for output channels >= cout), same `w`
 * addressing as above; cin % 8 == 0, coutp % 32 == 0, coutp >= cout.  (ABI version 5.) */
int lfdm_pack_wino4_weight_f32(const float* w, int ld_o, int cout, int cin, int coutp, float* out, lfdm_stream_t stream);
/* the bf16 operands of lfdm_conv2d_cl_wino_bf16: out[16][cin/16][coutp][16] of 16-bit bf16 words (last axis: k-slot kh, then 8 channels -
 * the channel inside the chunk, in order), each the round-to-nearest-even bf16 of the element lfdm_pack_wino_weight_f32 (dgrad = 0) holds
 * for the same filter (zero for output channels >= cout).  Same `w` addressing; cin % 16 == 0, coutp % 32 == 0, coutp >= cout, out 16-byte aligned. */
int lfdm_pack_wino_weight_bf16(const float* w, int ld_o, int cout, int cin, int coutp, void* out, lfdm_stream_t stream);

/* PixelwiseFlowPredictor around its hourglass (LFAE/modules/pixelwise_flow_predictor.py:48-128) for all N = batch*frames driving
 * frames of a training step, frame n = b*frames + t using source image / source regions b:
 * lfdm_lfae_motion_inputs_f32: heat-map representation (:48-65: Gaussian of the driving minus the source region, covariances
 * (N|B, K, 2, 2) or - both NULL - the constant region_var), sparse motions (:67-93: identity grid - driving shift, through
 * src_affine . drv_affine^-1 (times the sign of its [0][0] entry when revert_axis_swap) when the affines are given, + source
 * shift; region 0 = background: the identity grid through the 3x3 homography bg (N, 3, 3), or as is when NULL) and the K+1
 * bilinear / zero-padded / align_corners=False samples of the 3-channel source image src_img (B, 3, h, w) (:95-102).
 * rows: channels-last hourglass input (N*h*w, ld), channel 4*kk + {0: heat, 1..3: warped image}, columns >= 4*(K+1)
 * zeroed; sparse: (N, K+1, h, w, 2).
 * lfdm_lfae_motion_combine_f32: (:112-128) heads = channels-last rows (N*hw, ldh) of the mask (columns 0..K) and occlusion
 * (column K+1, read iff occ != NULL) convolutions: flow (N, h, w, 2) = sum_k softmax_k(mask) * sparse_k,
 * occ (N, 1, h, w) = sigmoid. */
/* Layout: motion_inputs: rows (ld): 16 B, ld % 4, ld >= 4*(regions+1); DELIBERATE EXCEPTION to the gap rule: the columns 4*(regions+1) ... ld-1 of every row are
 * WRITTEN as zero (ld is the consumer's channel count); sparse 8 B; the inputs dense.  region_stats: logits (ldh): any.  motion_combine: heads (ldh): any; sparse, flow 8 B. */
int lfdm_lfae_motion_inputs_f32(const float* src_img, const float* drv_shift, const float* drv_covar, const float* drv_affine,
                                const float* src_shift, const float* src_covar, const float* src_affine, const float* bg,
                                float region_var, int revert_axis_swap, int batch, int frames, int regions, int h, int w,
                                float* rows, int ld, float* sparse, lfdm_stream_t stream);
/* RegionPredictor tail (LFAE/modules/region_predictor.py:16-25,60-96) for n_img frames in one launch.  logits: channels-last
 * rows (n_img*h*w, ldh) of the `regions` head convolution, column k = region k.  heatmap (n_img, K, h, w) = spatial softmax of
 * logits / temperature; shift (n_img, K, 2) = its centre on the [-1, 1] grid; covar (n_img, K, 2, 2) = its covariance;
 * u (n_img*K, 2, 2), d (n_img*K, 2, 2) = diag(sqrt(S)) and affine (n_img, K, 2, 2) = U sqrt(S) from the covariance's SVD with
 * LAPACK xGESDD's sign convention (what torch.svd returns for a 2x2 input; closed form, no host round trip).  h*w <= 4096. */
int lfdm_lfae_region_stats_f32(const float* logits, int ldh, int n_img, int regions, int h, int w, float temperature,
                               float* heatmap, float* shift, float* covar, float* affine, float* u, float* d,
                               lfdm_stream_t stream);
/* (U, S) of n symmetric 2x2 matrices [[a, b], [b, c]] given as abc (n, 3), exactly as LAPACK xGESDD / torch.svd return them
 * (singular values descending, U's signs included) - the closed form lfdm_lfae_region_stats_f32 uses.  u (n, 2, 2), s (n, 2). */
int lfdm_svd2x2_sym_f32(const float* abc, int64_t n, float* u, float* s, lfdm_stream_t stream);
int lfdm_lfae_motion_combine_f32(const float* heads, int ldh, const float* sparse, int n_img, int regions, int hw, float* flow,
                                 float* occ, lfdm_stream_t stream);

/* Direct-form filter pack of lfdm_conv_params.weight ([ceil(K/32)][coutp][32], k contiguous per output column, zero padded)
 * from a weight in the reference layout, in ONE launch - training re-packs every filter every step
 * (video_flow_diffusion_model.py:181-188), the torch formulation costs three to five small kernels per filter.
 * w: element (o, i, tap) at w[o*stride_o + i*stride_i + tap], taps = kh*kw contiguous (a channel slice of either axis is a
 * pointer offset).  mode 0: the filter of the convolution itself, w = (Cout = n_o, Cin = n_i): K index tap*n_i + i, column o.
 * mode 1: the filter of its data-gradient convolution (channel roles exchanged, taps reversed): K index tap*n_o + o,
 * column i.  mode 2: the four parity packs of a ConvTranspose k4 s2 p1 with w = (Cin = n_o, Cout = n_i, 4, 4) (taps == 16),
 * stacked (4, 4*n_o/32 chunks, coutp, 32) in parity order 2*py + px = the `deconv4` operand (Upsample :156-158; also the
 * data gradient of Downsample :166-167 with the channel roles of its weight).  out holds round_up(K,32) * round_up(N,32)
 * floats (x4 for mode 2). */
int lfdm_pack_conv_weight_f32(const float* w, int n_o, int n_i, int taps, int64_t stride_o, int64_t stride_i, int mode,
                              float* out, lfdm_stream_t stream);

/* Convolution with at most 4 output channels on v_mfma_f32_4x4x1 (sixteen 4x4 blocks per instruction, lane = output
 * pixel): the LFAE generator's final Conv2d(64 -> 3, 7x7) + sigmoid (LFAE/modules/generator.py:54,161-162).
 * x: CL rows (n_img*h*w, cin) stride ldx; wgt: [k*k][cin][4] (tap-major, filters innermost, zero padded to 4);
 * bias: 4 floats or NULL; out: CL rows stride ldo (only `cout` columns are written); stride 1, zero padding k/2.
 * x and wgt 16-byte aligned, ldx % 4 == 0, cin % 16 == 0, odd k <= 7 (LFDM_EINVAL otherwise). */
/* Layout: x (ldx), wgt: 16 B, ldx % 4; out (ldo >= cout): any - exactly `cout` columns of a row are written, the rest of a 4-wide row is a gap. */
int lfdm_conv2d_smalln_cl_f32(const float* x, int ldx, int cin, int n_img, int h, int w, const float* wgt,
                              const float* bias, float* out, int ldo, int cout, int k, int act,
                              lfdm_stream_t stream);

/* ==========================================================================================
 * TRAINING (backward) kernels - the DM gradient step of
 * DM/modules/video_flow_diffusion_model.py:181-188 (loss.backward(); optimizer_diff.step()).
 * Data gradients of convolutions are convolutions with re-packed weights (lfdm_conv2d_cl_f32).
 * ========================================================================================== */

/* Weight gradient of every Conv3d k=(1,kh,kw) / Linear of Unet3D
 * (video_flow_diffusion.py:199,224,246-247,300-301,158,167,410):
 *   dw[(ky*kw + kx)][ci][co] = sum over output pixels r = (n, qy, qx) of
 *        x[n, qy*stride + ky - pad_y, qx*stride + kx - pad_x][ci] * dy[r][co]      (zeros outside)
 * x: CL rows (n_img*hi*wi, cin) stride ldx; dy: CL rows (n_img*hq*wq, cout) stride lddy.
 * The tap-major result (dw_layout = 0) is a plain permutation of the reference (cout, cin, 1, kh, kw) layout;
 * dw_layout = 1 (filters of <= 16 taps) writes that layout directly - dw[(co*dw_cin_total + dw_ci_off + ci)*kh*kw + tap],
 * so the two halves of a convolution over cat(x0, x1) land in one tensor and the result can BE the optimizer's
 * gradient slot (no permute copy, no gradient staging copy).  dbias != NULL also returns the bias gradient
 * (column sums of dy, video_flow_diffusion.py:199 bias=True) from the same pass over dy.
 * A ConvTranspose weight gradient is the same call with the roles of x and dy exchanged (stride 2):
 * dw_layout = 1 then yields the (cin, cout, 4, 4) ConvTranspose layout.  Sums are taken in a fixed order. */
typedef struct lfdm_wgrad_params {
  const float* x;
  int cin, ldx;
  int n_img, hi, wi;
  int hq, wq;
  int stride, kh, kw, pad_y, pad_x;
  const float* dy;
  int cout, lddy;
  float* dw;              /* dw_layout 0: [kh*kw][cin][cout]; 1: [cout][dw_cin_total][kh*kw] */
  int dw_layout;          /* 0 | 1 */
  int dw_cin_total;       /* (layout 1) input channels of the whole filter */
  int dw_ci_off;          /* (layout 1) this call's first input channel */
  float* dbias;           /* optional (cout): sum over rows of dy */
} lfdm_wgrad_params;
/* Layout: x (ldx), dy (lddy): 16 B, ld % 4, cin % 4, cout % 4 (a channel slice of a wider activation is a pointer offset); dw, dbias dense. */
size_t lfdm_conv2d_wgrad_ws_bytes(const lfdm_wgrad_params* p);
int lfdm_conv2d_wgrad_cl_f32(const lfdm_wgrad_params* p, void* ws, size_t ws_bytes, lfdm_stream_t stream);

/* out[i] = sum_s in[s*n + i], s in fixed order (second stage of every deterministic split reduction) */
/* Layout: dense, any (float4 form when n % 4 == 0 and both pointers 16 B, scalar otherwise). */
int lfdm_sum_leading_f32(const float* in, float* out, int64_t n, int s, lfdm_stream_t stream);

/* Bias gradient: out[c] = sum_r x[r][c] over CL rows (stride ld). */
/* Layout: x (ld): any. */
size_t lfdm_colsum_ws_bytes(int64_t rows, int c);
int lfdm_colsum_f32(const float* x, int64_t rows, int c, int ld, float* out, void* ws, size_t ws_bytes,
                    lfdm_stream_t stream);

/* Backward of lfdm_groupnorm_silu_cl_f32 (Block.forward norm/scale-shift/act, video_flow_diffusion.py:200-211).
 * x: the forward INPUT rows, dy: gradient of the output (before any residual add), partial/nchunk: the
 * (sum, sumsq) partials the forward pass used (first batch*nchunk*groups*2 floats of its workspace, or the
 * convolution's gn_partial).  Outputs: dx rows; dgamma_dbeta = [dgamma(C) | dbeta(C)];
 * dscale_shift (when scale_shift != NULL) = B rows [dscale(C) | dshift(C)] with stride dss_ld. */
/* Layout: x, dy, dx dense rows of C floats, 16 B; partial 8 B; scale_shift (ss_ld), dscale_shift (dss_ld): any. */
size_t lfdm_groupnorm_bwd_ws_bytes(int batch, int pixels, int channels);
int lfdm_groupnorm_silu_bwd_cl_f32(const float* x, const float* dy, float* dx, int batch, int pixels,
                                   int channels, int groups, const float* gamma, const float* beta,
                                   const float* scale_shift, int ss_ld, float eps, int apply_silu,
                                   const float* partial, int nchunk, float* dgamma_dbeta,
                                   float* dscale_shift, int dss_ld, void* ws, size_t ws_bytes,
                                   lfdm_stream_t stream);

/* Backward of lfdm_layernorm_cl_f32 (LayerNorm, video_flow_diffusion.py:170-179): dx rows and dgamma (C). */
/* Layout (both forms): x, dy, dx, dx_add dense rows, gamma: 16 B. */
size_t lfdm_layernorm_bwd_ws_bytes(int64_t rows, int channels);
int lfdm_layernorm_bwd_cl_f32(const float* x, const float* dy, float* dx, int64_t rows, int channels,
                              const float* gamma, float eps, float* dgamma, void* ws, size_t ws_bytes,
                              lfdm_stream_t stream);
/* The same with dx = (LayerNorm gradient) + dx_add (ABI 11; dx_add rows x C, may be NULL): the residual path's gradient of the pre-norm
 * blocks (Residual(PreNorm(...)), video_flow_diffusion.py:118-125, :181-188) summed in the kernel's store instead of by an ATen add. */
int lfdm_layernorm_bwd_add_cl_f32(const float* x, const float* dy, const float* dx_add, float* dx, int64_t rows, int channels,
                                  const float* gamma, float eps, float* dgamma, void* ws, size_t ws_bytes, lfdm_stream_t stream);

/* Backward of lfdm_attention_cl_f32 (Attention.forward, video_flow_diffusion.py:303-363): dqkv rows
 * (768 = [dq | dk | dv], same order as qkv) from the saved qkv rows and dout (rows of 256).  Scores and
 * softmax are recomputed.  dbias (8, L, L) = gradient of the relative-position bias table (must be given
 * iff bias is; the embedding gradient is its scatter by bucket, done by the caller).
 * ws: lfdm_attention_bwd_ws_bytes (per-wavefront bias partials, summed in a fixed order). */
size_t lfdm_attention_bwd_ws_bytes(int batch, int frames, int hw, int mode);
int lfdm_attention_bwd_cl_f32(const float* qkv, const float* dout, float* dqkv, int batch, int frames,
                              int hw, int mode, const float* bias, const float* rot_cos,
                              const float* rot_sin, float* dbias, void* ws, size_t ws_bytes,
                              lfdm_stream_t stream);

/* Long attention (additive under ABI 12; csrc/attention_long.hip): the same attention over 65 <= L <= 256 tokens per sequence, streaming
 * key / value tiles of 16 tokens past a resident block of queries (two-sweep softmax: exact row maximum first, then exp / sum / P V).
 * Arguments, row layouts, modes, bias (8, L, L) and rotary tables (L, 16) exactly as lfdm_attention_cl_f32 / lfdm_attention_bwd_cl_f32.
 * L <= 64 is refused (LFDM_EINVAL: the short kernels own that range, nothing is dispatched twice), L > 256 is refused with a message
 * naming 256; a refused call writes nothing.
 *   forward:  stats (may be NULL) receives, per (sequence, head), the row maxima and the row sums of exp(s - max):
 *             (nseq * 8, 2, L) floats, nseq = batch * hw (mode 0) or batch * frames (mode 1).
 *   backward: two-phase flash form, P and dP recomputed from qkv (nothing else saved), dbias iff bias; no atomics, every output element
 *             has one owner, bias partials summed in a fixed order: bit-identical from run to run.  ws is ALWAYS required, 16-byte
 *             aligned, lfdm_attention_long_bwd_ws_bytes: 3 * nseq * 8 * roundup(L, 16) floats of row statistics plus
 *             G * 8 * L * L floats of bias partials, G = min(nseq, max(1, 2048 / (8 * ceil(L / 16)))) - at most 32 MB, independent of
 *             batch * hw.  The query returns 0 for a shape the entry point refuses. */
int lfdm_attention_long_cl_f32(const float* qkv, float* out, int batch, int frames, int hw, int mode,
                               const float* bias, const float* rot_cos, const float* rot_sin, float* stats,
                               lfdm_stream_t stream);
size_t lfdm_attention_long_bwd_ws_bytes(int batch, int frames, int hw, int mode);
int lfdm_attention_long_bwd_cl_f32(const float* qkv, const float* dout, float* dqkv, int batch, int frames,
                                   int hw, int mode, const float* bias, const float* rot_cos,
                                   const float* rot_sin, float* dbias, void* ws, size_t ws_bytes,
                                   lfdm_stream_t stream);

/* Backward of lfdm_linear_attention_cl_f32 (SpatialLinearAttention core, :254-263): dqkv rows from qkv, dout. */
size_t lfdm_linear_attention_bwd_ws_bytes(int n_frames);
int lfdm_linear_attention_bwd_cl_f32(const float* qkv, const float* dout, float* dqkv, int n_frames,
                                     int hw, void* ws, size_t ws_bytes, lfdm_stream_t stream);

/* Small-batch Linear layers that share their INPUT, forward and backward in one launch each: the conditioning path of the
 * training step - ResnetBlock.mlp = SiLU -> Linear(cond_dim, 2*dim_out) of every block applied to the same (B, cond_dim)
 * vector (video_flow_diffusion.py:230-233,240-245,562) and time_mlp's Linear -> GELU -> Linear (:441-447).
 *   forward   y[j] = act(x) w[j]^T + bias[j]                        (rows, n[j])
 *   backward  dw[j] = dy[j]^T act(x); dbias[j] = colsum(dy[j]); dx = act'(x) * sum_j dy[j] w[j]
 * act applies to the input: 0 none, 1 SiLU, 2 GELU (erf form).  rows <= 16, k % 4 == 0, k <= 1024, n_blocks <= 32; all
 * tensors contiguous fp32, x / w / dw / dx 16-byte aligned.  Backward: dy[j] NULL = zero gradient; dw[j] / dbias[j] / dx
 * NULL = not wanted.  Sums in a fixed order. */
#define LFDM_MULTI_LINEAR_MAX 32
typedef struct lfdm_multi_linear_params {
  int n_blocks, rows, k, act;
  const float* x;                              /* (rows, k) */
  const float* w[LFDM_MULTI_LINEAR_MAX];       /* (n[j], k): torch Linear.weight */
  const float* bias[LFDM_MULTI_LINEAR_MAX];    /* (n[j]) or NULL */
  int n[LFDM_MULTI_LINEAR_MAX];
  float* y[LFDM_MULTI_LINEAR_MAX];             /* forward output (rows, n[j]) */
  const float* dy[LFDM_MULTI_LINEAR_MAX];      /* backward */
  float* dw[LFDM_MULTI_LINEAR_MAX];
  float* dbias[LFDM_MULTI_LINEAR_MAX];
  float* dx;                                   /* (rows, k) or NULL */
} lfdm_multi_linear_params;
/* Layout (forward and backward): dense; x, every w, every dw, dx and ws 16 B, k % 4 == 0. */
int lfdm_multi_linear_f32(const lfdm_multi_linear_params* p, lfdm_stream_t stream);
size_t lfdm_multi_linear_bwd_ws_bytes(const lfdm_multi_linear_params* p);
int lfdm_multi_linear_bwd_f32(const lfdm_multi_linear_params* p, void* ws, size_t ws_bytes, lfdm_stream_t stream);

/* Fused Adam over one flat parameter buffer: torch.optim.Adam(betas, eps, weight_decay) semantics (no amsgrad),
 * video_flow_diffusion_model.py:113-114,188.  grad is multiplied by grad_scale first (1/world for the
 * data-parallel mean).  step = 1-based step count (bias correction). */
/* Layout (lfdm_adam_step_f32, lfdm_adam_guarded_step_f32, lfdm_grad_sumsq_f32, lfdm_optim_plan_f32): flat dense buffers; param, grad, exp_avg, exp_avg_sq, ema
 * and the plan record 16 B. */
int lfdm_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                       float grad_scale, lfdm_stream_t stream);

/* Guarded optimizer step (additive; FlatAdam's opt-in ema_decay / max_grad_norm / skip_nonfinite).  Three launches on one
 * stream replace, per step, torch.nn.utils.clip_grad_norm_(params, max_norm) (~300 small launches and a host read-back of the norm), the
 * `if not torch.isfinite(norm): skip` test a training script would write around optimizer.step(), the Adam step itself and the
 * `for e, p in zip(ema, params): e.mul_(d).add_(p, alpha=1 - d)` loop of an EMA class (video_flow_diffusion.py:116-135, never wired in by
 * the reference).  Every decision is taken on the device; nothing here synchronises.  No floating-point atomics: all results are fixed
 * functions of their inputs, so data-parallel ranks holding the same all-reduced gradient take bit-identical updates.
 *
 * The plan: LFDM_OPTIM_PLAN_BYTES of device memory, 16-byte aligned, zeroed once by the caller and then owned by these calls (the two
 * counters persist across steps; a caller restoring a checkpoint writes applied_steps itself). */
#define LFDM_OPTIM_PLAN_BYTES 64
typedef struct {
  int apply;                    /* 0: the norm was not finite and the guard is on - the update pass does nothing */
  int reserved0;
  float clip_coef;              /* min(1, max_grad_norm / (total_norm + 1e-6)); 1 when clipping is off */
  float total_norm;             /* grad_scale * sqrt(sum g^2): the norm of the AVERAGED gradient; 0 when no norm pass ran */
  float bias1;                  /* 1 - beta1^t, t = applied_steps + 1 (computed in double) */
  float bias2_sqrt;             /* sqrt(1 - beta2^t) */
  float ema_decay;              /* effective decay of step t: 0 while t <= ema_start_step (the average tracks the parameters exactly) */
  float ema_one_minus_decay;    /* 1 - decay, rounded once from double */
  int64_t applied_steps;        /* += 1 when apply */
  int64_t skipped_steps;        /* += 1 when not */
  int reserved1[4];
} lfdm_optim_plan;

/* Pass 1 (only when clipping or the guard is on): one fp32 partial sum of squares per workgroup of the launch, written to
 * partials[0 .. lfdm_grad_sumsq_ws_bytes(n) / 4).  16-byte loads, four accumulators per thread, adam_step's launch geometry
 * (min(ceil(n / 1024), 4096) workgroups of 256): each accumulator is a chain of L = ceil((n / 4) / (256 * workgroups)) (+ 1 when n % 4)
 * fused multiply-adds, followed by 8 tree levels; the relative error of the norm is at most (L + 12) * 2^-24. */
size_t lfdm_grad_sumsq_ws_bytes(int64_t n);
int lfdm_grad_sumsq_f32(const float* grad, int64_t n, float* partials, size_t partials_bytes, lfdm_stream_t stream);
/* Pass 2 (one workgroup): sums the partials in a fixed order in fp64 and writes the plan for step applied_steps + 1, then advances
 * applied_steps or skipped_steps.  n_partials = 0 (partials may be NULL): no norm pass ran - total_norm 0, clip_coef 1, apply 1; then
 * max_grad_norm must be negative and skip_nonfinite 0.  max_grad_norm < 0: clipping off.  ema_decay < 0: no average (decay 0). */
int lfdm_optim_plan_f32(const float* partials, int n_partials, void* plan, size_t plan_bytes, float grad_scale, float max_grad_norm,
                        int skip_nonfinite, float beta1, float beta2, double ema_decay, int64_t ema_start_step, lfdm_stream_t stream);
/* Pass 3: the arithmetic of the plain Adam step above with grad = g * grad_scale * clip_coef + weight_decay * p (the clip acts on the
 * averaged gradient, before weight decay - the torch call order) and, when ema is not NULL, ema = d * ema + (1 - d) * p_new in the same
 * pass; clip_coef, the bias corrections, d and apply are read from the plan in device memory.  apply == 0: param, exp_avg, exp_avg_sq
 * and ema stay bit-for-bit untouched.  grad is never written. */
int lfdm_adam_guarded_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr,
                               float beta1, float beta2, float eps, float weight_decay, float grad_scale, const void* plan,
                               lfdm_stream_t stream);

/* AntiAliasInterpolation2d (LFAE/modules/util.py:217-264; region / pixelwise-flow predictor inputs): planar
 * (N, C, H, W) -> zero-pad (pad_lo before, pad_hi after) -> depthwise k x k filter wgt (C, k, k) -> every
 * stride-th pixel: out (N, C, ceil((H+pad_lo+pad_hi-k+1)/stride), ...). */
int lfdm_depthwise_down_planar_f32(const float* x, const float* wgt, float* out, int n_img, int channels,
                                   int h, int w, int k, int pad_lo, int pad_hi, int stride,
                                   lfdm_stream_t stream);

/* Nearest x2 upsample + pad (zeros or reflect, pad in {0,1}) of CL rows, materialised for the training path of the
 * use_deconv=False Upsample (video_flow_diffusion.py:160-163: Upsample(scale 2, nearest) -> Conv3d(padding_mode)).
 * backward = 0: x (n, h, w, C) -> out (n, 2h+2pad, 2w+2pad, C);  backward = 1: x is the gradient of that output and
 * out (n, h, w, C) its adjoint (sum over the positions that read each input pixel). */
int lfdm_upsample2_pad_cl_f32(const float* x, float* out, int n_img, int h, int w, int channels, int pad,
                              int reflect, int backward, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * LFAE stage-1 training glue (ABI version 10, BatchNorm segments 11; csrc/train_lfae.hip): what connects the convolutions of
 * ReconstructionModel.forward (LFAE/modules/model.py:141-217) - replaces the MIOpen BatchNorm, MIOpen / composable_kernel depth-wise
 * convolution and ATen grid_sampler kernels the reference's nn.Modules dispatch to.
 */
#define LFDM_BN_TICKETS 1024
/* nn.BatchNorm2d in training mode (+ optional ReLU) on channels-last rows: LFAE/modules/util.py:70-150 (ResBlock2d :84-90, UpBlock2d
 * :108-112, DownBlock2d :128-133, SameBlock2d :146-150).  y = relu(((x - mean) * rstd) * gamma + beta) with the batch mean / BIASED
 * variance per channel over `rows`; running_mean / running_var (may both be NULL) are updated with `momentum` and the UNBIASED variance like
 * torch; stat receives [mean (C) | rstd (C)] for the backward.  Two launches (row-chunk reduce folded by tickets in a fixed order - the
 * result does not depend on workgroup arrival order - and apply).  tickets: LFDM_BN_TICKETS zeroed 32-bit words, left zeroed. */
/* segments (ABI 11, 1..64): x / y hold `segments` batches of `rows` rows each, one after the other; every segment is normalised with
 * its own batch statistics (stat = [segment][mean (C) | rstd (C)]), the running statistics take the segments' momentum updates in segment
 * order and dgamma / dbeta are summed over the segments - exactly `segments` calls of the module on the separate batches (the region
 * predictor on source, driving and transformed frames, model.py:157-160, :190-191), as one launch pair. */
size_t lfdm_batchnorm_train_ws_bytes(int64_t rows, int channels, int segments);
/* Layout (forward and backward): x (ldx), y (ldy), dy (lddy), dx (lddx), dx_add (ldadd): 16 B, ld % 4, C % 4 - channel slices of wider channels-last tensors; stat 16 B. */
int lfdm_batchnorm_train_fwd_cl_f32(const float* x, float* y, int64_t rows, int channels, int segments, int ldx, int ldy,
                                    const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                                    float eps, int relu, float* stat, void* ws, size_t ws_bytes, unsigned* tickets, lfdm_stream_t stream);
/* Backward of the above from the saved input x and stat: dx, dgamma (C), dbeta (C) (either may be NULL); relu = 1 masks dy by the sign of
 * the recomputed pre-activation (the same arithmetic as the forward: identical mask).  dx_add (may be NULL, row stride ldadd): a second
 * gradient of x - the identity skip of ResBlock2d (util.py:84-92) - summed into dx by the kernel. */
int lfdm_batchnorm_train_bwd_cl_f32(const float* x, const float* dy, float* dx, int64_t rows, int channels, int segments, int ldx, int lddy,
                                    int lddx, const float* dx_add, int ldadd, const float* gamma, const float* beta, const float* stat, int relu,
                                    float* dgamma, float* dbeta,
                                    void* ws, size_t ws_bytes, unsigned* tickets, lfdm_stream_t stream);

/* AntiAliasInterpolation2d (LFAE/modules/util.py:217-264) / ImagePyramide (model.py:62-82) with any element strides on both sides:
 * out[n, c, oy, ox] = scale[c] * sum_k wgt[c, ky, kx] * x[n, c, oy*stride + ky - pad_lo, ox*stride + kx - pad_lo] + bias[c] (zero
 * padding; only the kept outputs are computed; scale / bias NULL = 1 / 0 - the VGG input normalisation of model.py:52 when given);
 * channels in [channels, c_store) of the output are written as zeros (the pad channel of 4-channel rows).  _bwd: dx from dy. */
typedef struct lfdm_blur_params {
  const float* x;
  const float* wgt;      /* (channels, k, k) */
  float* out;
  const float* dy;       /* backward: gradient of out (out strides) */
  float* dx;             /* backward: gradient of x (x strides) */
  int64_t xs_n, xs_c, xs_h, xs_w, os_n, os_c, os_h, os_w;
  int n_img, channels, c_store, h, w, k, pad_lo, pad_hi, stride;
  const float* scale;
  const float* bias;
} lfdm_blur_params;
int lfdm_blur_down_fwd_f32(const lfdm_blur_params* p, lfdm_stream_t stream);
int lfdm_blur_down_bwd_f32(const lfdm_blur_params* p, lfdm_stream_t stream);

/* Backward of Generator.deform_input + apply_optical (LFAE/modules/generator.py:59-88): out = grid_sample(src, resize(flow)) *
 * resize(occ) + prev * (1 - resize(occ)) per sample n (one source per sample; maps (fh, fw) planes, element (n, y, x) at n*fsn + y*fw + x,
 * resized bilinearly to (h, w) when the sizes differ - lfdm_warp_cl_f32's forward arithmetic).  Produces
 *   dprev = dout * (1 - occ)                                     (optional),
 *   dmaps (n_img, 3, h, w) = [d flow_x, d flow_y, d occ] at OUTPUT resolution (lfdm_resize_adjoint_f32 folds them to (fh, fw)),
 *   dsrc_fix: 64-bit fixed-point accumulators (n_img*h*w, C), zero on entry, += tap weight * occ * dout * 2^k (channels-last form only),
 *             k from *amax_bits = max |dout| (lfdm_absmax_f32) so that no sum can overflow; lfdm_fix_finalize_f32 converts to float and
 *             re-zeroes.  Integer atomics commute: the gradient is identical from run to run (ATen's float atomics are not).
 * layout_cl = 1: src / dout / prev / dprev are channels-last rows with the ld_* leading dimensions, C / 4 a power of two <= 64;
 * layout_cl = 0: any element strides (ss_*, ds_*, ps_*, dps_*), few channels, src shared by n_div consecutive samples, no dsrc. */
typedef struct lfdm_warp_bwd_params {
  const float* src;
  const float* dout;
  const float* prev;       /* NULL: no blend partner (out = warped * occ) */
  float* dprev;            /* NULL: not wanted */
  long long* dsrc_fix;     /* NULL: not wanted */
  unsigned* amax_bits;
  float* dmaps;
  const float* flow_x;
  const float* flow_y;
  const float* occ;        /* NULL: occ = 1 */
  int n_img, h, w, c, fh, fw, n_div, layout_cl;
  int64_t fsn;
  int ld_src, ld_dout, ld_prev, ld_dprev;
  int64_t ss_n, ss_c, ss_h, ss_w, ds_n, ds_c, ds_h, ds_w, ps_n, ps_c, ps_h, ps_w, dps_n, dps_c, dps_h, dps_w;
} lfdm_warp_bwd_params;
/* Layout: warp_bwd, channels-last form: src (ld_src), dout (ld_dout), prev (ld_prev), dprev (ld_dprev): 16 B, ld % 4; dsrc_fix 8 B, dense; the strided form takes any
 * element strides.  absmax: x (ld): any (float4 walk when 16 B, ld % 4 and C % 4, scalar otherwise).  fix_finalize: out (ld): any; acc dense. */
int lfdm_warp_bwd_f32(const lfdm_warp_bwd_params* p, lfdm_stream_t stream);
/* *out_bits = max(*out_bits, bit pattern of max |x|) over a (rows, channels) matrix with leading dimension ld (integer max). */
int lfdm_absmax_f32(const float* x, int64_t rows, int channels, int64_t ld, unsigned* out_bits, lfdm_stream_t stream);
/* out (rows, channels; ld) = acc * 2^-k, acc re-zeroed, *amax_bits cleared by the last workgroup (ticket: one zeroed word, left zeroed);
 * count = the per-address bound the scatter used (4 * h * w). */
int lfdm_fix_finalize_f32(long long* acc, float* out, int64_t rows, int channels, int64_t ld, unsigned* amax_bits, int64_t count,
                          unsigned* ticket, lfdm_stream_t stream);
/* Adjoint of F.interpolate(mode='bilinear', align_corners=False) from (fh, fw) to (h, w) on `planes` planes (gather form, no atomics). */
int lfdm_resize_adjoint_f32(const float* dhigh, float* dlow, int planes, int h, int w, int fh, int fw, lfdm_stream_t stream);

/* F.grid_sample(x, grid, mode='bilinear', align_corners=False) with an explicit grid (n_img, ho, wo, 2) on strided tensors of few channels;
 * x is shared by n_div consecutive samples (pixelwise_flow_predictor.py:95-102 repeats the source K+1 times); pad_mode 0 = zeros, 1 =
 * reflection (Transform.transform_frame, model.py:118-122).  _bwd: dgrid (n_img, ho, wo, 2) from dout (out strides), zeros padding. */
typedef struct lfdm_grid_sample_params {
  const float* x;
  const float* grid;
  float* out;
  const float* dout;
  float* dgrid;
  int64_t xs_n, xs_c, xs_h, xs_w, os_n, os_c, os_h, os_w;
  int n_img, channels, h, w, ho, wo, n_div, pad_mode;
} lfdm_grid_sample_params;
int lfdm_grid_sample_fwd_f32(const lfdm_grid_sample_params* p, lfdm_stream_t stream);
int lfdm_grid_sample_bwd_f32(const lfdm_grid_sample_params* p, lfdm_stream_t stream);

/* Backward of lfdm_svd2x2_sym_f32 / torch.svd on symmetric positive semi-definite 2x2 matrices (region_predictor.py:16-26): ga (n, 2, 2)
 * from u (n, 2, 2), s (n, 2) and the gradients gu / gs (either may be NULL) - torch's svd_backward with V = U, closed form. */
int lfdm_svd2x2_sym_bwd_f32(const float* u, const float* s, const float* gu, const float* gs, float* ga, int64_t n, lfdm_stream_t stream);

/* 2x2 pooling family on channels-last rows; (h, w) = the FINE resolution (even).  mode 0: average (DownBlock2d, util.py:133) | 1: sum
 * (backward of nearest x2) | 2: nearest x2 (UpBlock2d, util.py:109) | 3: nearest x2 * 0.25 (backward of the average) | 4: max (VGG-19's
 * MaxPool2d(2, 2), model.py:19-47) | 5: backward of the max (aux = dy at the coarse resolution, x = the forward's input; the gradient goes
 * to the first maximum of the window in row-major order, like ATen).  Modes 0 / 1 / 4 read fine and write coarse rows, 2 / 3 / 5 the reverse. */
int lfdm_pool2_cl_f32(const float* x, const float* aux, float* out, int n_img, int h, int w, int channels, int mode, lfdm_stream_t stream);
/* out = y > 0 ? dy : 0 over n floats: backward of a ReLU fused into the producing convolution (lfdm_conv_params.act = 1; VGG-19, model.py:19-59). */
int lfdm_relu_bwd_f32(const float* y, const float* dy, float* out, int64_t n, lfdm_stream_t stream);
/* *out = weight * mean |x - y| (the perceptual loss terms, model.py:189-195), partials folded in a fixed order by the last workgroup
 * (ws: 8 KB, 8-byte aligned; ticket: one zeroed word, left zeroed);  _bwd: dx = sign(x - y) * (*gout) * weight / n. */
int lfdm_l1_mean_fwd_f32(const float* x, const float* y, int64_t n, float weight, float* out, void* ws, size_t ws_bytes, unsigned* ticket,
                         lfdm_stream_t stream);
int lfdm_l1_mean_bwd_f32(const float* x, const float* y, int64_t n, float weight, const float* gout, float* dx, lfdm_stream_t stream);

/* The diffusion edge of the DM training step with known frames / elements held clean (ABI 14: one mask struct, one loss params struct;
 * DESIGN.md 4.12, 4.14, csrc/train_diffusion.hip).  Samples are dense rows of n floats (n % 4 == 0, n < 2^31); t: (B) int64 ON THE DEVICE,
 * clamped to [0, t_len) by the kernels; the tables are the registered fp32 buffers of t_len entries, read on the device.  Mask forms, as in
 * the known operands of the sampler step: none (both masks NULL, frames = frame_elems = 0) | frame_mask: (B, frames) bytes, non-zero = frame
 * (i / frame_elems) % frames of sample b is known, n a multiple of frames * frame_elems, frame_elems % 4 == 0 | elem_mask: (B, n) bytes,
 * 4-byte aligned, frames = frame_elems = 0.  No floating-point atomics, fixed summation order: two runs give the same bits.
 * Refusals (LFDM_EINVAL, nothing is enqueued): a null operand, n % 4 != 0, both masks, a frame split without frame_mask or one that does
 * not divide n or whose frames are no multiple of 4 elements, t_len <= 0, loss_type outside { LFDM_LOSS_L1, LFDM_LOSS_L2 }, an objective
 * outside the three or one whose operands are missing (refused with the list of what each needs).
 *   qsample:  x_noisy = known ? x_start : a_tab[t_b] * x_start + s_tab[t_b] * noise  (two fp32 products and one fp32 sum, each rounded on
 *             its own: the bits of q_sample's expression; a known element is the bits of x_start).  mask NULL = no mask.
 * The loss, per training objective and with a per-timestep weight.  `out`: the denoiser's output; (a, s, r, m, w) = (a_tab, .. w_tab)[t_b]:
 *   LFDM_OBJ_NOISE  target = noise                      pred_x0 = r * x_noisy - m * out   (without w_tab: the masked loss of 4.12)
 *   LFDM_OBJ_X0     target = x_start                    pred_x0 = out (its bits)
 *   LFDM_OBJ_V      target = a * noise - s * x_start    pred_x0 = a * x_noisy - s * out
 * every expression two fp32 products and one fp32 difference, each rounded on its own; the target is never stored.  Operands the objective
 * does not use may be NULL and are never read: x_start, a_tab, s_tab for LFDM_OBJ_NOISE; noise and all four tables for LFDM_OBJ_X0; r_tab,
 * m_tab for LFDM_OBJ_V and in the backward; in the backward also t and t_len unless it reads a table (LFDM_OBJ_V, or w_tab).  w_tab NULL = 1.
 *   fwd: S_b = sum over the unknown elements of |target - out| (LFDM_LOSS_L2: squared), N_b = their number;  inv_count[b] = 1 / max(N_b, 1);
 *        sample_loss[b] = S_b / max(N_b, 1) (unweighted);  *loss = (1 / B) sum_b w * S_b / max(N_b, 1), the weight applied in double in the
 *        last workgroup's fold;  in the same pass pred_x0 as above, x_noisy where known.
 *        ws: lfdm_masked_loss_ws_bytes, 8-byte aligned (too small: LFDM_EWORKSPACE); ticket: one zeroed word, left zeroed (one stream at a time)
 *   bwd: dout = c_b * d|target - out| / d out = -sign(target - out) c_b (LFDM_LOSS_L2: 2 (out - target) c_b), c_b = (((*gout) *
 *        inv_count[b]) * w) / B in fp32 in that order (w_tab NULL: no product); known: 0.f */
#define LFDM_LOSS_L1 0
#define LFDM_LOSS_L2 1
#define LFDM_OBJ_NOISE 0
#define LFDM_OBJ_X0 1
#define LFDM_OBJ_V 2
typedef struct lfdm_train_mask {
  const unsigned char *frame_mask, *elem_mask;
  int frames;
  int64_t frame_elems;
} lfdm_train_mask;
/* Both directions read objective .. n and inv_count (the forward writes it); an entry ignores the other direction's fields. */
typedef struct lfdm_train_loss_params {
  int objective, loss_type;
  const float *x_start, *noise, *out, *x_noisy;         /* x_noisy: forward only */
  const int64_t* t;
  const float *a_tab, *s_tab, *r_tab, *m_tab, *w_tab;   /* r_tab, m_tab: forward only */
  int t_len;
  lfdm_train_mask mask;
  int batch;
  int64_t n;
  float *loss, *inv_count, *sample_loss, *pred_x0;      /* forward outputs; inv_count is the backward's input */
  const float* gout;                                    /* backward only, as dout */
  float* dout;
  void* ws;                                             /* forward only, as ws_bytes and ticket */
  size_t ws_bytes;
  unsigned* ticket;
} lfdm_train_loss_params;
/* Layout: x_start, noise, x_noisy dense (B, n), 16 B; t dense (B) int64; a_tab, s_tab dense (t_len); masks dense.  x_noisy must not alias an input. */
int lfdm_train_qsample_f32(const float* x_start, const float* noise, const int64_t* t, const float* a_tab, const float* s_tab, int t_len,
                           const lfdm_train_mask* mask, float* x_noisy, int batch, int64_t n, lfdm_stream_t stream);
size_t lfdm_masked_loss_ws_bytes(int batch, int64_t n);
/* Layout: x_start, noise, out, x_noisy, pred_x0 dense (B, n), 16 B; t dense (B) int64; the tables dense (t_len); masks dense; loss 1 float,
 * inv_count, sample_loss (B) floats.  pred_x0 must not alias an input. */
int lfdm_objective_loss_fwd_f32(const lfdm_train_loss_params* p, lfdm_stream_t stream);
/* Layout: x_start, noise, out, dout dense (B, n), 16 B; t dense (B) int64; the tables dense (t_len); masks dense; inv_count (B) floats and
 * gout 1 float on the device.  dout must not alias an input. */
int lfdm_objective_loss_bwd_f32(const lfdm_train_loss_params* p, lfdm_stream_t stream);

/* Progressive distillation (Salimans & Ho 2022; additive, ABI version unchanged; DESIGN.md 4.16, csrc/distill.hip): the frozen teacher's
 * DDIM step with a coefficient row PER SAMPLE, and the target one student step has to reach.  Samples are dense rows of n floats (n % 4 == 0,
 * 0 < n < 2^24, batch <= 65 535); coef: (rows, 6) floats {c_x, c_eps, k_x0, k_eps, k_x, -} - a step table of the sampler, column 5 (the
 * noise scale) is never read: eta = 0; row: (B) int64 ON THE DEVICE, clamped to [0, rows) by the kernels.  Every product and sum is rounded
 * on its own; a coefficient that is exactly 0 skips its product, and an operand all of whose coefficients are 0 is never loaded (it may
 * hold NaN, but must be a valid pointer).  No atomics, no workspace, one owner per output element: two runs give the same bits.
 *   x0:    x0 = c_x x - c_eps out  (the bits of the eager fp32 expression; rows {0, -1}: the bits of out) - the operand of
 *          lfdm_abs_quantile_f32 when the model thresholds dynamically
 *   step:  x0 as above (recomputed);  s = thr ? max(thr[b], 1) : 1  (thr: (B) floats, NULL = the static clamp to [-1, 1]);
 *          m = min(max(x0, -s), s) / s;  v = k_x0 m [+ k_eps out] [+ k_x x] -> x_next (may be x itself; NULL in target mode: v is not stored)
 *          target mode (x_ref, tcoef, trow, x_target, eps_target: all or none; tcoef: (trows, 4) floats {q0, q1, q2, q3}, trow: (B) int64 on
 *          the device, clamped to [0, trows)):  xt = q0 v + q1 x_ref -> x_target;  et = q2 x_ref + q3 xt -> eps_target
 * Refusals (LFDM_EINVAL, nothing is enqueued): a null or misaligned operand, bad batch / n / rows, a partial set of target operands, trows
 * that does not go with them, no output at all, x_ref aliasing an output, two outputs aliasing each other, an output other than x_next = x
 * aliasing an input. */
/* Layout: x, out, x0 dense (B, n), 16 B; coef dense (rows, 6); row dense (B) int64.  x0 must not alias out. */
int lfdm_distill_x0_f32(const float* x, const float* out, const float* coef, const int64_t* row, int rows, float* x0, int batch, int64_t n,
                        lfdm_stream_t stream);
/* Layout: x, out, x_next, x_ref, x_target, eps_target dense (B, n), 16 B; coef dense (rows, 6), tcoef dense (trows, 4); row, trow dense (B)
 * int64; thr dense (B).  x_next may be x; no other output aliases an operand or another output. */
int lfdm_distill_step_f32(const float* x, const float* out, const float* coef, const int64_t* row, int rows, const float* thr, float* x_next,
                          const float* x_ref, const float* tcoef, const int64_t* trow, int trows, float* x_target, float* eps_target,
                          int batch, int64_t n, lfdm_stream_t stream);

/* im2col of channels-last rows with few channels (channels % 4 == 0, <= 16; stride 1, zero padding): out (n_img*hq*wq, k*k*channels),
 * column tap * channels + ch.  Lets the weight gradient of the generator's 7x7 RGB convolutions (LFAE/modules/generator.py:37,56: 3 -> 64
 * and 64 -> 3 channels) run as ONE 1x1 weight-gradient GEMM instead of 49 per-tap GEMMs that pad 4 channels to a 64-wide tile. */
/* Layout: x (ldx): 16 B, ldx % 4, C % 4; out dense, 16 B. */
int lfdm_im2col_cl_f32(const float* x, float* out, int n_img, int h, int w, int channels, int ldx, int k, int pad, lfdm_stream_t stream);

/* lfdm_pack_wino_weight_f32 for MANY filters in one launch: `jobs` is a table of n_jobs records IN DEVICE MEMORY, sorted by block0 = the first
 * workgroup of the job (job i covers ceil(K_i / 4 * coutp_i / 256) workgroups - a thread packs four reduction channels; total_blocks = their sum).  Same arguments per record as the single
 * call.  Training re-packs every 3x3 filter after each optimizer step (video_flow_diffusion_model.py:181-188; LFAE/train.py:96-104). */
typedef struct lfdm_pack_wino_job {
  const float* w;
  float* out;
  int ld_o, cout, cin, coutp, dgrad, block0;
} lfdm_pack_wino_job;
int lfdm_pack_wino_weights_multi_f32(const lfdm_pack_wino_job* jobs, int n_jobs, int total_blocks, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * uint8 preview strips of a sampled video (additive under ABI 12).  Replaces, on the device, what the reference's demo
 * scripts do per frame on the host between sample_one_video and imageio.mimsave: misc.py:66-73 flow2fig (flow_vis.flow_to_color),
 * misc.py:76-80 conf2fig, demo/demo_mug.py:26-32 sample_img and :124-143 the panel strip.  misc.py:44-63 grid2fig (a matplotlib line
 * drawing) is not rendered here.
 *
 * lfdm_flow_color_u8: out (batch * frames, s, s, 3) uint8 = flow_to_color(grid - identity) per frame.  grid: planar (batch, 2, frames,
 * s, s), channel 0 = x, contiguous within a batch element, batch elements batch_stride floats apart (so the first two channels of a
 * (batch, 3, frames, s, s) latent can be passed as they are).  ident: s floats, torch.linspace(-1, 1, s) made by the caller - the
 * subtraction is fp32 and must see the host's values.  Everything after the subtraction is fp64 in numpy's operation order; the maximum
 * radius is taken per frame (wave shuffles + LDS, no atomics).  One workgroup per frame.  s % 4 == 0; out 16-byte aligned. */
/* Layout: grid: any, batch item b at grid + b*batch_stride (>= 2*frames*s*s floats: the first two channels of a 3-channel latent are read in place); out dense, 16 B. */
int lfdm_flow_color_u8(const float* grid, int64_t batch_stride, const float* ident, unsigned char* out, int batch, int frames, int s,
                       lfdm_stream_t stream);
/* lfdm_render_strip_u8: out (batch, frames, S, n_panels * S, 3) uint8 RGB, or with indexed != 0 (batch, frames, S, n_panels * S) uint8
 * indices into the fixed 6x6x6 palette (index = 36 r + 6 g + b, level k = 51 k) under an 8x8 ordered dither:
 *   level = (c * 320 + 255 * bayer[y & 7][x & 7] + 127) / 16320   (integer division; c the channel value 0 .. 255; x the strip column).
 * panels: HOST array of n_panels (1 .. 8) LFDM_PANEL_* codes, left to right; only the operands of the listed panels are read, the others
 * may be NULL.  source (batch, 3, S, S), out_vid / warped_vid (batch, 3, frames, S, S) planar fp32: byte = trunc(clamp(float(double(x) +
 * mean_over_255[c]), 0, 1) * 255.f) (mean_over_255: HOST array of 3 doubles, mean / 255.0); flow_color: lfdm_flow_color_u8's output,
 * resized s -> S bilinearly (align_corners = false, round half to even); conf (batch, 1, frames, s, s): nearest, trunc(conf * 255.f) on
 * three channels.  NaN -> 0.  S == 4 * s, s % 4 == 0; out and the fp32 image operands 16-byte aligned.  Every store is a whole 16-byte
 * segment. */
#define LFDM_PANEL_SOURCE 0
#define LFDM_PANEL_OUT 1
#define LFDM_PANEL_WARPED 2
#define LFDM_PANEL_FLOW 3
#define LFDM_PANEL_CONF 4
int lfdm_render_strip_u8(const float* source, const float* out_vid, const float* warped_vid, const unsigned char* flow_color,
                         const float* conf, const double* mean_over_255, const int* panels, int n_panels, int indexed,
                         unsigned char* out, int batch, int frames, int S, int s, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Paired, full-reference metrics of two videos (additive under ABI 12): per frame and on the device what an evaluation
 * script would otherwise copy to the host for (LFAE/test_flowautoenc_*.py: the L1 behind out_loss / warp_loss).
 *
 * lfdm_video_metrics: a, b planar fp32 (batch, channels, frames, h, w), contiguous; out (batch, frames, 3) float64 = [l1, mse, ssim] of
 * every frame, each the mean over the frame's channels.  1 <= channels <= 4; h, w >= 11, any value.  The value domain:
 *   LFDM_METRIC_RAW    the operands as they are;
 *   LFDM_METRIC_UNIT   v = clamp(float(double(x) + mean_over_255[c]), 0, 1) (io_compat.sample_img before its scaling);
 *   LFDM_METRIC_UINT8  trunc(float(v * 255.f)) / 255: the bytes lfdm_render_strip_u8 writes, NaN -> 0.
 * mean_over_255: HOST array of `channels` doubles, mean / 255.0 (may be NULL for RAW).  l1 = mean |a - b| and mse = mean (a - b)^2 over the
 * whole frame.  ssim: Wang et al. 2004 - separable 11-tap Gaussian window, sigma 1.5, weights normalised to sum 1 per axis; variances and
 * covariance E[xy] - E[x] E[y]; C1 = 0.01^2, C2 = 0.03^2 (data range 1 in EVERY domain, RAW included); the map on the valid interior
 * (h - 10) x (w - 10) only, averaged.  Operands are converted exactly to fp64 and all arithmetic is fp64.  No atomics: per-tile sums go
 * to ws (lfdm_video_metrics_ws_bytes bytes, 8-byte aligned, need not be zeroed) and a second launch adds them in tile order, so a
 * frame's three numbers are bit-identical from run to run and do not depend on batch, frames or the frame's place among them. */
#define LFDM_METRIC_RAW 0
#define LFDM_METRIC_UNIT 1
#define LFDM_METRIC_UINT8 2
#define LFDM_METRIC_MAX_CHANNELS 4
size_t lfdm_video_metrics_ws_bytes(int batch, int channels, int frames, int h, int w);
int lfdm_video_metrics(const float* a, const float* b, const double* mean_over_255, int domain, double* out, int batch, int channels,
                       int frames, int h, int w, void* ws, size_t ws_bytes, lfdm_stream_t stream);
/* lfdm_flow_metrics: out (batch, frames, 2) float64 = [mean end-point error sqrt(dx^2 + dy^2) of two sampling grids in their normalised
 * units, mean |conf_a - conf_b|] per latent frame.  grid_a / grid_b: planar (batch, 2, frames, s, s), channel 0 = x, batch elements
 * stride_a / stride_b floats apart (as lfdm_flow_color_u8: the first two channels of a (batch, 3, frames, s, s) latent pass as they
 * are); conf_a / conf_b (batch, 1, frames, s, s) contiguous, both or neither - without them the second number is 0.  fp64, no atomics,
 * one workgroup per frame in a fixed order. */
/* Layout: grid_a (stride_a), grid_b (stride_b): any, each with its own batch stride; confidences dense; out 8 B. */
int lfdm_flow_metrics(const float* grid_a, int64_t stride_a, const float* grid_b, int64_t stride_b, const float* conf_a,
                      const float* conf_b, double* out, int batch, int frames, int s, lfdm_stream_t stream);
/* out[i] = 10 log10(1 / mse[i]) over n doubles (data range 1), +inf where mse[i] == 0. */
int lfdm_psnr_f64(const double* mse, double* out, int64_t n, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training batches from a packed uint8 frame store (additive under ABI 12): on the device what the host loader does per
 * frame between decode and the batch tensor - colour jitter, area shrink, mean subtraction, / 255, transpose.
 *
 * lfdm_video_prep_u8: out (batch, 3, frames, H, H) planar fp32, H = image_size, from store (store_frames, S, S, 3) uint8, S = store_size.
 * frame_index: DEVICE (batch, frames) int32 rows of store - a gather, repeats and any order allowed; every entry must lie in
 * 0 .. store_frames - 1 and THE CALLER CHECKS THAT (the entry point cannot read device memory).  S == k * H with k in {1, 2, 4};
 * S % 4 == 0 and H % 4 == 0; store 4-byte, out 16-byte aligned.  mean: HOST array of 3 floats.
 *   jitter == 0: out = fl32(fl32(avg - mean[c]) / 255.f), avg = the k x k byte sum / (k * k) (exact); params, hue_shift, valid and ws
 *                are not read and may be NULL.
 *   jitter != 0: every source pixel first goes through the colour jitter below with the factors of its batch element - params DEVICE
 *                (batch, 3) fp32 = (brightness, contrast, saturation), hue_shift DEVICE (batch) int32 (added to the 8-bit hue, mod 256).
 *                valid: DEVICE (batch, 4) int32 = (y0, x0, h, w), the part of a stored frame that is picture (the rest is the zero
 *                padding of a non-square video): jitter and the contrast mean see the picture only, padding stays 0.  NULL = all of it.
 *                Like frame_index it is device memory the entry point cannot read: THE CALLER CHECKS that every row has y0, x0 >= 0,
 *                h, w >= 1 (h * w == 0 divides by zero in the stats launch), y0 + h <= S and x0 + w <= S (a rectangle that leaves the
 *                frame silently changes n), and that params holds finite numbers (a NaN or inf factor reaches a float -> int cast).
 * Jitter, per pixel on bytes, in this order (blend(d, x, a) = trunc(fl32(d) + a * fl32(x - d)) in fp32 without fma, clamped to 0 .. 255
 * when a is outside [0, 1]; L = (19595 r + 38470 g + 7471 b + 0x8000) >> 16):
 *   brightness blend(0, x, bf); contrast blend(m, x, cf), m = (2 sum + n) / (2 n) over the frame's n picture pixels' L after brightness
 *   (integer); saturation blend(L, x, sf); RGB -> 8-bit HSV, hue + hue_shift, HSV -> RGB (fp32 / fp64 mix spelled out in DESIGN.md 4.7).
 * Two launches: with jitter, one workgroup per (batch, frame) writes m to ws (integer sums: wave shuffles, then LDS; no atomics); then
 * one thread per 4 adjacent output pixels.  launches: LFDM_PREP_STATS | LFDM_PREP_MAIN normally; one bit alone runs that launch alone
 * (measurement; MAIN alone with jitter reads the m a STATS run left in ws).  ws: lfdm_video_prep_ws_bytes bytes, 4-byte aligned. */
#define LFDM_PREP_STATS 1
#define LFDM_PREP_MAIN 2
size_t lfdm_video_prep_ws_bytes(int batch, int frames);
int lfdm_video_prep_u8(const unsigned char* store, int64_t store_frames, const int* frame_index, const float* params,
                       const int* hue_shift, const int* valid, const float* mean, float* out, int batch, int frames, int store_size,
                       int image_size, int jitter, int launches, void* ws, size_t ws_bytes, lfdm_stream_t stream);
/* lfdm_frame_pairs_prep_u8 (additive under ABI 12): the same for LFAE stage-1 training pairs - what lfae_train.FramePairs makes of two
 * frames of one video.  pair_index: DEVICE (batch, 2) int32 rows of store = (source, driving), checked BY THE CALLER like frame_index
 * (the two may be equal, in any order).  source, driving: (batch, 3, H, H) planar fp32 each, frame t of item b goes to output t:
 * fl32(avg / 255.f) - no mean.  params, hue_shift, valid as above: one jitter per pair, the contrast grey level m per frame (the stats
 * launch above with two frames per item; ws: lfdm_video_prep_ws_bytes(batch, 2) bytes).  flip: DEVICE (batch) int32, never NULL; where
 * flip[b] != 0 both frames of item b are mirrored left to right AFTER shrink and padding: out[y][x] = shrunk[y][H - 1 - x].  valid
 * stays in unflipped store coordinates; the padding moves with the picture.  The thread for output pixels 4 g .. 4 g + 3 computes
 * pixels H - 4 - 4 g .. H - 1 - 4 g exactly as without a flip and stores them in reversed order: whole dword loads and one 16-byte
 * store per channel plane either way, no atomics, no LDS beyond the stats launch's. */
/* Layout: store, pair_index, params, hue_shift, valid, flip dense; source, driving dense (batch, 3, H, H), 16 B each. */
int lfdm_frame_pairs_prep_u8(const unsigned char* store, int64_t store_frames, const int* pair_index, const float* params,
                             const int* hue_shift, const int* valid, const int* flip, float* source, float* driving, int batch,
                             int store_size, int image_size, int jitter, void* ws, size_t ws_bytes, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Temporal resampling of a sampled flow latent (additive under ABI 12): frames at other instants than the sampled ones -
 * a higher frame rate, slow motion, reverse, ping-pong - from the latent, without sampling more frames.  Every frame's warp field refers
 * to the same source image, so a field between two frames is a weighted mix of its neighbours.
 *
 * lfdm_latent_resample_f32: out (batch, channels, out_frames, h, w) from latent (batch, channels, frames, h, w), planar fp32.  Output
 * frame j is taken at time idx[j] + frac[j]: idx DEVICE (out_frames) int32 in 0 .. frames - 1, frac DEVICE (out_frames) fp32 in [0, 1),
 * any order, repeats allowed.  The tables are device memory the entry point cannot read: THE CALLER CHECKS them (and that frac == 0 where
 * idx == frames - 1); the kernel clamps idx and its neighbours into 0 .. frames - 1, so a bad table never reads outside latent.
 *   frac[j] == 0           frame idx[j] bit for bit, in both modes: selected, not multiplied - no other frame is read, so a NaN or an
 *                          infinity elsewhere cannot reach it, and frames == 1 is legal.  Not clamped.
 *   LFDM_RESAMPLE_LINEAR   x[i] + a * (x[i+1] - x[i]), a = frac[j]: three fp32 roundings, no fma.
 *   LFDM_RESAMPLE_CUBIC    Catmull-Rom over x0 .. x3 = frames max(i-1, 0), i, i+1, min(i+2, frames-1) (the end frames duplicated):
 *                          ((w0 x0 + w1 x1) + w2 x2) + w3 x3 in fp32 without fma, w0 = ((2 - a) a - 1) a / 2, w1 = ((3a - 5) a^2 + 2) / 2,
 *                          w2 = ((4 - 3a) a + 1) a / 2, w3 = (a - 1) a^2 / 2, each evaluated in fp64 and rounded once to fp32.
 * clamp_from: interpolated values of channels >= clamp_from are clamped to [-1, 1] (cubic weights overshoot, the occlusion channel
 * lives in [-1, 1]); clamp_from >= channels: no clamp.
 * The maps form (conf != NULL; channels == 3): the launch also does what FlowDiffusion._maps does behind it - conf (batch, 1,
 * out_frames, h, w) = (ch2 + 1) * 0.5 (two fp32 operations), and with ident_x (w floats) / ident_y (h floats) - DEVICE,
 * torch.linspace(-1, 1, .) made by the caller, both or neither - out channel 0 += ident_x[x], channel 1 += ident_y[y] (one fp32 add:
 * the residual-flow case).  At frac == 0 that is _maps of the selected frame bit for bit.
 * h * w % 4 == 0.  One thread per 4 adjacent values: 16-byte loads and stores; grid (plane chunks, out_frames, batch), out_frames and
 * batch <= 65535; no atomics, nothing depends on launch order: results are bit-identical from run to run. */
/* Layout: all operands dense; latent, out, conf 16 B; out / conf may not alias latent or each other. */
#define LFDM_RESAMPLE_LINEAR 0
#define LFDM_RESAMPLE_CUBIC 1
int lfdm_latent_resample_f32(const float* latent, const int* idx, const float* frac, const float* ident_x, const float* ident_y,
                             float* out, float* conf, int batch, int channels, int frames, int out_frames, int h, int w, int mode,
                             int clamp_from, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training latents from a flow-latent store (additive under ABI 13): the frozen LFAE's raw outputs of every frame of a
 * data set, computed once, as a flat (store_frames, 3, h, w) array - planes: sampling grid x, grid y, occlusion map - of fp32
 * (LFDM_LATENT_F32) or fp16 (LFDM_LATENT_F16) values.
 *
 * lfdm_latent_gather_f32: out (batch, 3, frames, h, w) planar fp32; out[b, :, t] is made from store[frame_index[b, t]] by what
 * FlowDiffusion._latent_of does to the LFAE's outputs.  An fp16 value is converted to fp32 first (exact).
 *   channels 0, 1   with ident_x (w floats) and ident_y (h floats) - DEVICE, torch.linspace(-1, 1, .) made by the caller - channel 0 is
 *                   v - ident_x[x] and channel 1 is v - ident_y[y], one fp32 subtraction each: the residual-flow case.  Both NULL: a copy.
 *                   One NULL and one not is refused.
 *   channel 2       occ * 2 - 1 as two fp32 operations.  occ * 2 is exact in binary floating point, so a contracted (fused) form rounds
 *                   the same value once all the same: the result does not depend on contraction.
 * frame_index: DEVICE (batch, frames) int32 rows of store - a gather, repeats and any order allowed.  It is device memory the entry
 * point cannot read: THE CALLER CHECKS that every entry lies in 0 .. store_frames - 1; the kernel clamps the row into that range, so a
 * bad table reads a wrong frame, never outside store.  All store addressing is 64-bit (a store of 349 526 fp32 frames of 32 x 32
 * passes 4 GiB).
 * h * w % 4 == 0.  One thread per 4 adjacent values of one plane: one 16-byte (fp32) or 8-byte (fp16) load and one 16-byte store; grid
 * (chunks of the 3 * h * w / 4 quads, frames, batch), frames and batch <= 65535; the row number is read once per workgroup; no atomics,
 * no LDS, nothing depends on launch order: results are bit-identical from run to run.
 * Refusals (LFDM_EINVAL, nothing is enqueued or written): a null or misaligned store / frame_index / out, a store_dtype that is neither
 * code, h * w % 4 != 0, one identity table without the other, store_frames < 1, batch / frames / h / w < 1 or a grid limit exceeded. */
/* Layout: all operands dense; store, out 16 B; frame_index, ident_x, ident_y 4 B. */
#define LFDM_LATENT_F32 0
#define LFDM_LATENT_F16 1
int lfdm_latent_gather_f32(const void* store, int store_dtype, int64_t store_frames, const int* frame_index, const float* ident_x,
                           const float* ident_y, float* out, int batch, int frames, int h, int w, lfdm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Joint sampling of a long video through overlapping windows (additive under ABI 13): one latent x of total_frames
 * frames is cut into `windows` windows of `frames` frames that go through the denoiser as one batch, and the window outputs are folded
 * back onto the global time line.  Planar fp32; frame_elems = the floats of one frame of one channel (S * S).  Window rows are ordered
 * b * windows + w.
 *
 * lfdm_window_gather_f32: xw[b * windows + w, c, t, :] = x[b, c, starts[w] + t, :] - a copy.  x (batch, channels, total_frames,
 * frame_elems), xw (batch * windows, channels, frames, frame_elems).  starts: DEVICE (windows) int32, the table the kernel reads (a captured
 * graph binds its address); starts_host: HOST (windows) int32, the caller's copy of the same table, which the entry point checks - every
 * start in [0, total_frames - frames].  The kernel clamps what it reads into that range, so a device table that differs from the host
 * copy reads other frames, never outside x.
 *
 * lfdm_window_fold_f32: out[b, c, f, :] = sum over j < count[f] of wgt[f, j] * ew[b * windows + win[f, j], c, loc[f, j], :], taken in
 * ascending j as ((w0 e0 + w1 e1) + w2 e2) + ...: one fp32 product and one fp32 addition per contributor, no fma.  A frame with ONE
 * contributor of weight 1.0f is that window's value bit for bit, and no other window is read for it (a NaN elsewhere cannot reach it).
 * ew (batch * windows, channels, frames, frame_elems), out (batch, channels, total_frames, frame_elems).  The contributor table is DEVICE
 * memory the caller prepares: count (total_frames) int32, win / loc (total_frames, LFDM_FOLD_MAX_CONTRIB) int32 - window number and frame
 * inside it -, wgt (total_frames, LFDM_FOLD_MAX_CONTRIB) fp32; slots j >= count[f] are not read.  count_host: HOST (total_frames) int32, the
 * caller's copy of count, which the entry point checks - every count in 1 .. LFDM_FOLD_MAX_CONTRIB.  THE CALLER CHECKS win and loc; the
 * kernel clamps them (and count) into range, so a bad table reads a wrong frame, never outside ew.
 *
 * Both: 16-byte loads and stores where frame_elems % 4 == 0 and both float operands are 16-byte aligned, else an element path with the
 * same values in the same order.  256-thread workgroups, one item (4 floats or 1) per thread and trip, min(ceil(items / 256), 1024)
 * workgroups in a grid-stride loop: the grid depends on the shapes only.  No atomics, no LDS, no workspace, nothing depends on launch
 * order: results are bit-identical from run to run.  Refusals (LFDM_EINVAL, nothing is enqueued or written): a null operand, a
 * non-positive size, frames > total_frames, an operand of 2^40 floats or more, out / xw overlapping the input, a start outside
 * [0, total_frames - frames], a count of 0 or above LFDM_FOLD_MAX_CONTRIB. */
#define LFDM_FOLD_MAX_CONTRIB 8
/* Layout: all operands dense; x, xw 4 B (16 B for the wide path); starts 4 B; starts_host is host memory; xw may not alias x. */
int lfdm_window_gather_f32(const float* x, const int* starts, const int* starts_host, float* xw, int batch, int windows, int channels,
                           int total_frames, int frames, int64_t frame_elems, lfdm_stream_t stream);
/* Layout: all operands dense; ew, out 4 B (16 B for the wide path); count, win, loc, wgt 4 B; count_host is host memory; out may not alias ew. */
int lfdm_window_fold_f32(const float* ew, const int* count, const int* win, const int* loc, const float* wgt, const int* count_host,
                         float* out, int batch, int windows, int channels, int total_frames, int frames, int64_t frame_elems,
                         lfdm_stream_t stream);

/* Box calibration, not on the product path (bench.py prints it beside every timing; ABI version 7): `blocks` workgroups of four
 * wavefronts run `iters` x 4 independent v_mfma_f32_32x32x2_f32 (2 * 32 * 32 * 2 FLOP each, pseudo-random operands) and
 * record, per workgroup b, out[2b] = shader cycles and out[2b+1] = 100 MHz real-time ticks of the loop: effective clock (MHz) =
 * 100 * out[2b] / out[2b+1]; the caller times the launch for the TFLOP/s.  out holds 2 * blocks + 256 floats. */
int lfdm_calib_mfma_f32(float* out, int blocks, int iters, lfdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LFDM_HIP_H */
