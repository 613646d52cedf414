/*
 * mquant_hip.h -- C ABI of the MI355X (gfx950) W4A8 static-quant hot path.
 *
 * This is the drop-in boundary.  The reference (StiphyJay/MQuant) has no native
 * code of its own: its hot path is Python calling torch ops plus ONE third-party
 * CUDA extension (fast_hadamard_transform).  Each entry point below replaces the
 * chain of reference calls cited next to it (paths relative to the reference
 * tree); INTEGRATION.md shows the ctypes binding a maintainer adds on the
 * reference side.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every pointer is a DEVICE pointer unless its name ends in _host.
 *   - stream is a hipStream_t passed as void* (NULL = default stream); all work is
 *     stream-ordered, nothing synchronises, nothing allocates.  Re-entrant: the entry points
 *     keep no mutable process state except (i) a per-device cache of kernel attributes behind
 *     a mutex and (ii) the TEST-ONLY overrides mq_gemm_debug_force / mq_hadamard_debug_threads, which are
 *     thread-local.  Nothing process-wide changes numerics: the non-default fast Hadamard stage is a flag of
 *     the call (MQ_HAD_FAST).
 *   - return value: 0 on success; >0 a hipError_t; <0 an argument error
 *     (MQ_EINVAL...).  mq_last_error() returns a thread-local message.
 *   - dtype codes: MQ_F16 / MQ_BF16 / MQ_F32 for activations and outputs.
 *   - bit-exactness contract: integer outputs (int8 levels, int32 accumulators,
 *     packed nibbles) equal oracle/mq_oracle.c bit for bit; fp outputs are
 *     computed with the same single-rounded fp32 operations as the oracle.
 */
#ifndef MQUANT_HIP_H
#define MQUANT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MQ_F16 0
#define MQ_BF16 1
#define MQ_F32 2
#define MQ_F64 3   /* mq_rotate_f64 only */

#define MQ_OK 0
#define MQ_EINVAL (-1)      /* bad argument (shape / alignment / dtype)          */
#define MQ_EUNSUPPORTED (-2) /* valid request this build does not implement       */

/* Layout of the int8 activation matrix handed from the quantizers to the GEMM.  Every entry point
 * that takes (int8 matrix, K_pad, leading dimension) accepts either
 *   ld >= K_pad      row-major [M, K_pad], ld bytes per row; or
 *   ld == MQ_LD_TILED  the TILED layout: [ceil(M/16)][K_pad/64] pieces of 1 KiB; inside a piece the
 *                    16-byte chunk holding k = 64 kt + 16 c .. +15 of row 16 mt + r sits at byte
 *                    (16 c + r) * 16, i.e. byte offset of element (m, k) =
 *                      ((m/16) * (K_pad/64) + k/64) * 1024 + (((k/16)%4) * 16 + m%16) * 16 + k%16.
 *                    K_pad % 64 == 0; the buffer holds ceil16(M) * K_pad bytes (rows >= M are never
 *                    read into a result).  One piece is one MFMA operand fragment in lane order, so
 *                    the GEMM fetches it with a single contiguous 1 KiB LDS-DMA: a CU gathers rows
 *                    of a row-major matrix at ~14.5 B/clk but streams contiguous KiB at 40-50 B/clk
 *                    (DESIGN.md 4.1). */
#define MQ_LD_TILED 0L

/* Geometry of the pre-tiled weight image consumed by mq_gemm_w4a8. */
#define MQ_W_TILE_N 16   /* output channels per MFMA fragment                     */
#define MQ_W_TILE_K 128  /* reduction elements per fragment pair (2 x K=64 MFMAs) */

int mq_version(void);
const char *mq_last_error(void);

/* Name and compute-unit count of the current device (host strings/ints). */
int mq_device_info(char *name_host, size_t name_len, int *cu_count_host);

/* ---------------------------------------------------------------------------
 * Static activation quantizer: fp -> int8 levels.
 * Replaces UniformQuantizer.quant on the static path
 *   fake_quant/quantizer/uniform.py:20-33, fake_quant/quantizer/base.py:44-50
 *   (called from ActQuantWrapper.forward, fake_quant/quant_utils.py:378-383).
 *   q = clamp(rint(float(x) / s), -128, 127), IEEE division, round-half-even.
 * x: [M, K] row-major with leading dimension ldx (elements).
 * out: [M, K_pad] int8 row-major, leading dimension ldo (bytes) >= K_pad; columns
 *      K..K_pad-1 are written as 0 so the GEMM can consume whole 128-wide tiles.
 * Scale selection:
 *   scale_vec0 == NULL: per-tensor scales passed by value (scale0 / scale1);
 *   scale_vec0 != NULL: per-channel scales [K] (calibration_mode="channel_wise").
 *   row_sel == NULL: every row uses set 0; else row_sel[m] in {0,1} picks the set
 *   (Modality-Specific Static Quantization: vision vs. text rows).
 * skip_col0 != 0 implements ActQuantWrapper.split (quant_utils.py:367-376): channel 0
 *   bypasses the quantizer: out[:,0] = 0 and x0_out[m] = float(x[m,0]).
 * ------------------------------------------------------------------------- */
int mq_quantize_act_i8(const void *x, int x_dtype, long M, long K, long ldx,
                       float scale0, float scale1,
                       const float *scale_vec0, const float *scale_vec1,
                       const uint8_t *row_sel, int skip_col0, float *x0_out,
                       int8_t *out, long K_pad, long ldo, void *stream);

/* Fused quantize->dequantize in x's dtype (the reference's simulated form,
 * uniform.py:20-43 + base.py:44-50), used when weights stay in floating point. */
int mq_fakequant_act(const void *x, int x_dtype, long M, long K, long ldx,
                     float scale0, float scale1,
                     const float *scale_vec0, const float *scale_vec1,
                     const uint8_t *row_sel, int skip_col0,
                     void *out, long ldo, void *stream);

/* ---------------------------------------------------------------------------
 * Online Hadamard rotation, optionally fused with the static quantizer.
 * Replaces revise_down_input + matmul_hadU_cuda (+ UniformQuantizer.quant):
 *   fake_quant/utils.py:465-471, fake_quant/hadamard_utils.py:115-128,
 *   fake_quant/quant_utils.py:334-341 (and :378-383 when quantizing).
 *   y = (H_K (x) H_{n/K}) [x ; 0] / sqrt(n),  flat index = k*(n/K) + j.
 * x: [M, n_in] (n_in <= n: zero padded up to n, the forward-pre-hook's job).
 * had_words: the signs of hadK as word-aligned rows: uint32 [K][ceil(K/32)], bit b of
 *           word w of row j is 1 when hadK[j][32*w + b] == +1 (unused high bits 0);
 *           NULL when K == 1.  (hadK itself is data: fake_quant/hadamard_utils.py:201-.)
 * fp32_had: 0 = the extension's behaviour for half inputs (butterflies in fp32,
 *           result rounded to x's dtype before the K x K stage and again after),
 *           1 = --fp32_had (fp32 throughout, one final cast to x's dtype).
 * The K x K stage accumulates in ascending k as a single fp32 chain (oracle step 4).
 *
 * mq_hadamard:        writes the rotated activations in x's dtype, [M, n].
 * mq_hadamard_quant_i8: writes int8 levels like mq_quantize_act_i8 (same scale /
 *           row_sel / skip_col0 / x0_out semantics); the rotated activations never
 *           reach HBM.
 * ------------------------------------------------------------------------- */
/* fp32_had is a flag word: MQ_HAD_FP32 = --fp32_had; MQ_HAD_PREPARED = had_words points at a
 * descriptor written by mq_hadamard_prepare (16-byte aligned, mq_hadamard_prepared_bytes(K) bytes): the sign
 * words, followed by the 64-lane masks of the fp32 MFMA sign operand (one VALU instruction per operand instead
 * of three -- the fp32 MFMA shares the vector ALU's datapath, every VALU instruction beside it is lost matrix
 * time) and by the +-1 half-precision operand images of the fast stage (MQ_HAD_FAST).  Results are
 * identical with and without the descriptor. */
#define MQ_HAD_FP32 1
#define MQ_HAD_PREPARED 2
/* NON-DEFAULT accuracy / speed flag of ONE call (there is no process-wide mode): without it the K x K stage is the sequential
 * fp32 add chain of the reference's CPU run, bit-identical to the goldens.  With MQ_HAD_FAST, half-precision activations
 * (x_dtype MQ_F16 / MQ_BF16, MQ_HAD_FP32 off, 64 <= n/K <= 512) run that stage on the fp16 / bf16 matrix core
 * (V_MFMA_F32_32X32X16): the products +-1 * y are exact, only the ORDER of the fp32 accumulation differs -- what the
 * reference's own GPU run does with a half-precision cuBLAS GEMM (hadamard_utils.py:127).  Not bit-identical to the exact
 * kernel: DESIGN.md 4.2 gives the measured int8 level flip rate and the verdict against the reference goldens
 * (tests/test_gpu_hadamard_fast.py).  Shapes / dtypes outside the fast kernel take the exact one. */
#define MQ_HAD_FAST 4
size_t mq_hadamard_prepared_bytes(int K);
int mq_hadamard_prepare(const uint32_t *had_words, int K, void *descriptor, void *stream);

int mq_hadamard(const void *x, int x_dtype, long M, long n_in, long ldx,
                long n, int K, const uint32_t *had_words, int fp32_had,
                void *out, long ldo, void *stream);

int mq_hadamard_quant_i8(const void *x, int x_dtype, long M, long n_in, long ldx,
                         long n, int K, const uint32_t *had_words, int fp32_had,
                         float scale0, float scale1, const uint8_t *row_sel,
                         int skip_col0, float *x0_out,
                         int8_t *out, long K_pad, long ldo, void *stream);

/* Same with the activation that produces the rotated Linear's input fused in front (SURVEY 8(f3):
 * "SiLU.up fused into the down_proj Hadamard-quant prologue"): the row fed to the transform is
 *   act == 1 (MQ_ACT_SILU_MUL):   cast(cast(x / (1 + exp(-x))) * x2)   x = gate, x2 = up (same ldx)
 *   act == 2 (MQ_ACT_QUICK_GELU): cast(x * cast(1 / (1 + exp(-cast(1.702 x)))))
 * i.e. torch's F.silu(gate) * up / QuickGELUActivation on tensors of x_dtype (fp32 inside an op,
 * one rounding per op, the device library's expf): bit-identical to running those torch ops on
 * this GPU and then mq_hadamard_quant_i8 (checked at full size in fp16, bf16 and fp32).  These
 * activations are HF model code, not MQuant's; the C oracle restates them with a correctly rounded
 * exp and agrees up to that last bit.  Requires n/K >= 8. */
int mq_act_hadamard_quant_i8(const void *x, const void *x2, int act, int x_dtype, long M,
                             long n_in, long ldx, long n, int K, const uint32_t *had_words,
                             int fp32_had, float scale0, float scale1, const uint8_t *row_sel,
                             int skip_col0, float *x0_out, int8_t *out, long K_pad, long ldo,
                             void *stream);

/* TEST-ONLY hook (thread-local, not part of the drop-in surface): 256 or 512 threads per row. */
int mq_hadamard_debug_threads(int threads);

/* TEST-ONLY: everything the host decides for a launch of the exact Hadamard kernel with these arguments and the calling thread's
 * mq_hadamard_debug_threads setting -- the launch itself is driven by the same plan.  Host arithmetic only (without a device the
 * CU count is taken as 256).  flags: MQ_HAD_*; quant != 0: mq_hadamard_quant_i8 (act: 0 or MQ_ACT_* of mq_act_hadamard_quant_i8;
 * tiled != 0: ldo = MQ_LD_TILED); aligned: MQ_HAD_ALIGN_* bits.  plan receives MQ_HAD_PLAN_INTS ints, indexed by MQ_HAD_PLAN_*.
 * Returns the code (and mq_last_error the message) of the launch for shapes the launch refuses. */
#define MQ_HAD_ALIGN_X 1    /* x (and x2): 16-byte aligned pointer and row stride, the loads are vector loads */
#define MQ_HAD_ALIGN_Q2 2   /* row-major int8 destination: even row stride */
#define MQ_HAD_ALIGN_Q4 4   /* row-major int8 destination: row stride a multiple of 4 (implies MQ_HAD_ALIGN_Q2) */
#define MQ_HAD_PLAN_THREADS 0      /* 256 / 512 threads per row */
#define MQ_HAD_PLAN_UNIT 1         /* 0, or 5 / 3: mask-driven 5 x 2 / 3 x 2 units of a prepared descriptor */
#define MQ_HAD_PLAN_HALF_LDS 2     /* the row is staged as 16-bit values */
#define MQ_HAD_PLAN_ACT 3          /* the fused-activation instantiation */
#define MQ_HAD_PLAN_PARTS_LOG2 4   /* 2^parts workgroups share one row's K x K units */
#define MQ_HAD_PLAN_GRID 5         /* workgroups */
#define MQ_HAD_PLAN_LDS 6          /* dynamic LDS bytes */
#define MQ_HAD_PLAN_BUTTERFLY 7    /* MQ_HAD_BF_* */
#define MQ_HAD_PLAN_KXK 8          /* MQ_HAD_KXK_* */
#define MQ_HAD_PLAN_REMAP 9        /* tiled output: rows handed out by the XCD row map */
#define MQ_HAD_PLAN_FAST_FIRST 10  /* MQ_HAD_FAST: the fast dispatcher is tried first, this plan is what runs if it declines */
#define MQ_HAD_PLAN_X_VEC 11       /* 16-byte loads of x */
#define MQ_HAD_PLAN_Q_VEC 12       /* int8 levels stored four (two) at a time instead of byte by byte */
#define MQ_HAD_PLAN_INTS 13
#define MQ_HAD_BF_SCALAR 0   /* n/K < 8: scalar staging, every butterfly through LDS */
#define MQ_HAD_BF_LANE 1     /* 8 .. 512: in-lane, DPP and shuffle butterflies */
#define MQ_HAD_BF_REG 2      /* 1024 .. 8192: plus one register-resident pass over the staged row */
#define MQ_HAD_BF_LDS 3      /* above: plus read-modify-write LDS passes from stride 512 */
#define MQ_HAD_KXK_K1_VEC4 0
#define MQ_HAD_KXK_K1_SCALAR 1
#define MQ_HAD_KXK_CLASSIC 2 /* one 16-row tile x four column tiles per wave step, sign words */
#define MQ_HAD_KXK_UNIT5 3
#define MQ_HAD_KXK_UNIT3 4
#define MQ_HAD_KXK_CHAIN 5   /* n/K < 64: scalar chain per output element */
int mq_hadamard_debug_plan(long M, long n_in, long n, int K, int x_dtype, int flags, int quant, int act, int tiled,
                           int aligned, int *plan);

/* ---------------------------------------------------------------------------
 * Weight formats.
 * mq_pack_i4 / mq_unpack_i4: the reference wire format, quant_utils.py:61-94
 *   (two's-complement nibbles, even index -> low nibble, along the last dim).
 * mq_weight_levels: integer levels of a fake-quantized weight,
 *   q[n][k] = clamp(rint(float(w[n][k]) / scale[n]), lo, hi)
 *   (the inverse of WeightQuantizer.quantize, quant_utils.py:42-45,512-518).
 * mq_prepack_w4 / mq_prepack_w8: re-tile int levels [N, K] into the image the GEMM
 *   streams straight into LDS (layout in DESIGN.md).  N_pad = ceil16(N),
 *   K_pad = ceil128(K); padding is zero.  Output bytes: N_pad*K_pad/2 (w4),
 *   N_pad*K_pad (w8).  zero_col0 clears column 0 (ActQuantWrapper.split: L2 has no
 *   column for the bypassed channel, quant_utils.py:320-326).
 * ------------------------------------------------------------------------- */
int mq_pack_i4(const int8_t *q, long rows, long cols, uint8_t *out, void *stream);
int mq_unpack_i4(const uint8_t *packed, long rows, long cols, int8_t *out, void *stream);
int mq_weight_levels(const void *w, int w_dtype, long N, long K, long ldw,
                     const float *scale, int lo, int hi, int8_t *q, void *stream);
int mq_prepack_w4(const int8_t *q, long N, long K, int zero_col0, uint8_t *out, void *stream);
int mq_prepack_w8(const int8_t *q, long N, long K, int zero_col0, int8_t *out, void *stream);
size_t mq_prepacked_bytes(long N, long K, int w_bits);

/* ---------------------------------------------------------------------------
 * Dynamic per-token activation quantizer: the reference's DEFAULT mode when --*_static is not
 * given (ActQuantizer.find_params + forward, quant_utils.py:116-133,205-268; symmetric,
 * act_per_tensor = False, groupsize = -1).  Per row m, fp32 arithmetic on the converted values:
 *   xmin = min(min_k x, 0)*clip_ratio; xmax = max(max_k x, 0)*clip_ratio; maxq = 2^(bits-1)-1
 *   scale_out[m] = max(|xmin|, xmax) / maxq   (1 where that is 0)
 *   out[m][k]    = clamp(rint(x / scale_out[m]), -(maxq+1), maxq), zero for K <= k < K_pad
 * skip_col0: column 0 is left out of the range, returned in x0_out and given level 0
 * (ActQuantWrapper.split, quant_utils.py:367-372).  Pair with mq_gemm_w4a8_rowscale_ws.
 * ------------------------------------------------------------------------- */
int mq_quantize_act_dyn_i8(const void *x, int x_dtype, long M, long K, long ldx, int bits,
                           float clip_ratio, int skip_col0, float *x0_out, float *scale_out,
                           int8_t *out, long K_pad, long ldo, void *stream);

/* The ASYMMETRIC variant (--a_asym without --*_static; quant_utils.py:239-268 else-branch + asym_quant
 * :27-31), maxq = 2^bits - 1, per row m:
 *   xmin / xmax as above (both 0 -> -1 / +1); scale = (xmax - xmin) / maxq; zero = rint(-xmin / scale)
 *   q = clamp(rint(x / scale) + zero, 0, maxq);  out[m][k] = q - 2^(bits-1)  (int8), zero for k >= K
 *   shift_out[m] = scale * (2^(bits-1) - zero):  x_hat[m][k] = scale * out[m][k] + shift_out[m]
 * Pair with mq_gemm_w4a8_rowscale_ws(s_x_rows = scale_out, x0 = shift_out, w0[n] = s_w[n] * sum_k q_w[n][k]):
 * the rank-1 epilogue term restores offset and zero point.  zero_out may be NULL. */
int mq_quantize_act_dyn_asym_i8(const void *x, int x_dtype, long M, long K, long ldx, int bits,
                                float clip_ratio, float *scale_out, float *zero_out, float *shift_out,
                                int8_t *out, long K_pad, long ldo, void *stream);

/* The PER-TENSOR variant (act_per_tensor = True; quant_utils.py:214-237): one range for the whole
 * tensor, taken from `minmax` = the two device floats written by mq_minmax_tensor (col_begin = 1 under
 * skip_col0) -- no host round trip.  asym = 0: scale = max(|xmin|, xmax) / (2^(bits-1) - 1) (1 if 0);
 * asym = 1: a zero bound becomes -1 resp. +1 on its own, scale / zero / stored levels / shift as in
 * mq_quantize_act_dyn_asym_i8 (no skip_col0 then).  scale_out (and zero_out / shift_out, may be NULL when
 * asym = 0) are written per row for mq_gemm_w4a8_rowscale_ws.  For fp16 / bf16 inputs every step is rounded to
 * x's dtype like the reference's (range * clip, scale, zero point, x / scale, level sum are 16-bit tensors there:
 * `torch.tensor(0).to(x)`, the int64 maxq tensor does not promote); the per-token entry points promote to fp32 (:239). */
int mq_quantize_act_range_i8(const void *x, int x_dtype, long M, long K, long ldx, int bits,
                             float clip_ratio, int asym, int skip_col0, const float *minmax,
                             float *x0_out, float *scale_out, float *zero_out, float *shift_out,
                             int8_t *out, long K_pad, long ldo, void *stream);

/* ---------------------------------------------------------------------------
 * RMSN + static quantizer in one pass.  Replaces module_util.RMSN.forward
 * (module_util.py:55-61) followed by UniformQuantizer.quant (uniform.py:20-33):
 *   h = fp32(x);  y = cast_to_x_dtype(h * (1/sqrt(sum(h*h)/mean_dim + eps)));
 *   out[m][k] = clamp(rint(y / scale_sel(m)), -128, 127), zero for K <= k < K_pad
 * x: [M, ldx], rows 16-byte aligned, K % 16 == 0 (MQ_BF16 rows are normalised in bf16 arithmetic, one
 * rounding per torch op, because upstream promotes fp16 only),
 * K <= 16384.  y_out (optional, [M, ldy], x's dtype) receives the normalised activations.
 * The sum of squares uses the fixed order documented in csrc/rmsn_quant.hip (oracle: orc_rmsn);
 * torch's own reduction order differs in the last fp32 bit, i.e. <= 1 ulp of y.
 * ------------------------------------------------------------------------- */
int mq_rmsn_quantize_i8(const void *x, int x_dtype, long M, long K, long ldx, float mean_dim,
                        float eps, float scale0, float scale1, const uint8_t *row_sel,
                        void *y_out, long ldy, int8_t *out, long K_pad, long ldo, void *stream);

/* ---------------------------------------------------------------------------
 * Weight quantizer on the device (offline weight pipeline).
 * Replaces WeightQuantizer.find_params + WeightQuantizer.quantize for the symmetric
 * per-output-channel case, quant_utils.py:446-518 (sym_quant_dequant :46-58):
 *   xmax[n]  = max(|min(min_k w, 0)|, max(max_k w, 0)) clamped to >= 1e-5
 *   scale[n] = xmax / maxq,  maxq = 2^(bits-1) - 1
 *   mse != 0: clip search over p = 1 - i/grid, i < (int)(maxshrink*grid):
 *             err_i = sum_k |s_i*q - w|^norm (fp32, ascending k), first strict minimum wins
 *   q[n][k]  = clamp(rint(w/scale[n]), -(maxq+1), maxq)
 * All arithmetic is fp32 on the exactly converted weights for EVERY w_dtype (the reference
 * promotes half tensors through the fp32 `tmp` of :458-460).  Optional outputs (NULL = skip):
 *   levels  int8 [N, K]
 *   packed  uint8 [N, K/2], the reference pack_i4 wire format (:61-69); bits == 4, K even
 *   wq      fake-quantized weights scale*q cast to w_dtype, [N, ldq] (what quantize() returns)
 * ------------------------------------------------------------------------- */
int mq_wquant_sym(const void *w, int w_dtype, long N, long K, long ldw, int bits, int mse,
                  float norm, int grid, float maxshrink, float *scale, int8_t *levels,
                  uint8_t *packed, void *wq, long ldq, void *stream);

/* ---------------------------------------------------------------------------
 * Rotary embedding (rotate-half), in place on `heads` consecutive head_dim-wide column blocks of
 * x [T, ldx] -- e.g. the q and k parts of a fused q|k|v GEMM output.  Not an MQuant function (the
 * reference never touches RoPE): glue of the whole-prefill TTFT harness, bit-identical to the HF
 * formula evaluated with torch ops on x_dtype tensors:
 *   out = cast(cast(x*cos) + cast(rotate_half(x)*sin)),  cos/sin: [T, head_dim] in x_dtype.
 * ------------------------------------------------------------------------- */
int mq_rope_inplace(void *x, int x_dtype, long T, int heads, int head_dim, long ldx,
                    const void *cos, const void *sin, void *stream);

/* ---------------------------------------------------------------------------
 * Offline rotation of weight rows in fp64.  Replaces the dense
 *   W <- (W.double() @ Q).to(W.dtype),  Q = random_hadamard_matrix(n) = diag(s) H_n / sqrt(n)
 * of fake_quant/rotation_utils.py (rotate_* helpers) as driven by qwen2vl_rotation.py:232-332 and
 * internvl_rotation.py:223-303; Q is built at hadamard_utils.py:107-112.  In place, per row:
 *   x <- cast( (H_K (x) H_{n/K}) (s . x) / (double)sqrtf(n) ),   flat index = k*(n/K) + j,
 * evaluated in fp64 (sign flip, butterflies, K x K sign stage, one division), cast to x's dtype
 * through fp32 like torch's double -> half conversion.  signs: n doubles (+-1), NULL = no flip
 * (plain H_n, e.g. the per-head Hadamard).  had_words as for mq_hadamard (plain words, NULL when
 * K == 1).  Q^T W is the same call on the rows of W^T.  n * 8 bytes must fit the 160 KiB LDS.
 * ------------------------------------------------------------------------- */
int mq_rotate_f64(void *x, int dtype, long M, long n, long ld, const double *signs,
                  int K, const uint32_t *had_words, void *stream);

/* ---------------------------------------------------------------------------
 * fp8 KV cache (BASELINE configuration 5).  No reference implementation exists
 * (fake_quant/utils.py:220-267 are flags of a parser nobody calls): parity is UNPINNED, the checker
 * is oracle/mq_oracle.c (orc_kv_quant_fp8 / orc_kv_dequant_fp8; its e4m3fn codec is pinned to
 * torch.float8_e4m3fn on the CPU).  OCP e4m3fn (not fnuz), one static scale per KV head:
 *   write:  q[t][h][d] = e4m3fn_rne(clamp(kv[t][h][d] / scale[h], -448, 448))
 *   read:   out[t][h][d] = cast(float(q[t][h][d]) * scale[h])
 * kv / out: [T][ld] elements with the heads * head_dim values of a token contiguous (ld lets the
 * K or V slice of a fused qkv GEMM output be read in place); q: [T][ldo] bytes.  head_dim % 8 == 0,
 * rows 16-byte aligned (8 for the fp8 side).
 * ------------------------------------------------------------------------- */
int mq_kv_quant_fp8(const void *kv, int dtype, long T, int heads, int head_dim, long ld,
                    const float *scale, uint8_t *out, long ldo, void *stream);
int mq_kv_dequant_fp8(const uint8_t *q, long T, int heads, int head_dim, long ld,
                      const float *scale, void *out, int out_dtype, long ldo, void *stream);
/* The write with the READ-BACK fused in: besides the e4m3 bytes it stores readback[t][h][d] = cast(float(q) * s[h])
 * (what mq_kv_dequant_fp8 would return later) in the source dtype, row stride ldr elements -- the K / V the
 * attention of the SAME prefill step consumes, so prefill and decode attend over identical values and the
 * separate dequantise-on-read launch is gone.  readback == NULL: mq_kv_quant_fp8. */
int mq_kv_quant_fp8_readback(const void *kv, int dtype, long T, int heads, int head_dim, long ld,
                             const float *scale, uint8_t *out, long ldo, void *readback, long ldr, void *stream);

/* Prefill attention straight off the e4m3 cache (no reference counterpart -- the reference leaves
 * attention to the HF model code and never quantizes a cache; parity unpinned, checker = softmax attention over the
 * dequantised cache).  K and V are read as ONE byte per element and widened inside the kernel; the per-head scales
 * fold into the score / output scale, so no dequantised copy of the cache ever exists in HBM:
 *     O[t][h][:] = softmax_k((Q[t][h] . K8[k][g]) * s[g] * softmax_scale) @ V8[k][g] * s[kv_heads + g],  g = h / (heads / kv_heads)
 * q / out: [T][ld] elements of `dtype` (MQ_F16 / MQ_BF16) with heads * head_dim values per token (ldq lets the Q
 * columns of a fused q|k|v GEMM output be read in place); kv_cache: [T][ldkv] bytes, per token the K heads then the
 * V heads (the layout mq_kv_quant_fp8 writes for the K|V columns); kv_scale: [2 * kv_heads] floats.  head_dim == 128;
 * q / cache rows 16-byte aligned, out rows 8-byte aligned.  causal != 0: key index <= query index. */
int mq_attn_prefill_fp8kv(const void *q, int dtype, long T, int heads, int kv_heads, int head_dim, long ldq,
                          const uint8_t *kv_cache, long ldkv, const float *kv_scale, float softmax_scale,
                          int causal, void *out, long ldo, void *stream);
/* The same kernel over UNQUANTISED K / V of q's dtype (the K and V column slices of the fused q|k|v GEMM output, read in
 * place): k / v point at the first K / V head of token 0, a token's kv_heads * head_dim values contiguous, row stride ldkv
 * ELEMENTS.  head_dim 128, 80 (Qwen2-VL's vision tower), 64 (InternViT-300M, InternVL2's tower) or 104 (Qwen-VL's ViT); a
 * head stays 16-byte aligned at each (160, 128 and 208 bytes).  Nothing outside a head's own head_dim columns is read: 104 is
 * contracted over 112 with zeros supplied inside the kernel.  Replaces repeat_kv + scaled_dot_product_attention in the glue of
 * the whole-prefill report. */
int mq_attn_prefill(const void *q, int dtype, long T, int heads, int kv_heads, int head_dim, long ldq,
                    const void *k, const void *v, long ldkv, float softmax_scale, int causal, void *out, long ldo,
                    void *stream);
/* TEST-ONLY, thread-local: force the waves per workgroup (= ways the keys are split) of the attention kernels: 2 or 4; 0 = by shape. */
int mq_attn_debug_waves(int waves);

/* Either attention with the NEXT Linear's static int8 activation quantizer fused into its store (the o_proj /
 * proj input): out[t][c] = clamp(rint(cast_dtype(o[t][c]) / s_t), -128, 127), s_t = scale1 where row_sel[t] != 0 else
 * scale0 -- the bytes mq_quantize_act_i8 writes for the 16-bit attention output, in the same activation layout (K_pad ==
 * heads * head_dim, a multiple of 64; ldo = MQ_LD_TILED or a row stride).  kv_cache != NULL: the e4m3 variant (k, v, ldkv
 * ignored; head_dim 128); else the 16-bit variant (kv_cache, ld_cache, kv_scale ignored; head_dim 128, 80, 64 or 104). */
int mq_attn_prefill_quant_i8(const void *q, int dtype, long T, int heads, int kv_heads, int head_dim, long ldq,
                             const void *k, const void *v, long ldkv, const uint8_t *kv_cache, long ld_cache,
                             const float *kv_scale, float softmax_scale, int causal, float scale0, float scale1,
                             const uint8_t *row_sel, int8_t *out, long K_pad, long ldo, void *stream);

/* Decode attention straight off the e4m3 cache: the generation-step counterpart of mq_attn_prefill_fp8kv (the same arithmetic, no
 * reference counterpart, parity unpinned; checker = softmax attention over the dequantised cache, tests/attn_decode_reference.py).
 * R query rows (1 .. 8, the LAST R positions of a sequence of n tokens) attend over the first n keys of a cache of capacity >= T:
 *     O[r][h][:] = softmax_k((Q[r][h] . K8[k][g]) * s[g] * softmax_scale) @ V8[k][g] * s[kv_heads + g],  g = h / (heads / kv_heads)
 * causal != 0: row r attends keys 0 .. n - R + r (R == 1: all n keys); causal == 0: every row attends all n keys.
 * n_keys_dev == NULL: n = T.  Else n = clamp(*n_keys_dev, R, T), read on the device by the launches themselves, and T is only the
 * capacity the plan and the grid are sized for: a generation loop is captured once and replayed while the cache grows.  Nothing at
 * or beyond key n reaches the output, whatever those cache rows hold.
 * q / out: [R][ld] elements of `dtype` (MQ_F16 / MQ_BF16) with heads * head_dim values per row (ldq lets the Q columns of a fused
 * q|k|v GEMM output be read in place); kv_cache: [T][ldkv] bytes, per token the K heads then the V heads (the layout
 * mq_kv_quant_fp8 writes for the K|V columns); kv_scale: [2 * kv_heads] floats.  head_dim == 128; q / cache rows 16-byte aligned,
 * out rows 8-byte aligned.
 * One workgroup serves one (kv head, range of keys): a cache byte is fetched once per kv head, not once per query head; R * heads /
 * kv_heads <= 16 is one pass over the keys, more rows take several.  When the plan cuts the keys into more than one range, every
 * range writes a partial state into `workspace` (fp32, 16-byte aligned, at least mq_attn_decode_workspace_bytes(R, T, heads,
 * kv_heads) bytes) and a second launch on the same stream merges the ranges in index order: same inputs, same plan, same bits.
 * The workspace needs no initialisation and holds nothing between calls. */
int mq_attn_decode_fp8kv(const void *q, int dtype, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads, int head_dim,
                         long ldq, const uint8_t *kv_cache, long ldkv, const float *kv_scale, float softmax_scale, int causal,
                         void *out, long ldo, void *workspace, size_t workspace_bytes, void *stream);
/* The same with the NEXT Linear's static int8 activation quantizer fused into the final store, exactly as
 * mq_attn_prefill_quant_i8 defines it: out[r][c] = clamp(rint(cast_dtype(o[r][c]) / s_r), -128, 127), s_r = scale1 where
 * row_sel[r] != 0 else scale0 (K_pad == heads * head_dim, a multiple of 64; ldo = MQ_LD_TILED or a row stride). */
int mq_attn_decode_fp8kv_quant_i8(const void *q, int dtype, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads, int head_dim,
                                  long ldq, const uint8_t *kv_cache, long ldkv, const float *kv_scale, float softmax_scale, int causal,
                                  float scale0, float scale1, const uint8_t *row_sel, int8_t *out, long K_pad, long ldo,
                                  void *workspace, size_t workspace_bytes, void *stream);
/* The same two calls over a 16-BIT cache (the reference's default: k_bits = v_bits = 16 leave K / V as they are): kv_cache is
 * [T][ldkv] ELEMENTS of `dtype`, per token the K heads then the V heads -- the e4m3 layout at two bytes per element, what
 * mq_kv_append_rope writes and what mq_attn_prefill reads with k = kv_cache, v = kv_cache + kv_heads * head_dim -- and there are
 * no scales:
 *     O[r][h][:] = softmax_k((Q[r][h] . K[k][g]) * softmax_scale) @ V[k][g]
 * Everything else is as above -- n, the clamp, causal, the strides, the workspace, the plan (it does not depend on the storage) --
 * and so is the arithmetic: the e4m3 kernel with both scales 1.0f, so equal cache VALUES give equal bits.  (T + 32) * ldkv * 2 must
 * stay below 4 GiB.  No reference counterpart, parity unpinned; checker = float64 softmax attention over the cache,
 * tests/attn_decode_reference.py. */
int mq_attn_decode(const void *q, int dtype, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads, int head_dim,
                   long ldq, const void *kv_cache, long ldkv, float softmax_scale, int causal,
                   void *out, long ldo, void *workspace, size_t workspace_bytes, void *stream);
/* ... with the fused int8 quantizer of mq_attn_decode_fp8kv_quant_i8 (checker = mq_quantize_act_i8 of mq_attn_decode's output). */
int mq_attn_decode_quant_i8(const void *q, int dtype, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads, int head_dim,
                            long ldq, const void *kv_cache, long ldkv, float softmax_scale, int causal,
                            float scale0, float scale1, const uint8_t *row_sel, int8_t *out, long K_pad, long ldo,
                            void *workspace, size_t workspace_bytes, void *stream);
/* Bytes of workspace the plan of such a call needs: 0 when the keys are not split.  Host arithmetic only (0 also for arguments the
 * call would refuse). */
size_t mq_attn_decode_workspace_bytes(int R, long T, int heads, int kv_heads);
/* TEST-ONLY, thread-local: force the number of key ranges and / or the keys per range (a multiple of 32) of the decode attention;
 * 0 = the heuristic.  A forced pair that does not cut T keys into non-empty ranges is refused by the call. */
int mq_attn_decode_debug_force(int splits, int keys_per_split);
/* TEST-ONLY: what the host decides for a call with these arguments and the calling thread's mq_attn_decode_debug_force setting --
 * the launch is driven by the same function.  Host arithmetic only (without a device the CU count is taken as 256).  plan receives
 * MQ_ATTN_DECODE_PLAN_INTS ints.  Returns the code (and mq_last_error the message) of the call for arguments the call refuses. */
#define MQ_ATTN_DECODE_PLAN_SPLITS 0           /* key ranges */
#define MQ_ATTN_DECODE_PLAN_KEYS_PER_SPLIT 1   /* keys per range, a multiple of the 32-key block */
#define MQ_ATTN_DECODE_PLAN_GRID 2             /* workgroups of the first launch: kv_heads x splits */
#define MQ_ATTN_DECODE_PLAN_PASSES 3           /* passes over the keys inside a workgroup: ceil(R * heads / kv_heads / 16) */
#define MQ_ATTN_DECODE_PLAN_WORKSPACE 4        /* workspace bytes */
#define MQ_ATTN_DECODE_PLAN_INTS 5
int mq_attn_decode_debug_plan(int R, long T, int heads, int kv_heads, int *plan);

/* The four decode attention calls over a BATCH: B sequences (1 .. 65535) of R rows each in one pair of launches, so that a
 * generation step streams the weights once for B tokens.  Sequence b is the second grid dimension of both launches and uses
 *   - its own key count n_b = clamp(n_keys_dev[b], R, T) (n_keys_dev: [B] int32 on the device; NULL: every sequence has T keys),
 *   - its own cache at kv_cache + b * seq_stride ELEMENTS of the storage (64-bit arithmetic; seq_stride >= T * ldkv, a multiple of
 *     16 bytes).  The 32-bit offsets inside a cache stay per sequence: (T + 32) x the row stride < 4 GiB holds for ONE sequence,
 *     the batch as a whole may be larger,
 *   - rows [b R, (b + 1) R) of q, out and row_sel (q / out: [B * R][ld]; the fused int8 store addresses global row b R + r, also in
 *     the tiled layout),
 *   - its own slice of `workspace`, which holds at least mq_attn_decode_batch_workspace_bytes(B, R, T, heads, kv_heads) bytes.
 * Everything inside a workgroup is the single-sequence kernel: a split at or beyond n_b leaves without writing and the merge does not
 * read its slot; nothing at or beyond key n_b of sequence b reaches the output, whatever those cache rows hold.  The plan is that of
 * the siblings with 2 x CUs / (kv_heads x B) key ranges wanted per sequence (B = 1: the sibling's plan, integer for integer);
 * mq_attn_decode_debug_force applies.  The output bits of sequence b depend on its own q, cache and length and on (splits, keys per
 * split) only: a batched call equals B single-sequence calls under the same plan, bit for bit.  B = 1 ignores seq_stride and IS the
 * sibling.  Everything else -- dtypes, strides, alignment, causal, the quantizer -- as the siblings state it. */
int mq_attn_decode_fp8kv_batch(const void *q, int dtype, int B, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads,
                               int head_dim, long ldq, const uint8_t *kv_cache, long ldkv, long seq_stride, const float *kv_scale,
                               float softmax_scale, int causal, void *out, long ldo, void *workspace, size_t workspace_bytes,
                               void *stream);
int mq_attn_decode_fp8kv_quant_i8_batch(const void *q, int dtype, int B, int R, long T, const int32_t *n_keys_dev, int heads,
                                        int kv_heads, int head_dim, long ldq, const uint8_t *kv_cache, long ldkv, long seq_stride,
                                        const float *kv_scale, float softmax_scale, int causal, float scale0, float scale1,
                                        const uint8_t *row_sel, int8_t *out, long K_pad, long ldo, void *workspace,
                                        size_t workspace_bytes, void *stream);
int mq_attn_decode_batch(const void *q, int dtype, int B, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads,
                         int head_dim, long ldq, const void *kv_cache, long ldkv, long seq_stride, float softmax_scale, int causal,
                         void *out, long ldo, void *workspace, size_t workspace_bytes, void *stream);
int mq_attn_decode_quant_i8_batch(const void *q, int dtype, int B, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads,
                                  int head_dim, long ldq, const void *kv_cache, long ldkv, long seq_stride, float softmax_scale,
                                  int causal, float scale0, float scale1, const uint8_t *row_sel, int8_t *out, long K_pad, long ldo,
                                  void *workspace, size_t workspace_bytes, void *stream);
/* The workspace of a batched call (B x the per-sequence figure of ITS plan) and its plan, in the MQ_ATTN_DECODE_PLAN_* slots: SPLITS,
 * KEYS_PER_SPLIT and PASSES per sequence, GRID = all kv_heads x splits x B workgroups of the first launch, WORKSPACE for the whole
 * batch.  Host arithmetic only, as the siblings. */
size_t mq_attn_decode_batch_workspace_bytes(int B, int R, long T, int heads, int kv_heads);
int mq_attn_decode_batch_debug_plan(int B, int R, long T, int heads, int kv_heads, int *plan);

/* The launch in front of mq_attn_decode_fp8kv in a generation step: rotate Q and K of the R new rows (1 .. 8) in place and
 * quantise K|V into rows [n - R, n) of the e4m3 cache, at a position read from DEVICE memory -- with it a whole decode step is
 * captured once and advances by incrementing one int32 (no reference counterpart; checkers = mq_rope_inplace and mq_kv_quant_fp8).
 * qkv: [R][ldqkv] elements of `dtype` (MQ_F16 / MQ_BF16), the fused projection output: per row `heads` Q heads, kv_heads K heads,
 * kv_heads V heads, head_dim wide each.  n = n_keys_dev ? clamp(*n_keys_dev, R, T) : T is the key count AFTER the append -- the
 * integer and the clamp of mq_attn_decode_fp8kv, which runs next on the stream; T = capacity of the cache in rows.  Row r is token
 * t = n - R + r and takes row p = clamp(t + (rope_delta_dev ? *rope_delta_dev : 0), 0, table_rows - 1) of the tables (cos / sin:
 * [table_rows][head_dim] in `dtype`, contiguous; the offset is HF Qwen2-VL's rope_deltas: after an image the text position is not
 * the cache index).  Both clamps are memory safety, not semantics: no device value moves an access outside the buffers the host
 * checked.
 *   - the Q and K columns of qkv receive the bits of mq_rope_inplace(row r, heads + kv_heads, head_dim, cos + p * head_dim, sin + ..);
 *   - cache row t receives the rotated K heads, then the V heads: the bytes of mq_kv_quant_fp8 applied to the rotated row
 *     (kv_scale: [2 * kv_heads] floats), in the layout the attention kernels read;
 *   - the V columns of qkv and every other cache byte (padding between 2 * kv_heads * head_dim and ldkv included) are not written.
 * cos == NULL && sin == NULL: append only, nothing is rotated; exactly one of them NULL is refused.  head_dim a multiple of 16;
 * qkv rows and the tables 16-byte aligned, cache rows 8-byte aligned, the device integers 4-byte aligned.  One launch whose grid
 * depends on R, heads, kv_heads and head_dim only. */
int mq_kv_append_rope_fp8(void *qkv, int dtype, int R, long T, const int32_t *n_keys_dev, const int32_t *rope_delta_dev,
                          int heads, int kv_heads, int head_dim, long ldqkv,
                          const void *cos, const void *sin, long table_rows,
                          uint8_t *kv_cache, long ldkv, const float *kv_scale, void *stream);
/* The launch in front of mq_attn_decode: mq_kv_append_rope_fp8 word for word -- the same n, t and p, the same two clamps, the same
 * append-only mode -- into a 16-BIT cache ([T][ldkv] elements of `dtype`): cache row t receives the BITS of the rotated, rounded K
 * heads and then the bits of the V heads; nothing is quantised and there are no scales (checker = mq_rope_inplace, then a copy).
 * The V columns of qkv and every cache byte outside row t's 2 * kv_heads * head_dim elements are not written.  head_dim a multiple
 * of 16; qkv rows, the tables and the cache rows 16-byte aligned. */
int mq_kv_append_rope(void *qkv, int dtype, int R, long T, const int32_t *n_keys_dev, const int32_t *rope_delta_dev,
                      int heads, int kv_heads, int head_dim, long ldqkv,
                      const void *cos, const void *sin, long table_rows,
                      void *kv_cache, long ldkv, void *stream);
/* The two appends over a BATCH of B sequences (1 .. 65535) of R new rows each, in front of the batched decode attention: qkv is
 * [B * R][ldqkv], rows [b R, (b + 1) R) belong to sequence b; n_b = clamp(n_keys_dev[b], R, T) and the offset rope_delta_dev[b] are
 * per sequence (both [B] int32 on the device, either may be NULL as above: every sequence has its own image, hence its own offset);
 * sequence b's cache starts at kv_cache + b * seq_stride elements (seq_stride >= T * ldkv, a multiple of 16 bytes; ignored at B = 1).
 * Per sequence everything is the sibling: both clamps, the lane-to-element map, append-only mode, what is and is not written -- the
 * bytes between the caches of two sequences included. */
int mq_kv_append_rope_fp8_batch(void *qkv, int dtype, int B, int R, long T, const int32_t *n_keys_dev, const int32_t *rope_delta_dev,
                                int heads, int kv_heads, int head_dim, long ldqkv,
                                const void *cos, const void *sin, long table_rows,
                                uint8_t *kv_cache, long ldkv, long seq_stride, const float *kv_scale, void *stream);
int mq_kv_append_rope_batch(void *qkv, int dtype, int B, int R, long T, const int32_t *n_keys_dev, const int32_t *rope_delta_dev,
                            int heads, int kv_heads, int head_dim, long ldqkv,
                            const void *cos, const void *sin, long table_rows,
                            void *kv_cache, long ldkv, long seq_stride, void *stream);

/* out[m][n] = sum_k x[m][k] * W[n][k], 16-bit x ([M <= 8, K], ldx elements per row) and W ([N, K], ldw), fp32 products and sums,
 * one rounding to the same 16-bit dtype: the UNQUANTIZED lm_head on the last position(s) of a prefill (the reference leaves
 * lm_head in 16 bits: exam/quant_qwen2vl.py:130-143 wraps the decoder's and the vision tower's Linears only; HF computes
 * logits = lm_head(hidden[:, -1:])).  Glue of the whole-prefill report, replaces torch.matmul (hipBLASLt) there: W is
 * streamed once at the chip's HBM rate.  K a multiple of 8, rows 16-byte aligned, M * K * 2 bytes <= 64 KiB. */
int mq_gemv_f16(const void *x, int dtype, int M, long K, long ldx, const void *w, long N, long ldw, void *out, long ldo,
                void *stream);
/* The same product with the greedy token picked on the device: the last launch of a captured generation step.  y[m][n] are the
 * 16-bit values mq_gemv_f16 stores for the same arguments, bit for bit (one kernel template, the same grid, row hand-out and
 * summation order).  logits != NULL: those bits are written there exactly as mq_gemv_f16 writes them ([M][ldo], ldo >= N);
 * logits == NULL: no logit reaches memory at all.  token_out[m] (device, int32) = argmax over n of the ROUNDED y[m][n] by IEEE
 * comparison, as the CPU torch.argmax defines it: among equal values the lowest index, -0 equals +0, a NaN counts as maximal and the
 * first NaN wins.  Every workgroup of the first launch writes M partial (value, index) results, 8 bytes each, into `workspace`
 * (16-byte aligned, at least mq_gemv_argmax_workspace_bytes(M, N) bytes); a second launch on the same stream takes their maximum
 * -- associative and commutative, so no atomics and no arrival counter: same inputs, same token.  The workspace needs no
 * initialisation and holds nothing between calls.  Everything mq_gemv_f16 requires, and 1 <= N < 2^31 (an argmax over nothing is
 * refused); token_out 4-byte aligned.  M == 0 returns MQ_OK and writes nothing. */
int mq_gemv_f16_argmax(const void *x, int dtype, int M, long K, long ldx, const void *w, long N, long ldw, void *logits, long ldo,
                       int32_t *token_out, void *workspace, size_t workspace_bytes, void *stream);
/* Bytes of workspace such a call needs: workgroups of the launch plan x M x 8, rounded up to 16.  Host arithmetic only (without a
 * device the CU count is taken as 256); 0 for arguments the call refuses (and for M == 0, which needs none). */
size_t mq_gemv_argmax_workspace_bytes(int M, long N);

/* The first launch of a captured generation step: out[r][0 .. dim) = table[clamp(ids_dev[r], 0, vocab - 1)][0 .. dim), a bit copy of
 * R = 1 .. 8 rows of a 16-bit embedding table ([vocab][ldt] elements of `dtype`, MQ_F16 / MQ_BF16) at ids read from DEVICE memory --
 * what mq_gemv_f16_argmax left in token_out -- so a step feeds itself (no reference counterpart; checker = the rows themselves).
 * id_log != NULL: the clamped id of row r is also stored at id_log[n - R + r], n = n_keys_dev ? clamp(*n_keys_dev, R, log_rows) :
 * log_rows -- the integer and the clamp of mq_kv_append_rope_fp8, so the log ([log_rows] int32) is indexed by cache position and the
 * host reads N generated ids after N replays.  Both clamps are memory safety, not semantics: no device value moves an access outside
 * the buffers the host checked.  Nothing else is written: no other log entry, no byte of out beyond dim in a row.  dim a multiple
 * of 8, table and out rows 16-byte aligned (16-byte loads and stores), the device integers 4-byte aligned.  One launch whose grid
 * depends on R and dim only. */
int mq_embed_gather(const void *table, int dtype, long vocab, long dim, long ldt, const int32_t *ids_dev, int R, void *out, long ldo,
                    int32_t *id_log, long log_rows, const int32_t *n_keys_dev, void *stream);
/* The same launch for B = 1 .. 8 SEQUENCES of one new row each (the first launch of a batched generation step):
 * out[b] = table[clamp(ids_dev[b], 0, vocab - 1)], and with id_log != NULL ([B][ld_log] int32, ld_log >= log_rows) the clamped id of
 * sequence b is stored at id_log[b * ld_log + n_b - 1], n_b = n_keys_dev ? clamp(n_keys_dev[b], 1, log_rows) : log_rows
 * (n_keys_dev: [B]).  Nothing else is written. */
int mq_embed_gather_batch(const void *table, int dtype, long vocab, long dim, long ldt, const int32_t *ids_dev, int B, void *out,
                          long ldo, int32_t *id_log, long ld_log, long log_rows, const int32_t *n_keys_dev, void *stream);


/* ---------------------------------------------------------------------------
 * GPTQ: the column loop of one lazy-batch block, gptq/gptq_utils.py:258-279 (symmetric
 * per-channel quantizer, no groups).  For i = 0..cols-1, per output row n:
 *   q = scale[n]*clamp(rint(w_i/scale[n]), -2^(bits-1), 2^(bits-1)-1);  err = (w_i - q)/Hinv1[i][i];
 *   w_j -= err*Hinv1[i][j]  (j > i);   Q1[n][i] = q;  Err1[n][i] = err
 * fp32, the reference's operation order (bit-identical to the torch loop).  W1 is read only
 * ([N, ldw], the block's columns of the working weights), cols <= 128, Hinv1 points at
 * Hinv[i1][i1] of the upper Cholesky factor with leading dimension ldh.  The caller applies the
 * trailing update W[:, i2:] -= Err1 @ Hinv[i1:i2, i2:] (a plain GEMM) as upstream does.
 * ------------------------------------------------------------------------- */
int mq_gptq_block(const float *W1, long N, int cols, long ldw, const float *Hinv1, long ldh,
                  const float *scale, int bits, float *Q1, long ldq, float *Err1, long lde,
                  void *stream);

/* ---------------------------------------------------------------------------
 * Quantized Linear: int8 activations x int4/int8 weights -> int32 -> dequant.
 * Replaces F.linear on fake-quantized tensors, quant_utils.py:384 (and the fp32
 * L1/L2 pair of :374-376 when x0/w0 are given), with
 *   acc[m][n] = sum_k a[m][k] * w[n][k]                      (int32, exact)
 *   y[m][n]   = ((float(acc) * s_x[row_sel[m]]) * s_w[n]) + bias[n] + x0[m]*w0[n]
 * each fp32 operation rounded once, in that order, then cast to out_dtype.
 * a: [M, K_pad] int8, leading dimension lda (bytes, multiple of 16) or lda = MQ_LD_TILED (the
 *    layout the quantizers write on request, fastest), K_pad % 128 == 0.
 * w: image produced by mq_prepack_w4 / _w8 for (N, K) with the same K_pad.
 * bias, x0, w0, row_sel may be NULL.  out: [M, N], leading dimension ldo (elements).
 * mq_gemm_w4a8_i32 stores the raw accumulators (parity interface).
 * ------------------------------------------------------------------------- */
int mq_gemm_w4a8(const int8_t *a, long lda, const void *w, int w_bits,
                 long M, long N, long K_pad,
                 float s_x0, float s_x1, const uint8_t *row_sel,
                 const float *s_w, const float *bias,
                 const float *x0, const float *w0,
                 void *out, int out_dtype, long ldo, void *stream);

/* Same GEMM with the residual add of the surrounding block folded into the epilogue:
 *   out[m][n] = cast(cast(y[m][n]) + residual[m][n])
 * i.e. torch's `hidden + linear(x)` on tensors of out_dtype (the Linear's output is rounded to
 * out_dtype before the add).  residual: [M, ldr] in out_dtype; may alias out (each element is read
 * and written by the same lane). */
int mq_gemm_w4a8_residual_ws(const int8_t *a, long lda, const void *w, int w_bits, long M, long N,
                             long K_pad, float s_x0, float s_x1, const uint8_t *row_sel,
                             const float *s_w, const float *bias, const float *x0, const float *w0,
                             const void *residual, long ldr, void *out, int out_dtype, long ldo,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Same GEMM with one activation scale PER ROW (s_x_rows[m], from mq_quantize_act_dyn_i8) instead of
 * the static scale set(s):  y[m][n] = ((float(acc) * s_x_rows[m]) * s_w[n]) + bias[n] + x0[m]*w0[n]. */
int mq_gemm_w4a8_rowscale_ws(const int8_t *a, long lda, const void *w, int w_bits, long M, long N,
                             long K_pad, const float *s_x_rows, const float *s_w, const float *bias,
                             const float *x0, const float *w0, void *out, int out_dtype, long ldo,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Same GEMM with TWO rank-1 epilogue terms, for the flag combinations whose integer evaluation needs the slot twice
 * (reference quant_utils.py:205-268 asymmetric activations, :367-376 split column, :446-509 asymmetric weights):
 *   y[m][n] = ((float(acc) * s_x[m]) * s_w[n]) + bias[n] + x0[m]*w0[n] + x1[m]*w1[n]      (one rounding per operation, in that order)
 * s_x[m] = s_x_rows[m] when s_x_rows is given (dynamic quantizers), else the static scale set(s) with row_sel.
 *   --w_asym + --visual_split:  (x[m][0], L1 weight)                       and (s_x sum_k a[m][k], s_w (2^(b-1) - z_w))
 *   --a_asym + --visual_split:  (x[m][0], L1 weight)                       and (s_x (2^(b-1) - z_x)[m], s_w sum_k q_w[n][k])
 *   --w_asym + --a_asym:        (s_x (2^(b-1) - z_x)[m], s_w (sum_k q_w[n][k] + K (2^(b-1) - z_w)))  and (s_x sum_k a[m][k], s_w (2^(b-1) - z_w))
 * (stored levels are q - 2^(bits-1) on an asymmetric side; goldens tests/golden/wrapper_rank2_*.npz from the reference's forward). */
int mq_gemm_w4a8_rank2_ws(const int8_t *a, long lda, const void *w, int w_bits, long M, long N, long K_pad,
                          float s_x0, float s_x1, const uint8_t *row_sel, const float *s_x_rows,
                          const float *s_w, const float *bias, const float *x0, const float *w0,
                          const float *x1, const float *w1, void *out, int out_dtype, long ldo,
                          void *workspace, size_t workspace_bytes, void *stream);

int mq_gemm_w4a8_i32(const int8_t *a, long lda, const void *w, int w_bits,
                     long M, long N, long K_pad, int32_t *acc, long ldacc, void *stream);

/* Same two entry points with a caller-owned scratch buffer, which lets the library split
 * the reduction over workgroups when M x N alone cannot fill the 256 CUs (e.g. down_proj:
 * K = 19968, N = 3584).  Partial sums are int32 and are combined in a fixed order, so the
 * result is bit-identical to the unsplit call.  workspace: 16-byte aligned device memory,
 * workspace_bytes >= 8 * M * N * 4 allows every split factor the heuristic may pick;
 * smaller buffers merely restrict it.  workspace == NULL degrades to the calls above. */
int mq_gemm_w4a8_ws(const int8_t *a, long lda, const void *w, int w_bits,
                    long M, long N, long K_pad,
                    float s_x0, float s_x1, const uint8_t *row_sel,
                    const float *s_w, const float *bias,
                    const float *x0, const float *w0,
                    void *out, int out_dtype, long ldo,
                    void *workspace, size_t workspace_bytes, void *stream);

int mq_gemm_w4a8_i32_ws(const int8_t *a, long lda, const void *w, int w_bits,
                        long M, long N, long K_pad, int32_t *acc, long ldacc,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Dynamic GROUP-WISE activation quantizer (--a_groupsize g; ActQuantizer.find_params_per_token_groupwise,
 * quant_utils.py:181-203, + sym_quant :46-50), symmetric: one scale per row and group of g consecutive channels,
 * scale = max(|amin * clip|, amax * clip) / maxq (1 for an all-zero group), no zero inclusion, every intermediate
 * rounded to x_dtype exactly like the reference's tensors of that dtype.  g: a power of two in 16..1024 dividing K;
 * K_pad must hold whole groups.  scales_out: fp32 [M, K / g].  out as for mq_quantize_act_i8 (row-major or tiled). */
int mq_quantize_act_group_i8(const void *x, int x_dtype, long M, long K, long ldx, int groupsize, int bits,
                             float clip_ratio, float *scales_out, int8_t *out, long K_pad, long ldo, void *stream);

/* The same with ASYMMETRIC levels (--a_groupsize g + --a_asym; the sym = False branch of quant_utils.py:181-203 + asym_quant
 * :27-31): per row and group  range = [amin, amax] * clip (0 need not be inside; (-1, +1) for an all-zero group),
 * scale = (xmax - xmin) / (2^bits - 1), zero = round(-xmin / scale), q = clamp(round(x / scale) + zero, 0, 2^bits - 1), every
 * intermediate rounded to x_dtype like the reference's tensors.  out holds q - 2^(bits-1); shift_out[m][g] = scale (2^(bits-1) -
 * zero) in fp32: x_hat = scale * out + shift.  zero_out may be NULL.  Pair with mq_gemm_w4a8_groupscale_asym. */
int mq_quantize_act_group_asym_i8(const void *x, int x_dtype, long M, long K, long ldx, int groupsize, int bits,
                                  float clip_ratio, float *scales_out, float *zero_out, float *shift_out, int8_t *out,
                                  long K_pad, long ldo, void *stream);

/* The GEMM for group-wise activation scales: y[m][n] = (sum_g (float(acc_g[m][n]) * s_x_groups[m][g])) * s_w[n] + bias[n],
 * acc_g = the exact int32 sum over the group's k, groups added in ascending order in fp32 (one rounding per group).
 * Replaces F.linear on the group-wise fake-quantized activations (quant_utils.py:384 after :181-203; the reference
 * accumulates s * q products in floating point in library order: outputs agree to the 1e-3 of the other modes).
 * group_k: 64 or a multiple of 128; n_groups * group_k covers K_pad up to its zero padding. */
int mq_gemm_w4a8_groupscale(const int8_t *a, long lda, const void *w, int w_bits, long M, long N, long K_pad,
                            const float *s_x_groups, long n_groups, int group_k, const float *s_w,
                            const float *bias, void *out, int out_dtype, long ldo, void *stream);

/* ... for asymmetric groups: y[m][n] = (sum_g (float(acc_g) * s_x_groups[m][g] + shift_groups[m][g] * wsum_groups[g][n])) * s_w[n] + bias[n],
 * wsum_groups[g * N + n] = sum_{k in group g} q_w[n][k] as fp32 (the constant part s (2^(b-1) - z) of a group's dequantised levels
 * meets the group's weight sum); the two products of a group are added to the fp32 accumulator in that order. */
int mq_gemm_w4a8_groupscale_asym(const int8_t *a, long lda, const void *w, int w_bits, long M, long N, long K_pad,
                                 const float *s_x_groups, const float *shift_groups, const float *wsum_groups,
                                 long n_groups, int group_k, const float *s_w, const float *bias, void *out,
                                 int out_dtype, long ldo, void *stream);

/* W4A8 Linear with the rotary position embedding of its q | k output columns folded into the store (the fused q|k|v projection of
 * a decoder layer).  NOT part of MQuant -- the reference never touches RoPE; it exists because the whole-prefill TTFT report chains
 * the Linears through the model's glue ("the step either side of the Linear").  Columns n < rope_cols are heads of
 * head_dim = 128 channels (one 128-wide output tile each, rope_cols % 128 == 0); cos / sin: [M, 128] in the output dtype, row = token
 * position.  Result = mq_gemm_w4a8 followed by mq_rope_inplace on the same columns, bit for bit:
 *   x = cast(linear output);  out = cast(cast(x * cos) + cast(rotate_half(x) * sin)),  rotate_half(x) = cat(-x[64:], x[:64]).
 * Needs tiled activations (lda = MQ_LD_TILED), a 16-bit output, N % 8 == 0; other head sizes: MQ_EUNSUPPORTED (run mq_rope_inplace). */
int mq_gemm_w4a8_rope_ws(const int8_t *a, long lda, const void *w, int w_bits, long M, long N, long K_pad, float s_x0, float s_x1,
                         const uint8_t *row_sel, const float *s_w, const float *bias, const void *rope_cos, const void *rope_sin,
                         long rope_cols, int head_dim, void *out, int out_dtype, long ldo, void *stream);

/* Activation of the CONSUMER folded into the GEMM's store (round 6).  The reference wraps every Linear on its own
 * (fake_quant/quant_utils.py:330-391); between two wrapped Linears the HF module applies its activation --
 * Qwen2MLP: down_proj(act_fn(gate_proj(x)) * up_proj(x)), the vision MLP: fc2(quick_gelu(fc1(x))) -- and the down_proj / fc2 wrapper
 * then reads that tensor (through the online Hadamard, fake_quant/hadamard_utils.py:115-128).  Here the producer GEMM stores the
 * ACTIVATED tensor: the Linear's output y is formed and rounded to out_dtype exactly as mq_gemm_w4a8_ws stores it, then
 *   act = MQ_ACT_SILU_MUL (1):   w is the image of a fused gate|up projection, gate = channels 0 .. N/2-1, up = N/2 .. N-1 (N / 2 a
 *                                multiple of 32); out[m][c] = cast(cast(silu(y[m][c])) * y[m][N/2 + c]) -- [M, N/2], ldo >= N/2
 *   act = MQ_ACT_QUICK_GELU (2): out[m][n] = cast(x * cast(sigmoid(cast(1.702 x)))), x = y[m][n] -- [M, N]
 * every torch op rounding once to out_dtype, as F.silu(gate) * up / QuickGELUActivation evaluate on tensors of that dtype (the same
 * device expf): bit-identical to mq_gemm_w4a8_ws followed by those torch ops.  Static scale set(s) (s_x0, s_x1, row_sel) or per-row
 * scales (s_x_rows); bias optional; no rank-1 terms.  Needs tiled activations (lda = MQ_LD_TILED: MQ_EUNSUPPORTED otherwise),
 * output columns and ldo multiples of 8, out 16-byte aligned. */
int mq_gemm_w4a8_act_ws(const int8_t *a, long lda, const void *w, int w_bits, long M, long N, long K_pad, float s_x0, float s_x1,
                        const uint8_t *row_sel, const float *s_x_rows, const float *s_w, const float *bias, int act,
                        void *out, int out_dtype, long ldo, void *stream);

/* out[m][n] = cast(y32[m][n] + x[m] * w[n]): a THIRD rank-1 term behind mq_gemm_w4a8_rank2_ws, for a layer that combines the split
 * column (--visual_split, quant_utils.py:367-376), asymmetric weights (--w_asym) and asymmetric dynamic activations (--a_asym): run
 * the two-slot GEMM with out_dtype = MQ_F32, then this pass -- the sum continues in fp32 and is rounded to the output dtype once,
 * exactly what a third epilogue slot would compute.  y32: fp32 [M, ldy]; out: [M, ldo] of out_dtype (may alias y32 for MQ_F32). */
int mq_rank1_add_cast(const float *y32, long M, long N, long ldy, const float *x, const float *w, void *out, int out_dtype,
                      long ldo, void *stream);

/* The GEMM for group-wise WEIGHT scales (--w_groupsize g; reference fake_quant/gptq/gptq_utils.py:263-273: the GPTQ solver re-runs
 * WeightQuantizer.find_params on every group of g consecutive input channels, so channel n carries one scale per group; flag at
 * exam/quant_qwen2vl.py:327).  s_w_groups[g * N + n] = that scale.
 *   y[m][n] = (sum_g ((float(acc_g[m][n]) * s_x_groups[m][g]) * s_w_groups[g][n])) * s_x(m) + bias[n]
 * acc_g = the exact int32 sum over the group's k; groups added in ascending order in fp32 (one rounding per product and per sum);
 * s_x(m) = s_x_rows[m] (dynamic per-token), or s_x1 where row_sel[m] else s_x0 (static, MSQ), or 1 when s_x_groups (group-wise
 * activation scales of the SAME group size, quant_utils.py:181-203; NULL otherwise: the factor is then 1 inside the sum).
 * Replaces F.linear on fake-quantized tensors (quant_utils.py:384): outputs agree with the reference to the 1e-3 of the other modes,
 * the per-group accumulators are exact.  group_k: 64 or a multiple of 128; n_groups * group_k covers K_pad up to its zero padding.
 * M <= 16 on tiled activations (int4 weights, N % 4 == 0, 16-byte aligned s_w_groups): the streaming kernel, same bits. */
int mq_gemm_w4a8_wgroupscale(const int8_t *a, long lda, const void *w, int w_bits, long M, long N, long K_pad,
                             const float *s_w_groups, long n_groups, int group_k, float s_x0, float s_x1,
                             const uint8_t *row_sel, const float *s_x_rows, const float *s_x_groups,
                             const float *bias, void *out, int out_dtype, long ldo, void *stream);

/* ... for ASYMMETRIC weight groups (--w_groupsize g --w_asym: the solver runs WeightQuantizer.find_params with sym = False on every
 * group, reference fake_quant/gptq/gptq_utils.py:263-275, fake_quant/quant_utils.py:446-509, asym_quant_dequant :27-40):
 *   W~[n][k] = s_g[n] (q - z_g[n]),  q in 0 .. 2^b - 1,  z_g[n] = round(-xmin / s) an integer in 0 .. 2^b - 1.
 * The image stores q - 2^(b-1) (as for per-channel --w_asym).  With the group's zero offset d_g[n] = 2^(b-1) - z_g[n]
 * (w_zero_offsets[g * N + n], int16: -7 .. 8 for int4, -127 .. 128 for int8) and the activation group sums r_g[m] = sum_{k in g} a[m][k]
 * (a_group_sums[m * n_groups + g], from mq_act_group_rowsum_i32 over the same levels)
 *   acc'_g[m][n] = acc_g[m][n] + d_g[n] r_g[m]            (exact integers: = sum_{k in g} a[m][k] (q - z))
 *   y[m][n] = (sum_g ((float(acc'_g) * s_x_groups[m][g]) * s_w_groups[g][n])) * s_x(m) + bias[n]
 * -- mq_gemm_w4a8_wgroupscale's formula with acc' in place of acc: the same ascending group order, roundings and s_x(m) cases.  Both
 * tables are required; int8 weights: groups of at most 512 (float(acc') stays exact), larger ones are MQ_EUNSUPPORTED.
 * M <= 16 on tiled activations (int4 weights, N % 4 == 0, 16-byte aligned s_w_groups, 8-byte aligned w_zero_offsets): the streaming
 * kernel, same bits. */
int mq_gemm_w4a8_wgroupscale_asym(const int8_t *a, long lda, const void *w, int w_bits, long M, long N, long K_pad,
                                  const float *s_w_groups, const int16_t *w_zero_offsets, const int32_t *a_group_sums,
                                  long n_groups, int group_k, float s_x0, float s_x1, const uint8_t *row_sel,
                                  const float *s_x_rows, const float *s_x_groups, const float *bias, void *out,
                                  int out_dtype, long ldo, void *stream);

/* The activation group sums of the call above: out[m * n_groups + g] = sum of a[m][g * group_k .. (g + 1) * group_k - 1], exact int32
 * (the row factor of the zero points of asymmetric weight groups, reference quant_utils.py:446-509 per group as gptq_utils.py:263-275
 * runs it).  a: [M, K_pad] int8 levels with lda bytes per row or lda = MQ_LD_TILED; group_k: 64 or a multiple of 128;
 * n_groups * group_k <= K_pad -- groups that lie in the zero padding sum to 0.  One launch. */
int mq_act_group_rowsum_i32(const int8_t *a, long lda, long M, long K_pad, int group_k, long n_groups, int32_t *out, void *stream);

/* Scaled row sums of the int8 activation levels, for ASYMMETRIC weights (--w_asym; WeightQuantizer with
 * sym = False, quant_utils.py:446-509).  With the weight levels stored as q - 2^(b-1) the fake-quantized
 * weight is s_w[n] (stored + 2^(b-1) - z_w[n]); the zero points come back through the rank-1 epilogue term
 *   x0[m] = s_x(m) * sum_k a[m][k]   (this function; s_x(m) as in the GEMM: s_x_rows[m], or s_x1 where
 *                                     row_sel[m], else s_x0)
 *   w0[n] = s_w[n] * (2^(b-1) - z_w[n])
 * of mq_gemm_w4a8 / _rowscale_ws.  a: [M, K_pad] int8 with lda bytes per row or lda = MQ_LD_TILED. */
int mq_act_rowsum_scaled(const int8_t *a, long lda, long M, long K_pad, float s_x0, float s_x1,
                         const uint8_t *row_sel, const float *s_x_rows, float *out, void *stream);

/* TEST-ONLY hook, not part of the drop-in surface: force the tile shape (-1 heuristic; ids as in
 * csrc/gemm_w4a8.hip dispatch_tile) and the split-K factor (0 heuristic; bits 8..15 of a positive value
 * force the number of m-groups of the XCD mapping, 0 = automatic) for the GEMM calls the CALLING THREAD
 * makes afterwards (thread-local state; other threads keep the heuristic). */
int mq_gemm_debug_force(int tile, int splits);
/* TEST-ONLY: the fused activations of the 16-bit dtypes (csrc/mq_common.h act_silu_16 / act_sigmoid_16 and the packed forms of the GEMM act
 * epilogues) against the reference forms (device expf + IEEE division, what torch's silu / sigmoid kernels execute), element by element:
 * which = 0 silu(x), 1 sigmoid(x), 2 silu(x) * u, 3 quick_gelu(x), 4 / 5 the packed two-at-a-time forms of 2 / 3.  in_bits / in2_bits /
 * out_*: n 16-bit patterns of dtype (MQ_F16 or MQ_BF16); in2_bits may be NULL (u = 1).  tests/test_gpu_act_exhaustive.py runs all 2^16 inputs. */
int mq_debug_act_table(int dtype, int which, const void *in_bits, const void *in2_bits, long n, void *out_fast, void *out_ref, void *stream);
/* TEST-ONLY: the plan (tile id, split-K factor) the dispatcher takes for a shape; host arithmetic only. */
int mq_gemm_debug_plan(long M, long N, long K_pad, int w_bits, int a_tiled, int have_workspace, int *tile, int *splits);
/* TEST-ONLY: the tile id a weight-group GEMM call takes (61 = the streaming kernel of gemm_skinny.hip; otherwise the id of the
 * tiled kernel, 26 = the round-1 kernel).  aligned: s_w_groups (and w_zero_offsets) meet the 16- / 8-byte alignment.
 * x_groups: the call carries s_x_groups.  asym: mq_gemm_w4a8_wgroupscale_asym.  Host arithmetic only (no device needed); honours
 * the calling thread's mq_gemm_debug_force: 61 = the streaming kernel wherever its requirements hold, a wave-specialised id or 26 =
 * the tiled kernels (asymmetric groups: 26 whatever wave-specialised id is forced). */
int mq_gemm_debug_group_plan(long M, long N, long K_pad, int w_bits, int a_tiled, int group_k, long n_groups,
                             int x_groups, int asym, int aligned, int *tile);

/* ---------------------------------------------------------------------------
 * Min/max observer reduction.  Replaces the two reductions of
 * MinmaxObserver.update, fake_quant/observer/minmax.py:13-28 (after
 * BaseObserver.reshape_tensor, observer/base.py:15-28): per-channel min and max of
 * x[M, C] over rows.  col_begin skips leading channels (split: the observer only
 * sees x[..., 1:], quant_utils.py:369).  Results are fp32 [C - col_begin].
 * mq_minmax_tensor reduces to two scalars (layer_wise): out2[0]=min, out2[1]=max.
 * ------------------------------------------------------------------------- */
int mq_minmax_channels(const void *x, int x_dtype, long M, long C, long ldx, long col_begin,
                       float *mn, float *mx, void *stream);
int mq_minmax_tensor(const void *x, int x_dtype, long M, long C, long ldx, long col_begin,
                     float *out2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MQUANT_HIP_H */
