// act_quant_dyn.hip -- the reference's DEFAULT activation quantizer: dynamic, symmetric, per token
// (ActQuantizer.find_params + forward, fake_quant/quant_utils.py:116-133,205-268 with
// act_per_tensor = False, groupsize = -1, sym = True), as int8 levels + one fp32 scale per row:
//     xmin = min(min_k x, 0) * clip;  xmax = max(max_k x, 0) * clip      (fp32: the `tmp` of :239
//     s    = max(|xmin|, xmax) / maxq,  s = 1 where that is 0              promotes half tensors)
//     q    = clamp(rint(x / s), -(maxq+1), maxq)
// One workgroup per row, the row stays in registers between the max pass and the quantize pass.
// skip_col0 (ActQuantWrapper.split, :367-372): column 0 is excluded from the range, comes back in
// x0_out as fp32 and gets level 0.
#include "act_quant_common.h"

namespace mq {

constexpr int DQ_THREADS = 256;
constexpr int DQ_MAX_CHUNKS = 8;   // rows up to 32768 elements

struct DqArgs {
    const void *x;
    long M, K, ldx;
    float clip, maxq;
    int skip_col0;
    float *x0_out, *scale_out;
    float *zero_out, *shift_out;   // asymmetric mode: zero point and scale * (2^(bits-1) - zero) per row
    float half;                    // asymmetric mode: 2^(bits-1), the offset of the stored levels
    const float *range_in;         // per-tensor mode: device [min, max] of the whole tensor (mq_minmax_tensor), else NULL
    int8_t *out;
    long K_pad, ldo;
    int vec_ok;
};

template <int DT, bool ASYM = false>
__global__ __launch_bounds__(DQ_THREADS) void act_quant_dyn_kernel(DqArgs p)
{
    kernarg_warm<sizeof(DqArgs)>();
    typedef typename Elem<DT>::T T;
    __shared__ float rmin[DQ_THREADS / 64], rmax[DQ_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long row = blockIdx.x;
    const T *xr = reinterpret_cast<const T *>(p.x) + row * p.ldx;
    const long chunks = ceil_div(p.K, 16);

    float v[DQ_MAX_CHUNKS][16];
    float mn = 0.0f, mx = 0.0f;
#pragma unroll
    for (int c = 0; c < DQ_MAX_CHUNKS; ++c) {
        const long ch = t + (long)c * DQ_THREADS;
        if (ch < chunks) {
            const long col = ch * 16;
            load_chunk16<DT>(xr + col, col, p.K, p.vec_ok, v[c]);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (p.skip_col0 && col + i == 0) continue;
                mn = fminf(mn, v[c][i]);
                mx = fmaxf(mx, v[c][i]);
            }
        }
    }
#pragma unroll
    for (int st = 1; st < 64; st <<= 1) {
        mn = fminf(mn, __shfl_xor(mn, st, 64));
        mx = fmaxf(mx, __shfl_xor(mx, st, 64));
    }
    if (lane == 0) { rmin[wave] = mn; rmax[wave] = mx; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < DQ_THREADS / 64; ++w) { mn = fminf(mn, rmin[w]); mx = fmaxf(mx, rmax[w]); }
    if (p.range_in) {                                   // act_per_tensor (quant_utils.py:214-237): one range for all rows
        mn = fminf(p.range_in[0], 0.0f);
        mx = fmaxf(p.range_in[1], 0.0f);
    }
    // The per-TENSOR rule is evaluated in x's dtype upstream (quant_utils.py:214-231: torch.tensor(0).to(x), the int64
    // maxq tensor does not promote): range * clip, the scale, the zero point, x / scale and the level sum are 16-bit
    // tensors for a half model, each torch op rounding its fp32 result once.  The per-token rule promotes to fp32 (:239).
    const bool faithful = (DT != MQ_F32) && p.range_in != nullptr;
    const QuantRange r = quant_range<DT, ASYM>(mn, mx, p.clip, p.maxq, faithful, /*each_bound=*/p.range_in != nullptr);
    if (t == 0) {
        if (p.scale_out) p.scale_out[row] = r.scale;
        if (ASYM) {                                     // quant_utils.py:255-268 + asym_quant :27-31
            if (p.zero_out) p.zero_out[row] = r.zero;
            if (p.shift_out) p.shift_out[row] = r.scale * (p.half - r.zero);
        }
    }

#pragma unroll
    for (int c = 0; c < DQ_MAX_CHUNKS; ++c) {
        const long ch = t + (long)c * DQ_THREADS;
        if (ch < chunks) {
            int q[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int lv = range_level<DT, ASYM>(v[c][i], r, p.half, faithful);
                q[i] = (ch * 16 + i < p.K) ? lv : 0;      // pad columns 0 (their weights are 0)
            }
            if (p.skip_col0 && ch == 0) {
                if (p.x0_out) p.x0_out[row] = v[c][0];
                q[0] = 0;
            }
            store_levels16(p.out, row, ch * 16, p.K_pad, p.ldo, q);
        }
    }
    zero_row_tail<DQ_THREADS>(p.out, row, chunks * 16, p.K_pad, p.ldo, t);
}

// The three per-token entry points after their own argument checks: the checks they share (in fn's name), the argument block,
// the launch.  asym: levels 0 .. 2^bits - 1 stored minus 2^(bits-1), zero points and shifts out; range_in: the per-tensor mode.
static int quantize_act_rows(const char *fn, const void *x, int x_dtype, long M, long K, long ldx, int bits, float clip_ratio, bool asym,
                             int skip_col0, const float *range_in, float *x0_out, float *scale_out, float *zero_out,
                             float *shift_out, int8_t *out, long K_pad, long ldo, void *stream)
{
    MQ_REQUIRE(bits >= 2 && bits <= 8, "%s: bits must be 2..8", fn);
    MQ_REQUIRE(K <= 16L * DQ_THREADS * DQ_MAX_CHUNKS, "%s: K=%ld too large (max %d)", fn, K, 16 * DQ_THREADS * DQ_MAX_CHUNKS);
    if (const int rc = check_act_dest(fn, out, K, K_pad, ldo)) return rc;
    DqArgs p;
    p.x = x; p.M = M; p.K = K; p.ldx = ldx; p.clip = clip_ratio;
    p.maxq = asym ? (float)((1 << bits) - 1) : (float)((1 << (bits - 1)) - 1);
    p.half = asym ? (float)(1 << (bits - 1)) : 0.0f;
    p.skip_col0 = skip_col0; p.x0_out = x0_out; p.scale_out = scale_out; p.zero_out = zero_out; p.shift_out = shift_out;
    p.range_in = range_in; p.out = out; p.K_pad = K_pad; p.ldo = ldo;
    p.vec_ok = rows_vec_ok(x, ldx, x_dtype);
    return with_dtype_asym(fn, x_dtype, asym, [&](auto dt, auto as) {
        hipLaunchKernelGGL((act_quant_dyn_kernel<decltype(dt)::value, decltype(as)::value>), dim3((unsigned)M), dim3(DQ_THREADS), 0,
                           (hipStream_t)stream, p);
        return check_launch(fn + 3);                    // the name without its mq_
    });
}

}  // namespace mq

extern "C" int mq_quantize_act_dyn_i8(const void *x, int x_dtype, long M, long K, long ldx, int bits,
                                      float clip_ratio, int skip_col0, float *x0_out, float *scale_out,
                                      int8_t *out, long K_pad, long ldo, void *stream)
{
    if (M == 0) return MQ_OK;                       // empty input: nothing to do (null pointers allowed)
    MQ_REQUIRE(x && out && scale_out && M >= 0 && K > 0 && ldx >= K, "mq_quantize_act_dyn_i8: bad shape");
    return mq::quantize_act_rows(__func__, x, x_dtype, M, K, ldx, bits, clip_ratio, false, skip_col0, nullptr, x0_out, scale_out,
                                 nullptr, nullptr, out, K_pad, ldo, stream);
}

/* Dynamic ASYMMETRIC per-token quantizer (--a_asym without --*_static; quant_utils.py:239-268 else-branch):
 *   scale = (xmax - xmin) / (2^bits - 1), zero = rint(-xmin / scale), q = clamp(rint(x / scale) + zero, 0, 2^bits - 1)
 * The int8 GEMM gets q - 2^(bits-1); shift_out[m] = scale * (2^(bits-1) - zero) is the row factor of the
 * rank-1 term that undoes the offset and the zero point: x_hat = scale * stored + shift, so
 *   y[m][n] = ((acc * scale[m]) * s_w[n]) + bias[n] + shift[m] * (s_w[n] * sum_k q_w[n][k])
 * (mq_gemm_w4a8_rowscale_ws with x0 = shift_out and w0 = s_w * column sums of the weight levels). */
extern "C" int mq_quantize_act_dyn_asym_i8(const void *x, int x_dtype, long M, long K, long ldx, int bits,
                                           float clip_ratio, float *scale_out, float *zero_out, float *shift_out,
                                           int8_t *out, long K_pad, long ldo, void *stream)
{
    if (M == 0) return MQ_OK;
    MQ_REQUIRE(x && out && scale_out && shift_out && M >= 0 && K > 0 && ldx >= K, "mq_quantize_act_dyn_asym_i8: bad shape");
    return mq::quantize_act_rows(__func__, x, x_dtype, M, K, ldx, bits, clip_ratio, true, 0, nullptr, nullptr, scale_out, zero_out,
                                 shift_out, out, K_pad, ldo, stream);
}

/* Dynamic PER-TENSOR quantizer (act_per_tensor = True; quant_utils.py:214-237): the range of the whole
 * tensor comes from mq_minmax_tensor (device [min, max], col_begin = 1 under skip_col0), so nothing
 * returns to the host.  Symmetric or asymmetric as above, except that the asymmetric rule replaces a
 * zero bound on its own (xmin == 0 -> -1; xmax == 0 -> +1).  scale_out / zero_out / shift_out are
 * written per row (all rows equal) for mq_gemm_w4a8_rowscale_ws. */
extern "C" int mq_quantize_act_range_i8(const void *x, int x_dtype, long M, long K, long ldx, int bits,
                                        float clip_ratio, int asym, int skip_col0, const float *minmax,
                                        float *x0_out, float *scale_out, float *zero_out, float *shift_out,
                                        int8_t *out, long K_pad, long ldo, void *stream)
{
    if (M == 0) return MQ_OK;
    MQ_REQUIRE(x && out && scale_out && minmax && M >= 0 && K > 0 && ldx >= K, "mq_quantize_act_range_i8: bad shape");
    MQ_REQUIRE(!asym || (shift_out && !skip_col0), "mq_quantize_act_range_i8: the asymmetric mode needs shift_out and no split column");
    return mq::quantize_act_rows(__func__, x, x_dtype, M, K, ldx, bits, clip_ratio, asym != 0, skip_col0, minmax, x0_out, scale_out,
                                 zero_out, shift_out, out, K_pad, ldo, stream);
}

/* Dynamic symmetric GROUP-WISE quantizer (--a_groupsize g; quant_utils.py:181-203 + sym_quant :46-50): one scale
 * per row and group of g consecutive channels,
 *     xmax = amax * clip; xmin = amin * clip (no zero inclusion); xmax = max(|xmin|, xmax)
 *     scale = xmax / maxq, 1 where xmax == 0;    q = clamp(rint(x / scale), -(maxq+1), maxq)
 * with every intermediate rounded to x's dtype like the reference's tensors of that dtype (amax * clip, the quotient
 * by maxq and x / scale are half tensors for a half model).  A thread owns 16 consecutive channels, the g / 16 lanes
 * of a group sit side by side in one wave and combine their extrema with shuffles.  scale_out: fp32 [M, K / g]. */
namespace mq {

struct GqArgs {
    const void *x;
    long M, K, ldx;
    int lanes_per_group;           // g / 16: 1 .. 64, a power of two
    float clip, maxq;
    float half = 0.0f;             // asymmetric levels: 2^(bits-1), maxq = 2^bits - 1
    float *scale_out;
    float *zero_out = nullptr, *shift_out = nullptr;
    long n_groups;
    int8_t *out;
    long K_pad, ldo;
    int vec_ok;
};

template <int DT, bool ASYM = false>
__global__ __launch_bounds__(256) void act_quant_group_kernel(GqArgs p)
{
    kernarg_warm<sizeof(GqArgs), true>();
    typedef typename Elem<DT>::T T;
    const long cpr = p.K_pad / 16;                                  // 16-channel chunks per row (a multiple of lanes_per_group)
    const long total = p.M * cpr;
    const long span = ((total + 63) / 64) * 64;                    // whole waves: every lane takes part in the shuffles
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < span; c += (long)gridDim.x * 256) {
        const bool live = c < total;
        const long cc = live ? c : total - 1;
        const long row = cc / cpr;
        const long col = (cc - row * cpr) * 16;
        float v[16];
        load_chunk16<DT>(reinterpret_cast<const T *>(p.x) + row * p.ldx + col, col, p.K, p.vec_ok, v);
        float mn = v[0], mx = v[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) { mn = fminf(mn, v[i]); mx = fmaxf(mx, v[i]); }
        for (int st = 1; st < p.lanes_per_group; st <<= 1) {
            mn = fminf(mn, __shfl_xor(mn, st, 64));
            mx = fmaxf(mx, __shfl_xor(mx, st, 64));
        }
        // sym = False: the range is [amin, amax] * clip (0 need not be inside), (-1, +1) when both are 0
        const QuantRange r = quant_range<DT, ASYM>(mn, mx, p.clip, p.maxq, /*round_dt=*/true, /*each_bound=*/false);
        if (!live) continue;
        const long chunk = cc - row * cpr;
        if ((chunk % p.lanes_per_group) == 0 && col < p.K) {
            const long gi = row * p.n_groups + chunk / p.lanes_per_group;
            p.scale_out[gi] = r.scale;
            if (ASYM) {
                if (p.zero_out) p.zero_out[gi] = r.zero;
                p.shift_out[gi] = r.scale * (p.half - r.zero);
            }
        }
        int q[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int lv = range_level<DT, ASYM>(v[i], r, p.half, true);
            q[i] = (col + i < p.K) ? lv : 0;
        }
        store_levels16(p.out, row, col, p.K_pad, p.ldo, q);
    }
}

static int quantize_act_group(const void *x, int x_dtype, long M, long K, long ldx, int groupsize, int bits, float clip_ratio,
                              bool asym, float *scale_out, float *zero_out, float *shift_out, int8_t *out, long K_pad, long ldo,
                              void *stream)
{
    const char *fn = "mq_quantize_act_group_i8";        // both entry points speak in the symmetric one's name
    if (M == 0) return MQ_OK;
    MQ_REQUIRE(x && out && scale_out && (!asym || shift_out) && M >= 0 && K > 0 && ldx >= K, "mq_quantize_act_group_i8: bad shape");
    MQ_REQUIRE(bits >= 2 && bits <= 8, "mq_quantize_act_group_i8: bits must be 2..8");
    MQ_REQUIRE(groupsize >= 16 && groupsize <= 1024 && (groupsize & (groupsize - 1)) == 0 && K % groupsize == 0,
               "mq_quantize_act_group_i8: groupsize=%d must be a power of two in 16..1024 that divides K=%ld", groupsize, K);
    if (const int rc = check_act_dest(fn, out, K, K_pad, ldo, "bad K_pad / ldo / alignment (K_pad must hold whole groups)", groupsize))
        return rc;
    GqArgs p;
    p.x = x; p.M = M; p.K = K; p.ldx = ldx; p.lanes_per_group = groupsize / 16; p.clip = clip_ratio;
    p.maxq = asym ? (float)((1 << bits) - 1) : (float)((1 << (bits - 1)) - 1);
    p.half = (float)(1 << (bits - 1));
    p.zero_out = zero_out; p.shift_out = shift_out;
    p.scale_out = scale_out; p.n_groups = K / groupsize; p.out = out; p.K_pad = K_pad; p.ldo = ldo;
    p.vec_ok = rows_vec_ok(x, ldx, x_dtype);
    long blocks = ceil_div(M * (K_pad / 16), 256);
    if (blocks > 256L * 16) blocks = 256L * 16;
    return with_dtype_asym(fn, x_dtype, asym, [&](auto dt, auto as) {
        hipLaunchKernelGGL((act_quant_group_kernel<decltype(dt)::value, decltype(as)::value>), dim3((unsigned)blocks), dim3(256), 0,
                           (hipStream_t)stream, p);
        return check_launch("quantize_act_group_i8");
    });
}

}  // namespace mq

extern "C" int mq_quantize_act_group_i8(const void *x, int x_dtype, long M, long K, long ldx, int groupsize, int bits,
                                        float clip_ratio, float *scale_out, int8_t *out, long K_pad, long ldo, void *stream)
{
    return mq::quantize_act_group(x, x_dtype, M, K, ldx, groupsize, bits, clip_ratio, false, scale_out, nullptr, nullptr, out, K_pad, ldo, stream);
}

extern "C" int mq_quantize_act_group_asym_i8(const void *x, int x_dtype, long M, long K, long ldx, int groupsize, int bits,
                                             float clip_ratio, float *scale_out, float *zero_out, float *shift_out, int8_t *out,
                                             long K_pad, long ldo, void *stream)
{
    return mq::quantize_act_group(x, x_dtype, M, K, ldx, groupsize, bits, clip_ratio, true, scale_out, zero_out, shift_out, out, K_pad, ldo, stream);
}
