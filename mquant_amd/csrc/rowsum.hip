// rowsum.hip -- scaled row sums of the int8 activation levels: the per-row factor of the rank-1 epilogue
// term that carries the zero points of ASYMMETRIC weights (--w_asym; WeightQuantizer with sym = False,
// fake_quant/quant_utils.py:446-509).  With stored weight levels q' = q - 2^(b-1) the fake-quantized
// weight is W~[n][k] = s_w[n] (q'[n][k] + 2^(b-1) - z_w[n]), so
//     y[m][n] = ((acc * s_x) * s_w[n]) + bias[n] + (s_x * sum_k a[m][k]) * (s_w[n] (2^(b-1) - z_w[n]))
// and the GEMM's x0 / w0 slot takes the two factors.  out[m] = s_x(m) * float(sum_k a[m][k]); the integer
// sum is exact, one rounding in the product.  One wave per row, 16 bytes per lane per access.
#include "act_quant_common.h"

namespace mq {

struct RsArgs {
    const int8_t *a;
    long M, K_pad, lda;
    float sx0, sx1;
    const uint8_t *row_sel;
    const float *sx_vec;
    float *out;
};

__global__ __launch_bounds__(256) void act_rowsum_kernel(RsArgs p)
{
    kernarg_warm<sizeof(RsArgs)>();
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.M) return;
    int acc = 0;
    for (long k = lane * 16L; k < p.K_pad; k += 64 * 16L) {
        const v4i v = *reinterpret_cast<const v4i *>(p.a + act_offset(row, k, p.K_pad, p.lda));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int w = v[j];
            acc += (int)(signed char)(w & 0xff) + (int)(signed char)((w >> 8) & 0xff) +
                   (int)(signed char)((w >> 16) & 0xff) + (w >> 24);
        }
    }
#pragma unroll
    for (int st = 1; st < 64; st <<= 1) acc += __shfl_xor(acc, st, 64);
    if (lane == 0) {
        float sx = p.sx0;
        if (p.sx_vec) sx = p.sx_vec[row];
        else if (p.row_sel && p.row_sel[row]) sx = p.sx1;
        p.out[row] = sx * (float)acc;
    }
}

// Group sums of the int8 activation levels, r_g[m] = sum_{k in g} a[m][k] as exact int32: the row factor of the integer correction
// d_g[n] r_g[m] that carries the zero points of ASYMMETRIC WEIGHT GROUPS (--w_groupsize g --w_asym; WeightQuantizer.find_params with
// sym = False per group, reference gptq/gptq_utils.py:263-275, quant_utils.py:446-509).  One wave per row, 16 bytes per lane per access;
// LPG = group_k / 16 lanes share a group.  POW2 (LPG a power of two <= 64: groups of 64 .. 1024): the wave reads 1024 consecutive
// levels at a time and every run of LPG lanes reduces its own group; otherwise the wave walks the row group by group.
struct GrsArgs {
    const int8_t *a;
    long M, K_pad, lda, n_groups;
    int group_k;
    int32_t *out;
};

__device__ __forceinline__ int sum_levels16(const v4i v)
{
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int w = v[j];
        acc += (int)(signed char)(w & 0xff) + (int)(signed char)((w >> 8) & 0xff) + (int)(signed char)((w >> 16) & 0xff) + (w >> 24);
    }
    return acc;
}

template <bool POW2>
__global__ __launch_bounds__(256) void act_group_rowsum_kernel(GrsArgs p)
{
    kernarg_warm<sizeof(GrsArgs)>();
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.M) return;                            // (whole waves leave: the shuffles below see full waves)
    const int lpg = p.group_k >> 4;
    int32_t *dst = p.out + row * p.n_groups;
    if (POW2) {
        for (long k0 = 0; k0 < p.K_pad; k0 += 1024) {
            const long k = k0 + lane * 16L;
            int acc = 0;
            if (k < p.K_pad) acc = sum_levels16(*reinterpret_cast<const v4i *>(p.a + act_offset(row, k, p.K_pad, p.lda)));
            for (int st = 1; st < lpg; st <<= 1) acc += __shfl_xor(acc, st, 64);
            const long g = k / p.group_k;
            if ((lane & (lpg - 1)) == 0 && k < p.K_pad && g < p.n_groups) dst[g] = acc;
        }
    } else {
        for (long g = 0; g < p.n_groups; ++g) {
            int acc = 0;
            for (int c = lane; c < lpg; c += 64)
                acc += sum_levels16(*reinterpret_cast<const v4i *>(p.a + act_offset(row, g * p.group_k + c * 16L, p.K_pad, p.lda)));
#pragma unroll
            for (int st = 1; st < 64; st <<= 1) acc += __shfl_xor(acc, st, 64);
            if (lane == 0) dst[g] = acc;
        }
    }
}

// out[m][n] = cast(y32[m][n] + x[m] * w[n]): the THIRD rank-1 term of a layer that uses the split column, asymmetric weights and
// asymmetric dynamic activations at once (the GEMM epilogue has two slots).  The GEMM runs with an fp32 output, so this pass
// continues the epilogue's sum in fp32 and rounds to the output dtype once -- the same arithmetic a third slot would do.
struct R1Args {
    const float *y;
    long M, N, ldy;
    const float *x, *w;
    void *out;
    long ldo;
};

template <int DT>
__global__ __launch_bounds__(256) void rank1_add_cast_kernel(R1Args p)
{
    kernarg_warm<sizeof(R1Args), true>();
    typedef typename Elem<DT>::T T;
    const long quads = (p.N + 3) / 4;
    const long total = p.M * quads;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / quads, n = (i - m * quads) * 4;
        const float xm = p.x[m];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (n + r >= p.N) break;
            const float pr = xm * p.w[n + r];
            const float v = p.y[m * p.ldy + n + r] + pr;
            reinterpret_cast<T *>(p.out)[m * p.ldo + n + r] = Elem<DT>::st(v);
        }
    }
}

}  // namespace mq

extern "C" int mq_rank1_add_cast(const float *y32, long M, long N, long ldy, const float *x, const float *w, void *out, int out_dtype,
                                 long ldo, void *stream)
{
    using namespace mq;
    if (M == 0 || N == 0) return MQ_OK;
    MQ_REQUIRE(y32 && x && w && out && M > 0 && N > 0 && ldy >= N && ldo >= N, "mq_rank1_add_cast: bad arguments");
    R1Args p{y32, M, N, ldy, x, w, out, ldo};
    long blocks = ceil_div(M * ((N + 3) / 4), 256);
    if (blocks > 4096) blocks = 4096;
    return with_dtype(__func__, out_dtype, [&](auto dt) {
        hipLaunchKernelGGL(rank1_add_cast_kernel<decltype(dt)::value>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
        return check_launch("rank1_add_cast");
    });
}

extern "C" int mq_act_group_rowsum_i32(const int8_t *a, long lda, long M, long K_pad, int group_k, long n_groups, int32_t *out, void *stream)
{
    using namespace mq;
    if (M == 0) return MQ_OK;
    MQ_REQUIRE(a && out && M > 0 && K_pad > 0 && ((uintptr_t)out) % 4 == 0, "mq_act_group_rowsum_i32: bad shape");
    if (const int rc = check_act_dest(__func__, a, K_pad, K_pad, lda, "bad lda / alignment")) return rc;
    MQ_REQUIRE(group_k == 64 || (group_k > 0 && group_k % 128 == 0), "mq_act_group_rowsum_i32: group size %d (64 or a multiple of 128)", group_k);
    MQ_REQUIRE(n_groups > 0 && n_groups * (long)group_k <= K_pad, "mq_act_group_rowsum_i32: %ld groups of %d exceed K_pad=%ld", n_groups, group_k, K_pad);
    GrsArgs p{a, M, K_pad, lda, n_groups, group_k, out};
    const bool pow2 = group_k <= 1024 && (group_k & (group_k - 1)) == 0;
    if (pow2) hipLaunchKernelGGL(act_group_rowsum_kernel<true>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(act_group_rowsum_kernel<false>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("act_group_rowsum_i32");
}

extern "C" int mq_act_rowsum_scaled(const int8_t *a, long lda, long M, long K_pad, float s_x0, float s_x1,
                                    const uint8_t *row_sel, const float *s_x_rows, float *out, void *stream)
{
    using namespace mq;
    if (M == 0) return MQ_OK;
    MQ_REQUIRE(a && out && M > 0 && K_pad > 0 && K_pad % 16 == 0, "mq_act_rowsum_scaled: bad shape");
    if (const int rc = check_act_dest(__func__, a, K_pad, K_pad, lda, "bad lda / alignment")) return rc;
    RsArgs p{a, M, K_pad, lda, s_x0, s_x1, row_sel, s_x_rows, out};
    hipLaunchKernelGGL(act_rowsum_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("act_rowsum_scaled");
}
