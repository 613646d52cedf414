// gemv_f16.hip -- out[m][n] = sum_k x[m][k] * W[n][k] for a handful of rows x (M <= 8) against a LARGE 16-bit matrix W:
// the unquantized lm_head on the last position of a prefill (the reference keeps lm_head in 16 bits: every exam/quant_*.py
// skips it, e.g. exam/quant_qwen2vl.py's skip list; HF computes logits = lm_head(hidden[:, -1:])).  152 064 x 3584 fp16 weights
// are 1.09 GB that are read once: an HBM stream, nothing else.  hipBLASLt's kernel for this shape moves them at 5.0 TB/s (219 us);
// this one at the rate the chip streams (guide: 6.3 TB/s copy, 6.5-6.8 with non-temporal loads).
//
//   * x ([M][K], a few KB) sits in LDS; a wave owns whole rows of W, four at a time (four independent 16-byte loads per lane
//     and step in flight), lane l takes the 16-byte chunks l, l + 64, ... of each row;
//   * products and sums in fp32 (V_DOT2_F32_F16 / fp32 FMA for bf16), one butterfly over the 64 lanes per output, one rounding
//     to the output dtype -- hipBLASLt's accumulation is fp32 as well, the summation ORDER differs (glue of the whole-prefill
//     report, not the W4A8 path: checked against an fp64 product with a half-precision tolerance, tests/test_gpu_gemv.py);
//   * rows are handed out wave by wave in one pass (grid = every wave slot of the chip), no tail round.
//
// mq_gemv_f16_argmax is the SAME kernel template with one more compile-time flag -- the same grid, row hand-out and summation
// order, so the same 16-bit logits bit for bit -- that also picks the greedy token on the device, the end of a captured
// generation step: the lane that stores (or, with logits == NULL, would store) y[m][n] folds the rounded bits and n into a
// running 64-bit key (argmax_key: a larger key is a better candidate), the wave's four row slots and then the workgroup's four
// waves meet (shuffles, LDS), the workgroup writes M keys to the workspace, and a second launch on the same stream takes the
// maximum over the workgroups.  The maximum of keys is associative and commutative: no atomics, no arrival counter, no "last
// workgroup merges" (attn_decode_merge_kernel), and equal inputs give equal tokens whatever order the workgroups ran in.
#include <type_traits>

#include "mq_common.h"

namespace mq {

struct GemvArgs {
    const void *x;      // [M][K], row stride ldx elements
    const void *w;      // [N][K], row stride ldw elements
    void *out;          // [M][N], row stride ldo elements
    long N, K, ldx, ldw, ldo;
    int M;
};

struct GemvArgmaxArgs : GemvArgs {                 // out may be null: no logits leave the chip
    unsigned long long *part;                      // [workgroups][M] keys
};

typedef _Float16 gv_h2 __attribute__((ext_vector_type(2)));

template <int DT>
__device__ __forceinline__ float dot8(const v4i a, const v4i b, float acc)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int aj = a[j], bj = b[j];      // (a bit_cast straight from a vector ELEMENT reads element 0: copy to a scalar first)
        if (DT == MQ_F16) {
            acc = __builtin_amdgcn_fdot2(__builtin_bit_cast(gv_h2, aj), __builtin_bit_cast(gv_h2, bj), acc, false);
        } else {
            const unsigned ua = (unsigned)aj, ub = (unsigned)bj;
            acc = fmaf(__uint_as_float(ua << 16), __uint_as_float(ub << 16), acc);
            acc = fmaf(__uint_as_float(ua & 0xffff0000u), __uint_as_float(ub & 0xffff0000u), acc);
        }
    }
    return acc;
}

constexpr int GV_ROWS = 4;      // rows of W a wave has in flight
constexpr int GV_THREADS = 256;

// The 16-bit logit h at index n as one key: the maximum over keys is torch.argmax's answer (IEEE comparison of the ROUNDED values,
// -0 == +0, every NaN maximal, among equals the lowest index).  High word: the value's rank (NaN 0x10000, else 0x8000 +- the
// magnitude bits: both zeros 0x8000, -inf 0x400 / 0x80), low word: 2^32 - 1 - n.  No key of a logit is 0: 0 is the neutral element.
template <int DT>
__device__ __forceinline__ unsigned long long argmax_key(unsigned h, long n)
{
    const unsigned mag = h & 0x7fffu, inf = DT == MQ_F16 ? 0x7c00u : 0x7f80u;
    const unsigned rank = mag > inf ? 0x10000u : (h & 0x8000u) ? 0x8000u - mag : 0x8000u + mag;
    return ((unsigned long long)rank << 32) | (0xffffffffu - (unsigned)n);
}
__device__ __forceinline__ unsigned long long key_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

template <int DT, int M, bool ARGMAX = false>
__global__ __launch_bounds__(GV_THREADS) void gemv_f16_kernel(std::conditional_t<ARGMAX, GemvArgmaxArgs, GemvArgs> p)
{
    kernarg_warm<sizeof(p), true>();
    extern __shared__ __attribute__((aligned(16))) char smem[];       // x: [M][K] 16-bit
    const int tid = threadIdx.x, lane = tid & 63;
    const long chunks = p.K / 8;
    for (int c = tid; c < (int)chunks * M; c += GV_THREADS) {
        const int m = c / (int)chunks, cc = c - m * (int)chunks;
        *reinterpret_cast<v4i *>(smem + ((long)m * p.K + cc * 8) * 2) =
            *reinterpret_cast<const v4i *>(reinterpret_cast<const unsigned short *>(p.x) + (long)m * p.ldx + cc * 8);
    }
    __syncthreads();
    const long wave = (long)blockIdx.x * (GV_THREADS / 64) + (tid >> 6), waves = (long)gridDim.x * (GV_THREADS / 64);
    const unsigned short *w = reinterpret_cast<const unsigned short *>(p.w);
    unsigned long long best = 0;                                      // ARGMAX: lane (m, r)'s running key over the wave's groups
    (void)best;
    for (long n0 = wave * GV_ROWS; n0 < p.N; n0 += waves * GV_ROWS) {
        float acc[GV_ROWS][M];
#pragma unroll
        for (int r = 0; r < GV_ROWS; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) acc[r][m] = 0.0f;
        // the last group of a matrix whose N is not a multiple of four re-reads its last row (never stored)
        const unsigned short *wr[GV_ROWS];
#pragma unroll
        for (int r = 0; r < GV_ROWS; ++r) wr[r] = w + (n0 + r < p.N ? n0 + r : p.N - 1) * p.ldw;
        for (long c = lane; c < chunks; c += 64) {
            v4i wv[GV_ROWS];
#pragma unroll
            for (int r = 0; r < GV_ROWS; ++r) wv[r] = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(wr[r] + c * 8));
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const v4i xv = *reinterpret_cast<const v4i *>(smem + ((long)m * p.K + c * 8) * 2);
#pragma unroll
                for (int r = 0; r < GV_ROWS; ++r) acc[r][m] = dot8<DT>(wv[r], xv, acc[r][m]);
            }
        }
#pragma unroll
        for (int r = 0; r < GV_ROWS; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) {
                float v = acc[r][m];
#pragma unroll
                for (int st = 1; st < 64; st <<= 1) v += __shfl_xor(v, st, 64);
                acc[r][m] = v;
            }
        if (lane < GV_ROWS * M) {                                     // lane (m, r) stores out[m][n0 + r]
            const int r = lane % GV_ROWS, m = lane / GV_ROWS;
            float v = 0.0f;
#pragma unroll
            for (int rr = 0; rr < GV_ROWS; ++rr)
#pragma unroll
                for (int mm = 0; mm < M; ++mm)
                    if (rr == r && mm == m) v = acc[rr][mm];
            if constexpr (!ARGMAX) {
                if (n0 + r < p.N)
                    reinterpret_cast<unsigned short *>(p.out)[(long)m * p.ldo + n0 + r] = (unsigned short)Elem<DT>::st(v);
            } else if (n0 + r < p.N) {                                // (the re-read last row never becomes a candidate)
                const unsigned short h = (unsigned short)Elem<DT>::st(v);
                if (p.out) reinterpret_cast<unsigned short *>(p.out)[(long)m * p.ldo + n0 + r] = h;
                best = key_max(best, argmax_key<DT>(h, n0 + r));
            }
        }
    }
    if constexpr (ARGMAX) {
        // lanes 4 m .. 4 m + 3 hold row m's four slots (the other lanes, and a wave that owned no rows, the neutral 0)
        best = key_max(best, __shfl_xor(best, 1, 64));
        best = key_max(best, __shfl_xor(best, 2, 64));
        __syncthreads();                                              // every wave is done with x: its LDS takes the waves' keys
        unsigned long long *red = reinterpret_cast<unsigned long long *>(smem);      // [4][M]; the launch sizes the LDS for it
        if (lane < GV_ROWS * M && lane % GV_ROWS == 0) red[(tid >> 6) * M + lane / GV_ROWS] = best;
        __syncthreads();
        if (tid < M)
            p.part[(long)blockIdx.x * M + tid] = key_max(key_max(red[tid], red[M + tid]), key_max(red[2 * M + tid], red[3 * M + tid]));
    }
}

// The second launch of mq_gemv_f16_argmax: workgroup m takes the maximum over the first launch's workgroups.
__global__ __launch_bounds__(256) void gemv_argmax_merge_kernel(const unsigned long long *part, int blocks, int M, int32_t *token_out)
{
    __shared__ unsigned long long red[4];
    const int m = blockIdx.x, tid = threadIdx.x;
    unsigned long long best = 0;
    for (int b = tid; b < blocks; b += 256) best = key_max(best, part[(long)b * M + m]);
#pragma unroll
    for (int st = 1; st < 64; st <<= 1) best = key_max(best, __shfl_xor(best, st, 64));
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) token_out[m] = (int32_t)(0xffffffffu - (unsigned)key_max(key_max(red[0], red[1]), key_max(red[2], red[3])));
}

}  // namespace mq

// every wave slot of the chip that the rows can fill: 8 workgroups of 4 waves per CU
static long gemv_blocks(long N, int cus)
{
    using namespace mq;
    const long blocks = (long)cus * 8, need = ceil_div(ceil_div(N, GV_ROWS), GV_THREADS / 64);
    return blocks > need ? need : blocks;
}

template <int DT, bool ARGMAX, typename Args>
static void gemv_launch(const Args &a, long blocks, hipStream_t st)
{
    using namespace mq;
    size_t lds = (size_t)a.M * a.K * 2;
    if (ARGMAX && lds < (size_t)a.M * 32) lds = (size_t)a.M * 32;     // the four waves' keys take x's place
    const dim3 grid((unsigned)blocks), block(GV_THREADS);
    switch (a.M) {
    case 1: hipLaunchKernelGGL((gemv_f16_kernel<DT, 1, ARGMAX>), grid, block, lds, st, a); break;
    case 2: hipLaunchKernelGGL((gemv_f16_kernel<DT, 2, ARGMAX>), grid, block, lds, st, a); break;
    case 3: hipLaunchKernelGGL((gemv_f16_kernel<DT, 3, ARGMAX>), grid, block, lds, st, a); break;
    case 4: hipLaunchKernelGGL((gemv_f16_kernel<DT, 4, ARGMAX>), grid, block, lds, st, a); break;
    case 5: hipLaunchKernelGGL((gemv_f16_kernel<DT, 5, ARGMAX>), grid, block, lds, st, a); break;
    case 6: hipLaunchKernelGGL((gemv_f16_kernel<DT, 6, ARGMAX>), grid, block, lds, st, a); break;
    case 7: hipLaunchKernelGGL((gemv_f16_kernel<DT, 7, ARGMAX>), grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL((gemv_f16_kernel<DT, 8, ARGMAX>), grid, block, lds, st, a); break;
    }
}

// What the two entry points check alike.  MQ_OK for M == 0 or N == 0 too: the caller decides what an empty call means.
static int gemv_check(const char *who, const void *x, int dtype, int M, long K, long ldx, const void *w, long N, long ldw, const void *out,
                      bool out_optional, long ldo)
{
    MQ_REQUIRE(dtype == MQ_F16 || dtype == MQ_BF16, "%s: dtype must be fp16 or bf16 (got %d)", who, dtype);
    MQ_REQUIRE(M >= 0 && M <= 8 && N >= 0 && K > 0 && K % 8 == 0, "%s: M must be 0..8 and K a positive multiple of 8 (M %d, N %ld, K %ld)", who, M, N, K);
    if (M == 0 || N == 0) return MQ_OK;
    MQ_REQUIRE(x && w && (out || out_optional), "%s: null pointer", who);
    MQ_REQUIRE(ldx >= K && ldw >= K && (!out || ldo >= N), "%s: row strides too short", who);
    MQ_REQUIRE(((uintptr_t)x) % 16 == 0 && (ldx * 2) % 16 == 0 && ((uintptr_t)w) % 16 == 0 && (ldw * 2) % 16 == 0,
               "%s: x / W rows must be 16-byte aligned", who);
    MQ_REQUIRE((long)M * K * 2 <= 64 * 1024, "%s: x (%d x %ld) must fit 64 KiB of LDS", who, M, K);
    return MQ_OK;
}

extern "C" int mq_gemv_f16(const void *x, int dtype, int M, long K, long ldx, const void *w, long N, long ldw, void *out, long ldo,
                           void *stream)
{
    using namespace mq;
    const int rc = gemv_check("mq_gemv_f16", x, dtype, M, K, ldx, w, N, ldw, out, false, ldo);
    if (rc != MQ_OK || M == 0 || N == 0) return rc;
    GemvArgs a{x, w, out, N, K, ldx, ldw, ldo, M};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long blocks = gemv_blocks(N, device_cu_count());
    if (dtype == MQ_F16) gemv_launch<MQ_F16, false>(a, blocks, st);
    else gemv_launch<MQ_BF16, false>(a, blocks, st);
    return check_launch("gemv_f16");
}

// N columns an int32 token can name
static bool gemv_argmax_columns_ok(long N) { return N >= 1 && N <= 0x7fffffffL; }

extern "C" size_t mq_gemv_argmax_workspace_bytes(int M, long N)
{
    if (M < 1 || M > 8 || !gemv_argmax_columns_ok(N)) return 0;
    return ((size_t)gemv_blocks(N, mq::device_cu_count()) * M * 8 + 15) / 16 * 16;
}

extern "C" int mq_gemv_f16_argmax(const void *x, int dtype, int M, long K, long ldx, const void *w, long N, long ldw, void *logits, long ldo,
                                  int32_t *token_out, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace mq;
    const char *who = "mq_gemv_f16_argmax";
    const int rc = gemv_check(who, x, dtype, M, K, ldx, w, N, ldw, logits, true, ldo);
    if (rc != MQ_OK) return rc;
    MQ_REQUIRE(gemv_argmax_columns_ok(N), "%s: N = %ld columns (1 .. 2^31 - 1: an argmax over nothing has no token, and the token is an int32)", who, N);
    if (M == 0) return MQ_OK;
    MQ_REQUIRE(token_out, "%s: token_out is null", who);
    MQ_REQUIRE(((uintptr_t)token_out) % 4 == 0, "%s: token_out must be 4-byte aligned", who);
    const size_t need = mq_gemv_argmax_workspace_bytes(M, N);
    MQ_REQUIRE(workspace, "%s: workspace is null (%zu bytes needed)", who, need);
    MQ_REQUIRE(((uintptr_t)workspace) % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    MQ_REQUIRE(workspace_bytes >= need, "%s: the workspace needs %zu bytes (got %zu)", who, need, workspace_bytes);
    const long blocks = gemv_blocks(N, device_cu_count());
    GemvArgmaxArgs a{{x, w, logits, N, K, ldx, ldw, ldo, M}, reinterpret_cast<unsigned long long *>(workspace)};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MQ_F16) gemv_launch<MQ_F16, true>(a, blocks, st);
    else gemv_launch<MQ_BF16, true>(a, blocks, st);
    const int lrc = check_launch("gemv_f16_argmax");
    if (lrc != MQ_OK) return lrc;
    hipLaunchKernelGGL(gemv_argmax_merge_kernel, dim3((unsigned)M), dim3(256), 0, st, a.part, (int)blocks, M, token_out);
    return check_launch("gemv_argmax_merge");
}
