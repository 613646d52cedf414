// kv_append.hip -- the launch between the fused q|k|v projection and the decode attention of a generation step: rotate Q and K
// of the R new rows in place (rotate-half RoPE) and quantise K|V into rows [n - R, n) of the e4m3 cache, with n -- and an
// optional RoPE position offset -- read from DEVICE memory.  One launch where mq_rope_inplace and mq_kv_quant_fp8 were two, and
// neither of those can be captured once for a growing cache: both take their position from the host (a pointer into the tables,
// a pointer into the cache).  With this one a whole decode step is a linear graph that advances by incrementing one int32:
//
//     n = n_keys_dev ? clamp(*n_keys_dev, R, T) : T          the key count AFTER the append: what mq_attn_decode_fp8kv reads next
//     t = n - R + r                                          token (= cache row) of row r
//     p = clamp(t + (rope_delta_dev ? *rope_delta_dev : 0), 0, table_rows - 1)      row of the cos / sin tables
//
// The clamps are MEMORY SAFETY, not semantics: the host checks the buffers against R, T and table_rows, and whatever the two
// device integers hold, every access stays inside those buffers.  A caller that lets n leave [R, T] or p leave the tables gets
// a defined, wrong-position result instead of a fault.
//
// No reference counterpart (the reference neither rotates nor quantises a cache): the checkers are this library's own
// mq_rope_inplace and mq_kv_quant_fp8, bit for bit -- the arithmetic is theirs (kv_rope_common.h): the rotated value is
// rounded to the dtype, and that rounded value is what is divided by the head's scale.
//
// Element-wise and tiny (the 7B geometry at R = 8: 8 x 36 x 128 elements, nine workgroups): the cost is one dispatch, so the
// argument block is pulled in one round trip and the two device integers arrive through the vector memory path (a buffer load
// every lane of which receives the same dword), as in attn_decode.hip.  One lane = eight rotate-half pairs of a Q or K head
// (two 16-byte loads and stores; a K lane also stores two 8-byte groups of e4m3) or sixteen elements of a V head (two 16-byte
// loads, two 8-byte stores).  The grid depends on R, heads, kv_heads and head_dim only -- never on n.
//
// mq_kv_append_rope is the same launch for a 16-BIT cache (the reference's default k_bits = v_bits = 16; what mq_attn_decode
// reads): the store is the kernel's second template parameter KVB, the bytes of a cache element.  With KVB = 2 nothing is
// quantised -- cache row t receives the BITS of the rotated, rounded K heads and of the V heads -- and the lane-to-element map
// is the same: a K lane stores its two 16-byte pieces, a V lane its two.
//
// A BATCH of B sequences (mq_kv_append_rope_fp8_batch, mq_kv_append_rope_batch) is the second grid dimension: workgroup (x, b) is
// workgroup x of a single-sequence call on sequence b -- n from n_keys_dev[b], the offset from rope_delta_dev[b] (every sequence
// has its own image, hence its own offset), the qkv rows [b R, (b + 1) R) and the cache at kv + b * seq_stride.  The
// single-sequence entry points launch B = 1.
#include "kv_rope_common.h"

namespace mq {

struct KvAppendArgs {
    void *qkv;                 // [R][ldqkv]: per row `heads` Q heads, kv_heads K heads, kv_heads V heads
    const void *cos, *sin;     // [table_rows][head_dim], or both null: append only
    uint8_t *kv;               // cache: [T][ldkv] elements (e4m3 bytes, or qkv's dtype), per token the K heads, then the V heads
    const float *kv_scale;     // [2 * kv_heads]; null for a 16-bit cache
    const int32_t *n_dev;      // optional device-side key count (after the append)
    const int32_t *delta_dev;  // optional device-side RoPE position offset
    long T, ldqkv, ldkv, table_rows;
    int R, heads, kv_heads, head_dim;
    long seq_stride;           // a batch: elements between the caches of consecutive sequences (0 at B = 1)
};

template <int DT>
__device__ __forceinline__ v2i append_quant8(const v8us &x, float s)
{
    typedef typename Elem<DT>::T E;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = Elem<DT>::ld((E)x[e]);
    return kv_quant8_e4m3(v, s);
}

// eight elements of a cache row at element offset `at`: quantised to e4m3 with the head's scale, or their bits as they are
template <int DT, int KVB>
__device__ __forceinline__ void append_store8(uint8_t *crow, long at, const v8us &x, float s)
{
    if constexpr (KVB == 1) *reinterpret_cast<v2i *>(crow + at) = append_quant8<DT>(x, s);
    else *reinterpret_cast<v8us *>(crow + at * 2) = x;
}

template <int DT, int KVB>
__global__ __launch_bounds__(256) void kv_append_rope_kernel(KvAppendArgs p)
{
    kernarg_warm<sizeof(KvAppendArgs)>();
    typedef typename Elem<DT>::T E;
    const long b = blockIdx.y;                                        // the sequence of a batch (0 in a single-sequence call)
    long n = p.T, delta = 0;
    if (p.n_dev) {
        n = load_device_int(p.n_dev + b);
        n = n < p.R ? p.R : n;                                       // memory safety: rows [n - R, n) lie inside [0, T)
        n = n > p.T ? p.T : n;
    }
    if (p.delta_dev) delta = load_device_int(p.delta_dev + b);

    const unsigned gph = (unsigned)p.head_dim / 16;                   // lanes per head
    const unsigned per_row = (unsigned)(p.heads + 2 * p.kv_heads) * gph;
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (unsigned)p.R * per_row) return;
    const unsigned r = i / per_row, j = i - r * per_row;
    const unsigned hh = j / gph, g = j - hh * gph;                    // head of the row (Q, K, V in this order), lane of the head
    const long t = n - p.R + r;
    const int D = p.head_dim, half = D / 2, qk = p.heads + p.kv_heads;
    E *row = reinterpret_cast<E *>(p.qkv) + (b * p.R + r) * p.ldqkv;
    uint8_t *crow = p.kv + (b * p.seq_stride + t * p.ldkv) * KVB;

    if ((int)hh >= qk) {                                              // ---- V: sixteen consecutive elements, stored as they are
        const int vh = p.kv_heads + ((int)hh - qk);                   // head of the cache row
        const E *src = row + (long)hh * D + g * 16;
        const v8us x0 = *reinterpret_cast<const v8us *>(src), x1 = *reinterpret_cast<const v8us *>(src + 8);
        const float s = KVB == 1 ? p.kv_scale[vh] : 1.0f;
        const long at = (long)vh * D + g * 16;
        append_store8<DT, KVB>(crow, at, x0, s);
        append_store8<DT, KVB>(crow, at + 8, x1, s);
        return;
    }
    const bool rotate = p.cos != nullptr;
    if ((int)hh < p.heads && !rotate) return;                         // append only: Q stays as it is
    E *x = row + (long)hh * D + g * 8;
    v8us a8 = *reinterpret_cast<const v8us *>(x), b8 = *reinterpret_cast<const v8us *>(x + half);
    if (rotate) {
        long pos = t + delta;                                         // memory safety: the table row lies inside [0, table_rows)
        pos = pos < 0 ? 0 : pos;
        pos = pos > p.table_rows - 1 ? p.table_rows - 1 : pos;
        const E *ct = reinterpret_cast<const E *>(p.cos) + pos * D + g * 8, *st = reinterpret_cast<const E *>(p.sin) + pos * D + g * 8;
        const v8us c0 = *reinterpret_cast<const v8us *>(ct), c1 = *reinterpret_cast<const v8us *>(ct + half);
        const v8us s0 = *reinterpret_cast<const v8us *>(st), s1 = *reinterpret_cast<const v8us *>(st + half);
        v8us lo8, hi8;
        rope_pairs8<DT>(a8, b8, c0, c1, s0, s1, lo8, hi8);
        *reinterpret_cast<v8us *>(x) = lo8;
        *reinterpret_cast<v8us *>(x + half) = hi8;
        a8 = lo8;                                                     // the cache receives the ROUNDED rotated values
        b8 = hi8;
    }
    if ((int)hh >= p.heads) {                                         // ---- K: the two halves of the rotated head
        const int kh = (int)hh - p.heads;
        const float s = KVB == 1 ? p.kv_scale[kh] : 1.0f;
        const long at = (long)kh * D + g * 8;
        append_store8<DT, KVB>(crow, at, a8, s);
        append_store8<DT, KVB>(crow, at + half, b8, s);
    }
}

}  // namespace mq

// the checks and the launch of both entry points; kvb = bytes of a cache element: 1 = e4m3 with scales, 2 = qkv's dtype without
static int kv_append_run(const char *who, const char *kernel, int kvb, void *qkv, int dtype, int B, int R, long T, const int32_t *n_keys_dev,
                         const int32_t *rope_delta_dev, int heads, int kv_heads, int head_dim, long ldqkv, const void *cos, const void *sin,
                         long table_rows, void *kv_cache, long ldkv, long seq_stride, const float *kv_scale, void *stream)
{
    using namespace mq;
    MQ_REQUIRE(B >= 1 && B <= 65535, "%s: B = %d sequences (1 .. 65535: the second grid dimension)", who, B);
    MQ_REQUIRE(qkv && kv_cache && (kv_scale || kvb == 2), "%s: null pointer", who);
    MQ_REQUIRE(dtype == MQ_F16 || dtype == MQ_BF16, "%s: qkv dtype must be fp16 or bf16 (got %d)", who, dtype);
    MQ_REQUIRE(R >= 1 && R <= 8, "%s: R = %d new rows (1 .. 8)", who, R);
    MQ_REQUIRE(T >= R, "%s: T = %ld cache rows for R = %d new rows (the rows are the last R positions: T >= R)", who, T, R);
    MQ_REQUIRE(heads >= 1 && kv_heads >= 1 && heads % kv_heads == 0, "%s: bad head counts %d / %d", who, heads, kv_heads);
    MQ_REQUIRE(head_dim >= 16 && head_dim % 16 == 0, "%s: head_dim %d (a multiple of 16)", who, head_dim);
    const long cols = ((long)heads + 2L * kv_heads) * head_dim;
    MQ_REQUIRE(cols < (1L << 31) / 8, "%s: %ld columns per row exceed the grid", who, cols);
    MQ_REQUIRE(ldqkv >= cols, "%s: qkv row stride %ld shorter than (heads + 2 kv_heads) * head_dim = %ld", who, ldqkv, cols);
    MQ_REQUIRE(((uintptr_t)qkv) % 16 == 0 && (ldqkv * 2) % 16 == 0, "%s: qkv rows must be 16-byte aligned", who);
    MQ_REQUIRE(ldkv >= 2L * kv_heads * head_dim, "%s: cache row stride %ld shorter than 2 kv_heads * head_dim = %ld", who, ldkv, 2L * kv_heads * head_dim);
    const int align = 8 * kvb;                                         // of a lane's stores: eight cache elements
    MQ_REQUIRE(((uintptr_t)kv_cache) % align == 0 && ldkv % 8 == 0, "%s: cache rows must be %d-byte aligned", who, align);
    MQ_REQUIRE((cos == nullptr) == (sin == nullptr), "%s: cos and sin must both be given or both be null (append only)", who);
    if (cos) {
        MQ_REQUIRE(table_rows >= 1, "%s: table_rows = %ld (at least one row of cos / sin)", who, table_rows);
        MQ_REQUIRE(((uintptr_t)cos) % 16 == 0 && ((uintptr_t)sin) % 16 == 0, "%s: cos / sin tables must be 16-byte aligned", who);
    }
    MQ_REQUIRE(((uintptr_t)n_keys_dev) % 4 == 0, "%s: n_keys_dev must be 4-byte aligned", who);
    MQ_REQUIRE(((uintptr_t)rope_delta_dev) % 4 == 0, "%s: rope_delta_dev must be 4-byte aligned", who);

    if (B > 1) {                                                      // sequence b's cache: kv_cache + b * seq_stride (64-bit)
        MQ_REQUIRE(seq_stride >= T * ldkv, "%s: seq_stride %ld shorter than one sequence's T * ldkv = %ld elements", who, seq_stride, T * ldkv);
        MQ_REQUIRE((seq_stride * kvb) % 16 == 0, "%s: seq_stride must be a multiple of 16 bytes (got %ld bytes)", who, seq_stride * kvb);
    } else {
        seq_stride = 0;
    }

    KvAppendArgs a{qkv, cos, sin, reinterpret_cast<uint8_t *>(kv_cache), kv_scale, n_keys_dev, rope_delta_dev, T, ldqkv, ldkv, table_rows, R, heads, kv_heads,
                   head_dim, seq_stride};
    const unsigned lanes = (unsigned)(R * (cols / 16));
    const dim3 grid((lanes + 255) / 256, (unsigned)B);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (kvb == 1) {
        if (dtype == MQ_F16) hipLaunchKernelGGL((kv_append_rope_kernel<MQ_F16, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((kv_append_rope_kernel<MQ_BF16, 1>), grid, dim3(256), 0, st, a);
    } else {
        if (dtype == MQ_F16) hipLaunchKernelGGL((kv_append_rope_kernel<MQ_F16, 2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((kv_append_rope_kernel<MQ_BF16, 2>), grid, dim3(256), 0, st, a);
    }
    return check_launch(kernel);
}

extern "C" int mq_kv_append_rope_fp8(void *qkv, int dtype, int R, long T, const int32_t *n_keys_dev, const int32_t *rope_delta_dev,
                                     int heads, int kv_heads, int head_dim, long ldqkv, const void *cos, const void *sin, long table_rows,
                                     uint8_t *kv_cache, long ldkv, const float *kv_scale, void *stream)
{
    return kv_append_run("mq_kv_append_rope_fp8", "kv_append_rope_fp8", 1, qkv, dtype, 1, R, T, n_keys_dev, rope_delta_dev, heads, kv_heads, head_dim, ldqkv,
                         cos, sin, table_rows, kv_cache, ldkv, 0, kv_scale, stream);
}

extern "C" int mq_kv_append_rope(void *qkv, int dtype, int R, long T, const int32_t *n_keys_dev, const int32_t *rope_delta_dev, int heads,
                                 int kv_heads, int head_dim, long ldqkv, const void *cos, const void *sin, long table_rows, void *kv_cache,
                                 long ldkv, void *stream)
{
    return kv_append_run("mq_kv_append_rope", "kv_append_rope", 2, qkv, dtype, 1, R, T, n_keys_dev, rope_delta_dev, heads, kv_heads, head_dim, ldqkv, cos, sin,
                         table_rows, kv_cache, ldkv, 0, nullptr, stream);
}

// ---- the same two launches over a batch: B sequences of R rows each (qkv [B * R][ldqkv]), sequence b's cache at kv_cache +
// b * seq_stride elements, its key count at n_keys_dev[b], its offset at rope_delta_dev[b].  B = 1 is the sibling.
extern "C" int mq_kv_append_rope_fp8_batch(void *qkv, int dtype, int B, int R, long T, const int32_t *n_keys_dev, const int32_t *rope_delta_dev,
                                           int heads, int kv_heads, int head_dim, long ldqkv, const void *cos, const void *sin, long table_rows,
                                           uint8_t *kv_cache, long ldkv, long seq_stride, const float *kv_scale, void *stream)
{
    return kv_append_run("mq_kv_append_rope_fp8_batch", "kv_append_rope_fp8_batch", 1, qkv, dtype, B, R, T, n_keys_dev, rope_delta_dev, heads, kv_heads,
                         head_dim, ldqkv, cos, sin, table_rows, kv_cache, ldkv, seq_stride, kv_scale, stream);
}

extern "C" int mq_kv_append_rope_batch(void *qkv, int dtype, int B, int R, long T, const int32_t *n_keys_dev, const int32_t *rope_delta_dev,
                                       int heads, int kv_heads, int head_dim, long ldqkv, const void *cos, const void *sin, long table_rows,
                                       void *kv_cache, long ldkv, long seq_stride, void *stream)
{
    return kv_append_run("mq_kv_append_rope_batch", "kv_append_rope_batch", 2, qkv, dtype, B, R, T, n_keys_dev, rope_delta_dev, heads, kv_heads, head_dim,
                         ldqkv, cos, sin, table_rows, kv_cache, ldkv, seq_stride, nullptr, stream);
}
