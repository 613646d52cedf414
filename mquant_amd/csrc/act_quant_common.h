// act_quant_common.h -- what the activation quantizers share (act_quant.hip, act_quant_dyn.hip, rmsn_quant.hip; rowsum.hip and
// minmax.hip use the host half): the 16-channel row load, the pack of 16 levels into one 16-byte store, the zero tail of a row,
// the range rule of the dynamic quantizers, and on the host the destination check, the row-alignment rule and the dtype dispatch.
// A new quantizer variant is a new caller of these pieces, not a new copy of them.
#pragma once
#include <type_traits>

#include "mq_common.h"

namespace mq {

// ---- device: load ---------------------------------------------------------------------------------------------------------
// Channels col .. col + 15 of a row as fp32; src points at channel col.  A whole chunk of a row whose base and stride are
// multiples of 16 bytes (vec_ok, rows_vec_ok below) takes 16-byte loads; a chunk that crosses K or a misaligned row is read
// element by element, channels from K on as 0.  TAIL = false: the caller has refused everything but whole aligned chunks
// (rmsn_quant.hip), the element path does not exist.
template <int DT, bool TAIL = true>
__device__ __forceinline__ void load_chunk16(const typename Elem<DT>::T *src, long col, long K, int vec_ok, float (&v)[16])
{
    typedef typename Elem<DT>::T T;
    if (!TAIL || (col + 16 <= K && vec_ok)) {
        if (sizeof(T) == 2) {
            const v8us a = *reinterpret_cast<const v8us *>(src);
            const v8us b = *reinterpret_cast<const v8us *>(src + 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                v[i] = Elem<DT>::ld((T)a[i]);
                v[8 + i] = Elem<DT>::ld((T)b[i]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const v4f a = *reinterpret_cast<const v4f *>((const float *)src + 4 * j);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[4 * j + i] = a[i];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = (col + i < K) ? Elem<DT>::ld(src[i]) : 0.0f;
    }
}

// ---- device: store --------------------------------------------------------------------------------------------------------
// 16 levels -> the 16 bytes of channels col .. col + 15 (col % 16 == 0) of the int8 image, either layout (act_offset).
__device__ __forceinline__ void store_levels16(int8_t *out, long row, long col, long K_pad, long ldo, const int (&q)[16])
{
    v4i pk;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        pk[j] = (q[4 * j] & 0xff) | ((q[4 * j + 1] & 0xff) << 8) | ((q[4 * j + 2] & 0xff) << 16) | ((q[4 * j + 3] & 0xff) << 24);
    *reinterpret_cast<v4i *>(out + act_offset(row, col, K_pad, ldo)) = pk;
}

// Zero channels K_end .. K_pad (K_end % 16 == 0) of a row that a workgroup of THREADS threads owns; t = threadIdx.x.  The GEMM
// reads whole 128-byte k-steps.
template <int THREADS>
__device__ __forceinline__ void zero_row_tail(int8_t *out, long row, long K_end, long K_pad, long ldo, int t)
{
    for (long k = K_end + t * 16L; k < K_pad; k += THREADS * 16L)
        *reinterpret_cast<v4i *>(out + act_offset(row, k, K_pad, ldo)) = v4i{0, 0, 0, 0};
}

// ---- device: the range rule of the dynamic quantizers (fake_quant/quant_utils.py:181-268) ----------------------------------
//   symmetric:   s = max(|xmin|, xmax) / maxq, 1 where that is 0;            q = clamp(rint(x / s), -(maxq + 1), maxq)
//   asymmetric:  s = (xmax - xmin) / maxq, zero = rint(-xmin / s);           q = clamp(rint(x / s) + zero, 0, maxq), stored - half
// with (xmin, xmax) = (mn, mx) * clip.  round_dt: the reference evaluates the rule on tensors of x's dtype (group-wise and
// per-tensor modes), every torch op rounding its fp32 result once; the per-token mode promotes to fp32.  An empty asymmetric
// range becomes (-1, +1); each_bound: the per-tensor rule replaces a zero bound on its own (:229-232) instead.
struct QuantRange {
    float scale, zero, lo, hi;
};

template <int DT, bool ASYM>
__device__ __forceinline__ QuantRange quant_range(float mn, float mx, float clip, float maxq, bool round_dt, bool each_bound)
{
    auto rd = [&](float f) { return round_dt ? Elem<DT>::rnd(f) : f; };
    float xmin = rd(mn * clip), xmax = rd(mx * clip);
    QuantRange r;
    if (ASYM) {
        if (each_bound) {
            if (xmin == 0.0f) xmin = -1.0f;
            if (xmax == 0.0f) xmax = 1.0f;
        } else if (xmin == 0.0f && xmax == 0.0f) {
            xmin = -1.0f;
            xmax = 1.0f;
        }
        r.scale = rd(rd(xmax - xmin) / maxq);
        r.zero = rintf(rd(-xmin / r.scale));
        r.lo = 0.0f;
    } else {
        xmax = fmaxf(fabsf(xmin), xmax);
        r.scale = (xmax == 0.0f) ? 1.0f : rd(xmax / maxq);
        r.zero = 0.0f;
        r.lo = -(maxq + 1.0f);
    }
    r.hi = maxq;
    return r;
}

// The stored level of x under r; half = 2^(bits-1) for the asymmetric levels (the int8 GEMM takes q - half).
template <int DT, bool ASYM>
__device__ __forceinline__ int range_level(float x, const QuantRange &r, float half, bool round_dt)
{
    auto rd = [&](float f) { return round_dt ? Elem<DT>::rnd(f) : f; };
    float lv = rintf(rd(x / r.scale));
    if (ASYM) lv = rd(lv + r.zero);
    lv = fminf(fmaxf(lv, r.lo), r.hi);
    return ASYM ? (int)(lv - half) : (int)lv;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// Rows that the 16-byte loads can read: base and row stride multiples of 16 bytes.
inline bool rows_vec_ok(const void *x, long ldx, int x_dtype)
{
    return ((uintptr_t)x) % 16 == 0 && (ldx * (x_dtype == MQ_F32 ? 4 : 2)) % 16 == 0;
}

// An int8 image that takes 16-byte stores through act_offset: 16-byte aligned, K_pad >= K a multiple of 16 (of `granule`, for a
// caller that needs more), row-major with ldo >= K_pad a multiple of 16 or tiled with whole 64-channel pieces.  fn: the entry
// point's own name; what: its own words for this refusal.
inline int check_act_dest(const char *fn, const void *out, long K, long K_pad, long ldo, const char *what = "bad K_pad / ldo / alignment",
                          long granule = 16)
{
    if (K_pad >= K && K_pad % granule == 0 && ((uintptr_t)out) % 16 == 0 &&
        (ldo == MQ_LD_TILED ? K_pad % 64 == 0 : (ldo >= K_pad && ldo % 16 == 0)))
        return MQ_OK;
    return fail(MQ_EINVAL, "%s: %s", fn, what);
}

// f(std::integral_constant<int, dtype>) for the three activation dtypes; anything else is refused in fn's name.
template <typename F>
static int with_dtype(const char *fn, int dtype, F f)
{
    switch (dtype) {
    case MQ_F16: return f(std::integral_constant<int, MQ_F16>{});
    case MQ_BF16: return f(std::integral_constant<int, MQ_BF16>{});
    case MQ_F32: return f(std::integral_constant<int, MQ_F32>{});
    }
    return fail(MQ_EINVAL, "%s: unknown dtype %d", fn, dtype);
}

// The same crossed with the asymmetric switch of the dynamic quantizers: f(dtype constant, std::bool_constant<asym>).
template <typename F>
static int with_dtype_asym(const char *fn, int dtype, bool asym, F f)
{
    return with_dtype(fn, dtype, [&](auto dt) { return asym ? f(dt, std::true_type{}) : f(dt, std::false_type{}); });
}

}  // namespace mq
