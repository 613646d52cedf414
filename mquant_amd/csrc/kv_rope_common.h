// kv_rope_common.h -- the two element-wise expressions that rope.hip, kv_fp8.hip and kv_append.hip must evaluate identically:
// the rotate-half pair and the e4m3 quantise step.  kv_append.hip promises the BITS of mq_rope_inplace followed by
// mq_kv_quant_fp8, so the three files share the text instead of restating it.
#pragma once
#include "mq_common.h"

namespace mq {

// One rotate-half pair (a = x[d], b = x[d + head_dim / 2]) with the HF formula's roundings: every product and the sum round to DT.
template <int DT>
__device__ __forceinline__ void rope_pair(float a, float b, float c0, float c1, float s0, float s1, float &lo, float &hi)
{
    lo = Elem<DT>::rnd(a * c0) + Elem<DT>::rnd(-b * s0);
    hi = Elem<DT>::rnd(b * c1) + Elem<DT>::rnd(a * s1);
}

// Eight pairs of a 16-bit dtype: a8 / b8 the two halves of the head, c0 / s0 and c1 / s1 the table entries at d and d + half.
template <int DT>
__device__ __forceinline__ void rope_pairs8(const v8us &a8, const v8us &b8, const v8us &c0, const v8us &c1, const v8us &s0, const v8us &s1,
                                            v8us &lo8, v8us &hi8)
{
    typedef typename Elem<DT>::T E;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float lo, hi;
        rope_pair<DT>(Elem<DT>::ld((E)a8[e]), Elem<DT>::ld((E)b8[e]), Elem<DT>::ld((E)c0[e]), Elem<DT>::ld((E)c1[e]), Elem<DT>::ld((E)s0[e]),
                      Elem<DT>::ld((E)s1[e]), lo, hi);
        lo8[e] = (unsigned short)Elem<DT>::st(lo);
        hi8[e] = (unsigned short)Elem<DT>::st(hi);
    }
}

// Eight values -> eight e4m3fn bytes (element e in byte e & 3 of word e >> 2): true division by the head's scale, clamp to
// +-448 in front of the conversion (the result then does not depend on its overflow mode), V_CVT_PK_FP8_F32.
__device__ __forceinline__ v2i kv_quant8_e4m3(const float (&v)[8], float s)
{
    float q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float t = v[e] / s;
        t = fminf(fmaxf(t, -448.0f), 448.0f);
        q[e] = t;
    }
    int w0 = 0, w1 = 0;
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], w0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], w1, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], w1, true);
    return v2i{w0, w1};
}

}  // namespace mq
