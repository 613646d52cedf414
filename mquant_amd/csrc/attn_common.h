// attn_common.h -- what the attention kernels share (attn_prefill.hip, attn_decode.hip): the matrix-core instruction per
// dtype and the exact widening of e4m3 bytes to 16-bit operands.
#pragma once
#include "mq_common.h"

namespace mq {

typedef short at_v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) at_v4s at_lds_v4s;
typedef _Float16 at_v8h __attribute__((ext_vector_type(8)));
typedef __bf16 at_v8bf __attribute__((ext_vector_type(8)));
typedef float at_v16f __attribute__((ext_vector_type(16)));

template <int DT> struct AttnMma;
template <> struct AttnMma<MQ_F16> {
    static __device__ __forceinline__ at_v16f mma(v4i a, v4i b, at_v16f c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(at_v8h, a), __builtin_bit_cast(at_v8h, b), c, 0, 0, 0);
    }
};
template <> struct AttnMma<MQ_BF16> {
    static __device__ __forceinline__ at_v16f mma(v4i a, v4i b, at_v16f c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(at_v8bf, a), __builtin_bit_cast(at_v8bf, b), c, 0, 0, 0);
    }
};

template <int DT> struct AttnCvt;
typedef float at_v2f __attribute__((ext_vector_type(2)));
template <> struct AttnCvt<MQ_F16> {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ unsigned pack2(float a, float b) { return __builtin_bit_cast(unsigned, __builtin_convertvector(at_v2f{a, b}, h2)); }   // V_CVT_PK_F16_F32, RNE
    static __device__ __forceinline__ int lo(int w) { return __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false)); }
    static __device__ __forceinline__ int hi(int w) { return __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true)); }
};
template <> struct AttnCvt<MQ_BF16> {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ unsigned pack2(float a, float b) { return __builtin_bit_cast(unsigned, __builtin_convertvector(at_v2f{a, b}, b2)); }   // V_CVT_PK_BF16_F32, RNE
    static __device__ __forceinline__ int lo(int w) { return __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false)); }
    static __device__ __forceinline__ int hi(int w) { return __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true)); }
};

// sixteen e4m3 bytes -> two operands of eight 16-bit values (exact: e4m3 has 3 mantissa bits)
template <int DT>
__device__ __forceinline__ void widen16(const v4i w, v4i &a, v4i &b)
{
    a = v4i{AttnCvt<DT>::lo(w[0]), AttnCvt<DT>::hi(w[0]), AttnCvt<DT>::lo(w[1]), AttnCvt<DT>::hi(w[1])};
    b = v4i{AttnCvt<DT>::lo(w[2]), AttnCvt<DT>::hi(w[2]), AttnCvt<DT>::lo(w[3]), AttnCvt<DT>::hi(w[3])};
}

}  // namespace mq
