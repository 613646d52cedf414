// attn_decode.hip -- decode attention: R <= 8 query rows (the last positions of a sequence) over the first n keys of the fp8
// (OCP e4m3fn) KV cache, read DIRECTLY: one byte per element leaves HBM, the bytes are widened inside the kernel, and no
// dequantised copy of the cache exists anywhere (BASELINE configuration 5).  The generation-step counterpart of
// mq_attn_prefill_fp8kv (attn_prefill.hip), with that kernel's arithmetic:
//
//     S[m][k] = (sum_d Q[m][d] * K8[k][d]) * s_k[kvh] * softmax_scale          (causal: k <= n - R + row of m)
//     O[m][d] = (sum_k softmax_k(S)[m][k] * V8[k][d]) * s_v[kvh]
//
// the matrix core multiplies the e4m3 VALUES (exact in fp16 / bf16), the K scale, softmax_scale and log2(e) are ONE fp32 score
// factor, P is packed to q's dtype against the running maximum, everything accumulates in fp32, and the V scale and 1 / L meet
// the result in one product that is rounded once at the store.  The reference has no attention kernel and no cache quantizer:
// PARITY UNPINNED -- the checker is float64 softmax attention over the dequantised cache with a bound per output element
// (tests/attn_decode_reference.py, the formula of tests/attn_reference.py evaluated for R rows over n keys).
//
// What is different from a prefill is the SHAPE: one query row per head.  The prefill grid would be `heads` workgroups on 256
// CUs, and every query head of a GQA group would fetch the same cache bytes again.  Here
//   * one workgroup = one (kv head, key split).  The rep = heads / kv_heads query heads that share the kv head, times the R rows,
//     are the M dimension of both GEMMs (m = row * rep + head-in-group): a cache byte is fetched once per kv head.  A pass serves
//     AD_M = 16 such rows (the generation step of both Qwen2-VL geometries: rep 7 and 8 at R = 1); more take further passes over
//     the same keys inside the workgroup -- the keys are then read again, from L2 at best: correct first, R * rep > 16 is not the
//     generation step;
//   * the keys [0, n) are cut into `splits` contiguous ranges of keys_per_split (a multiple of the 32-key block), chosen on the
//     host so that kv_heads x splits workgroups fill the chip (attn_decode_plan); inside a workgroup the four waves take the
//     range's blocks w, w + 4, ... with running statistics of their own and merge through LDS, as in the prefill kernel;
//   * splits == 1: the workgroup stores the result.  splits > 1: it writes ONE partial state per (row, head) -- m (log2 domain),
//     l and the unnormalised acc[128] -- into the caller's fp32 workspace, and a second, small launch on the same stream merges
//     the splits IN INDEX ORDER (M = max m_s, w_s = exp2(m_s - M), O = s_v sum w_s acc_s / sum w_s l_s) and stores.  Workgroups
//     never talk to each other inside a launch: no arrival counters, no polling, no "last workgroup merges" -- the second
//     launch costs about a dispatch gap, is deterministic by construction and cannot hang;
//   * the key count may live on the DEVICE (n_keys_dev): n = clamp(*n_keys_dev, R, T), loaded through the vector memory path by
//     both launches, so a generation loop is captured once and replayed while the cache grows.  T is then the capacity the plan
//     and the grid are sized for; a split that starts at or beyond n leaves at once, writes nothing, and the merge does not
//     read its slot -- whatever the workspace held before the call cannot reach the output.
// K / V arrive as in the prefill kernel: a key's K row of one kv head is one 128-byte line, its V row another (kv_heads * 128
// bytes on); a lane loads whole 16-byte pieces straight into registers through buffer descriptors that END AT KEY n - 1, so a
// row at or beyond n comes back as zeros from the hardware's range check whatever it holds (a 0x7F byte is a NaN, and 0 x NaN
// would be one too); the next block is in flight while the current one is multiplied.  S is computed transposed (lane = M row),
// so the softmax statistics are lane-local; columns 16 .. 31 of the 32-wide tile carry zero queries and are never stored.
//
// The same kernel serves a 16-BIT cache (mq_attn_decode, mq_attn_decode_quant_i8: the reference's default k_bits = v_bits = 16):
// the storage is the kernel's second template parameter KVB, the bytes of a cache element.  KVB = 2 is the layout above at two
// bytes per element in q's dtype, and only the LOAD side differs: a lane's K piece is 128 contiguous bytes -- eight 16-byte
// loads that ARE the eight MFMA operands -- its V piece another 128 that go to the LDS tile where widen16 puts the same values,
// and there are no scales: the score and output factors are the expressions above with both scales 1.0f, so the two storages
// give equal bits on equal values.  Everything after the loads is the same source.  What is in flight differs: sixteen 16-byte
// loads per lane next to the eight K operands in use do not fit the 256 registers of two workgroups per CU, so the 16-bit path
// prefetches the next block's K only (issued once S has consumed the operands, in flight during the softmax and P V) and
// loads the CURRENT block's V at the top of the iteration, in flight during S -- its registers are then free for P V.
//
// A BATCH of B sequences (the *_batch entry points) is the second grid dimension of both launches: workgroup (x, b) is the
// workgroup x of a single-sequence call on sequence b -- its own key count n_keys_dev[b], its own cache kv + b * seq_stride, the
// rows [b R, (b + 1) R) of q / out / row_sel, its own slice of the workspace -- and everything inside it is the source above
// (decode_sequence shifts the argument block; the single-sequence entry points launch B = 1, where every shift is zero).  The
// plan fills the chip with kv_heads x B x splits workgroups; with ragged lengths a short sequence's empty splits leave at once.
#include "attn_common.h"

namespace mq {

constexpr int AD_KB = 32;                        // keys per block
constexpr int AD_NW = 4;                         // waves per workgroup = ways a split's blocks are dealt out
constexpr int AD_M = 16;                         // (row, head-in-group) pairs of one pass
constexpr int AD_D = 128;
constexpr int AD_VROW = 256;                     // bytes of a V row in LDS (16-bit values)
constexpr int AD_WAVE_LDS = 4 * 16 * 64 * 4;     // a wave's partial O^T in the merge (16 KiB); the V tile (8 KiB) lives in the same bytes
constexpr int AD_STATS = AD_NW * 32 * 2 * 4;     // [wave][32 columns][m, l]
constexpr int AD_PART = AD_D + 2;                // floats of one partial state: acc[128], then (m, l) in a table of their own

struct AttnDecArgs {
    const void *q;             // [R, heads * 128] (row stride ldq elements), fp16 / bf16; a batch: [B * R, ..], as out, qout and row_sel
    const uint8_t *kv;         // cache: [T][ldkv] elements (e4m3 bytes, or q's dtype), per token the K heads, then the V heads
    const float *kv_scale;     // [2 * kv_heads]; null for a 16-bit cache (no scales: both factors 1)
    const int32_t *n_dev;      // optional device-side key count; a batch: [B]
    void *out;                 // [R, heads * 128] (row stride ldo elements), q's dtype
    float *ws;                 // splits > 1: acc [splits][R * heads][128], then ml [splits][R * heads][2]; a batch: B such slices
    long T, ldq, ldkv, ldo;
    int R, heads, kv_heads, causal;
    int splits, kps, passes;
    float softmax_scale;
    // optional: the int8 levels of the NEXT Linear's static activation quantizer instead of 16-bit values (AttnArgs of
    // attn_prefill.hip: the same fields, the same arithmetic)
    int8_t *qout;
    long q_kpad, q_ld;
    float qs0, qs1;
    const uint8_t *row_sel;
    float qi0, qi1;
    int qr0, qr1;
    // a batch: the cache of sequence b starts seq_stride ELEMENTS after that of b - 1 (0 at B = 1); row0 is set by decode_sequence
    long seq_stride, row0;
    int B;
};

// Workgroup (x, b) of a batched launch becomes workgroup x of a call on sequence b alone: the key count, the cache and the
// workspace slice move to b's, and row0 = b R is the global row of its first query row (q, out, row_sel and the tiled int8
// layout are addressed by global row).  b is blockIdx.y: uniform, scalar arithmetic on the argument block.  KVB = bytes of a
// cache element.
template <int KVB>
__device__ __forceinline__ void decode_sequence(AttnDecArgs &p)
{
    const long b = blockIdx.y;
    p.row0 = b * p.R;
    p.kv += b * p.seq_stride * KVB;
    if (p.n_dev) p.n_dev += b;
    if (p.ws) p.ws += b * ((long)p.splits * p.R * p.heads * AD_PART);
}

// n = clamp(*n_dev, R, T) through the VECTOR memory path (a buffer load; every lane receives the same dword)
__device__ __forceinline__ long decode_key_count(const AttnDecArgs &p)
{
    if (!p.n_dev) return p.T;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(p.n_dev), 0, 4, 0x00020000);
    long n = __builtin_amdgcn_readfirstlane((int)__builtin_amdgcn_raw_buffer_load_b32(rs, 0, 0, 0));
    n = n < p.R ? p.R : n;
    return n > p.T ? p.T : n;
}

// Four consecutive output values of row `row`, columns col .. col + 3: rounded once to DT and stored, or -- fused quantizer --
// the levels quantize_act_i8 gives for those rounded values (quant_levels_i8_packed, act_offset: the store of attn_prefill.hip)
template <int DT>
__device__ __forceinline__ void decode_store4(const AttnDecArgs &p, long row, long col, const float (&v)[4], unsigned sel)
{
    if (p.qout) {
        float r4[4];
        unsigned w[1];
#pragma unroll
        for (int e = 0; e < 4; ++e) r4[e] = Elem<DT>::rnd(v[e]);                       // the 16-bit value the unfused path stores
        quant_levels_i8_packed<4>(r4, sel ? p.qs1 : p.qs0, sel ? p.qi1 : p.qi0, (sel ? p.qr1 : p.qr0) != 0, w);
        *reinterpret_cast<unsigned *>(p.qout + act_offset(row, col, p.q_kpad, p.q_ld)) = w[0];
    } else {
        v4us h;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = Elem<DT>::st(v[e]);
        *reinterpret_cast<v4us *>(reinterpret_cast<unsigned short *>(p.out) + row * p.ldo + col) = h;
    }
}

template <int DT, int KVB>
__global__ __launch_bounds__(AD_NW * 64, 2) void attn_decode_kernel(AttnDecArgs p)
{
    kernarg_warm<sizeof(AttnDecArgs)>();
    typedef AttnMma<DT> MM;
    __shared__ __attribute__((aligned(16))) char smem[AD_NW * AD_WAVE_LDS + AD_STATS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    decode_sequence<KVB>(p);
    const int kvh = blockIdx.x % p.kv_heads, split = blockIdx.x / p.kv_heads;
    const int rep = p.heads / p.kv_heads, m_all = p.R * rep;
    const long n = decode_key_count(p);
    const long k0 = (long)split * p.kps;
    if (k0 >= n) return;                                              // an empty split (device key count): the whole workgroup leaves
    const long k1 = k0 + p.kps < n ? k0 + p.kps : n;
    const int n_blocks = (int)((k1 - k0 + AD_KB - 1) / AD_KB);

    const int ko = lane >> 5;                                         // lane half: d 64 ko.. of K / Q, keys + 4 ko of S, octet ko of P
    const float s_k = KVB == 1 ? p.kv_scale[kvh] : 1.0f;
    const float sc = s_k * p.softmax_scale * 1.4426950408889634f;     // K scale and log2(e) folded into the score scale
    const float s_v = KVB == 1 ? p.kv_scale[p.kv_heads + kvh] : 1.0f;
    char *vt = smem + wave * AD_WAVE_LDS;                             // this wave's V tile: [32 keys] rows of 256 bytes, swizzled
    float *stats = reinterpret_cast<float *>(smem + AD_NW * AD_WAVE_LDS);

    // K / V of this kv head, keys [0, n): rows at or beyond n answer zero (see the head of the file).  Everything here is in
    // BYTES (a head is AD_D * KVB of them); host: (T + 32) x the row stride in bytes < 2^32
    constexpr int NL = 4 * KVB;                                       // 16-byte loads of a lane's K piece, and of its V piece
    const unsigned ldkv = (unsigned)p.ldkv * KVB, kv_bytes = (unsigned)(n - 1) * ldkv + AD_D * KVB;
    const __amdgpu_buffer_rsrc_t k_rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p.kv) + (long)kvh * AD_D * KVB, 0, kv_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t v_rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p.kv) + (long)(p.kv_heads + kvh) * AD_D * KVB, 0, kv_bytes, 0x00020000);
    // K: the 64 values d 64 ko.. of key (lane & 31), straight into MFMA operands; V: the 64 values d 64 (lane & 1).. of key lane / 2
    const int v_key = lane >> 1, v_d = (lane & 1) * 64;
    const unsigned off_k = (unsigned)(lane & 31) * ldkv + 64 * KVB * ko, off_v = (unsigned)v_key * ldkv + v_d * KVB;
    auto load_k = [&](int kb, v4i (&kraw)[NL]) {
        const unsigned blk = (unsigned)(k0 + (long)kb * AD_KB) * ldkv;
#pragma unroll
        for (int j = 0; j < NL; ++j) kraw[j] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(k_rs, blk + off_k, 16 * j, 0));
    };
    auto load_v = [&](int kb, v4i (&vraw)[NL]) {
        const unsigned blk = (unsigned)(k0 + (long)kb * AD_KB) * ldkv;
#pragma unroll
        for (int j = 0; j < NL; ++j) vraw[j] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(v_rs, blk + off_v, 16 * j, 0));
    };
    auto load_block = [&](int kb, v4i (&kraw)[NL], v4i (&vraw)[NL]) {
        const unsigned blk = (unsigned)(k0 + (long)kb * AD_KB) * ldkv;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            kraw[j] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(k_rs, blk + off_k + 16 * j, 0, 0));
            vraw[j] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(v_rs, blk + off_v + 16 * j, 0, 0));
        }
    };
    const int t16 = lane & 15, g16 = (lane >> 4) & 1;

    for (int pass = 0; pass < p.passes; ++pass) {
        // ---- this lane's M row: m = row * rep + head-in-group; columns 16 .. 31 of the tile (and m >= R rep) are idle ----
        const int col = lane & 31, m = pass * AD_M + col;
        const bool live = col < AD_M && m < m_all;
        const int row = live ? m / rep : 0, head = kvh * rep + (live ? m - row * rep : 0);
        const unsigned sel = (live && p.qout && p.row_sel) ? p.row_sel[p.row0 + row] : 0;
        const long kmax = p.causal ? n - p.R + row : n - 1;           // last key this row attends to
        v4i Qf[8];
        {
            const unsigned short *qp = reinterpret_cast<const unsigned short *>(p.q) + (p.row0 + row) * p.ldq + (long)head * AD_D + 64 * ko;
#pragma unroll
            for (int ds = 0; ds < 8; ++ds) Qf[ds] = live ? *reinterpret_cast<const v4i *>(qp + ds * 8) : v4i{0, 0, 0, 0};
        }
        at_v16f O[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) O[dt][e] = 0.0f;
        float m_run = -1.0e30f, l_run = 0.0f;                          // log2 domain

        v4i kraw[NL], vraw[NL];
        if (wave < n_blocks) {
            if constexpr (KVB == 1) load_block(wave, kraw, vraw);
            else load_k(wave, kraw);
        }
        for (int kb = wave; kb < n_blocks; kb += AD_NW) {
            // ---- K into MFMA operands, V into this wave's LDS tile; e4m3 is widened on the way, 16-bit values go as they are
            v4i Kf[8];
            if constexpr (KVB == 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) widen16<DT>(kraw[j], Kf[2 * j], Kf[2 * j + 1]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v4i a, b;
                    widen16<DT>(vraw[j], a, b);
                    const int c = ((v_d + 16 * j) * 2) ^ ((v_key & 3) << 5);      // 32 B = sixteen values = one swizzle group
                    *reinterpret_cast<v4i *>(vt + v_key * AD_VROW + c) = a;
                    *reinterpret_cast<v4i *>(vt + v_key * AD_VROW + c + 16) = b;
                }
            } else {
                load_v(kb, vraw);                                                // this block's V: in flight during S
#pragma unroll
                for (int j = 0; j < 8; ++j) Kf[j] = kraw[j];                     // load j = the eight values d 64 ko + 8 j ..
            }
            if constexpr (KVB == 1)
                if (kb + AD_NW < n_blocks) load_block(kb + AD_NW, kraw, vraw);    // in flight during this block's arithmetic
            const long key0 = k0 + (long)kb * AD_KB;

            // ---- S^T = K Q^T : [32 keys][32 columns] ---------------------------------------------------------------
            at_v16f S;
#pragma unroll
            for (int e = 0; e < 16; ++e) S[e] = 0.0f;
#pragma unroll
            for (int ds = 0; ds < 8; ++ds) S = MM::mma(Kf[ds], Qf[ds], S);
            if constexpr (KVB == 2) {
                if (kb + AD_NW < n_blocks) load_k(kb + AD_NW, kraw);             // the next block's K: in flight from here on
#pragma unroll
                for (int j = 0; j < 8; ++j) {                                    // V piece j = the eight values d 64 (lane & 1) + 8 j ..
                    const int c = ((v_d + 8 * j) * 2) ^ ((v_key & 3) << 5);      // the swizzle moves bits 5, 6: bit 4 (odd j) stays
                    *reinterpret_cast<v4i *>(vt + v_key * AD_VROW + c) = vraw[j];
                }
            }

            // ---- online softmax (log2 domain); register r <-> key key0 + (r & 3) + 8 (r >> 2) + 4 ko.  A key this row may
            // not see scores -inf: it leaves the maximum alone and exp2 makes it an exact 0, also where a causal row has no
            // key at all in this block (m_run then keeps its start value, -1e30, and alpha below is exp2(0) = 1 on zeros).
            if (key0 + AD_KB - 1 > (p.causal ? n - p.R : n - 1)) {    // wave-uniform: some row loses some key of this block
                const long lim = kmax - key0;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if ((r & 3) + 8 * (r >> 2) + 4 * ko > lim) S[r] = -__builtin_inff();
            }
            float m_raw = fmaxf(S[0], S[1]);
#pragma unroll
            for (int r = 2; r < 16; ++r) m_raw = fmaxf(m_raw, S[r]);
            {                                                         // lane + 32 holds the other 16 keys of this column
                const auto mx = __builtin_amdgcn_permlane32_swap(__float_as_uint(m_raw), __float_as_uint(m_raw), false, false);
                m_raw = fmaxf(__uint_as_float(mx[0]), __uint_as_float(mx[1]));
            }
            const float m_new = fmaxf(m_run, m_raw * sc);
            float psum = 0.0f;
            unsigned pk[8];                                           // P as 16-bit pairs: pk[2 g + e2] = keys 8 g + 4 ko + 2 e2, + 1
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = __builtin_amdgcn_exp2f(fmaf(S[r], sc, -m_new));
                const float p1 = __builtin_amdgcn_exp2f(fmaf(S[r + 1], sc, -m_new));
                psum += p0 + p1;
                pk[r >> 1] = AttnCvt<DT>::pack2(p0, p1);
            }
            if (__any(m_new > m_run)) {                               // some column's maximum moved: rescale the running output
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
                l_run *= alpha;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                    for (int e = 0; e < 16; ++e) O[dt][e] *= alpha;
                m_run = m_new;
            }
            l_run += psum;

            // ---- O^T += V^T P^T : 2 k-steps of 16 keys x 4 tiles of 32 d ---------------------------------------------
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");    // this wave's V tile stores before its transpose reads
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const auto x0 = __builtin_amdgcn_permlane32_swap(pk[4 * ks + 0], pk[4 * ks + 2], false, false);
                const auto x1 = __builtin_amdgcn_permlane32_swap(pk[4 * ks + 1], pk[4 * ks + 3], false, false);
                const v4i pf = v4i{(int)x0[0], (int)x1[0], (int)x0[1], (int)x1[1]};
                v4i Af[4];
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const int d_lane = dt * 32 + 16 * g16 + 4 * (t16 & 3);
                    const int kA = ks * 16 + 8 * ko + (t16 >> 2);
                    const at_v4s r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((at_lds_v4s *)(vt + kA * AD_VROW + ((d_lane * 2) ^ ((kA & 3) << 5))));
                    const at_v4s r1 =
                        __builtin_amdgcn_ds_read_tr16_b64_v4i16((at_lds_v4s *)(vt + (kA + 4) * AD_VROW + ((d_lane * 2) ^ (((kA + 4) & 3) << 5))));
                    const v2i lo = __builtin_bit_cast(v2i, r0), hi = __builtin_bit_cast(v2i, r1);
                    Af[dt] = v4i{lo[0], lo[1], hi[0], hi[1]};
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) O[dt] = MM::mma(Af[dt], pf, O[dt]);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");    // ... and the reads before the next block's stores
            __builtin_amdgcn_wave_barrier();
        }

        // ---- merge the four waves' states (index order); wave w finishes d-tile w -------------------------------------
        l_run += __shfl_xor(l_run, 32, 64);
        float *mine = reinterpret_cast<float *>(vt);                  // [dt][e][lane]
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) mine[(dt * 16 + e) * 64 + lane] = O[dt][e];
        if (lane < 32) {
            stats[(wave * 32 + lane) * 2] = m_run;
            stats[(wave * 32 + lane) * 2 + 1] = l_run;
        }
        __syncthreads();
        float M = -1.0e30f;
#pragma unroll
        for (int w = 0; w < AD_NW; ++w) M = fmaxf(M, stats[(w * 32 + col) * 2]);
        float L = 0.0f, fw[AD_NW];
#pragma unroll
        for (int w = 0; w < AD_NW; ++w) {
            fw[w] = __builtin_amdgcn_exp2f(stats[(w * 32 + col) * 2] - M);
            L += stats[(w * 32 + col) * 2 + 1] * fw[w];
        }
        const int dt = wave;
        float acc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
        for (int w = 0; w < AD_NW; ++w) {
            const float *src = reinterpret_cast<const float *>(smem + w * AD_WAVE_LDS) + dt * 16 * 64 + lane;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] += src[e * 64] * fw[w];
        }
        if (live) {
            const long c0 = (long)head * AD_D + dt * 32 + 4 * ko;    // this lane's values: d = 32 dt + 8 g + 4 ko + e
            if (p.splits == 1) {
                const float f = L > 0.0f ? s_v / L : 0.0f;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float v4[4] = {acc[4 * g] * f, acc[4 * g + 1] * f, acc[4 * g + 2] * f, acc[4 * g + 3] * f};
                    decode_store4<DT>(p, p.row0 + row, c0 + 8 * g, v4, sel);
                }
            } else {
                const long rows = (long)p.R * p.heads, slot = (long)split * rows + (long)row * p.heads + head;
                float *a = p.ws + slot * AD_D + dt * 32 + 4 * ko;
#pragma unroll
                for (int g = 0; g < 4; ++g) *reinterpret_cast<v4f *>(a + 8 * g) = v4f{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                if (wave == 0 && ko == 0) {
                    float *ml = p.ws + (long)p.splits * rows * AD_D + slot * 2;
                    ml[0] = M;
                    ml[1] = L;
                }
            }
        }
        __syncthreads();                                              // the next pass's V tiles overwrite what the merge read
    }
}

// The second launch of a split call: one (row, head) per 32 lanes, four output columns per lane, the splits in index order.
template <int DT>
__global__ __launch_bounds__(256) void attn_decode_merge_kernel(AttnDecArgs p)
{
    decode_sequence<0>(p);                                            // the merge never touches the cache: its shift is unused
    const long rows = (long)p.R * p.heads, slot = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (slot >= rows) return;
    const int d = 4 * (threadIdx.x & 31);
    const long n = decode_key_count(p);
    int ns = (int)((n + p.kps - 1) / p.kps);                          // the splits that hold keys; the others wrote nothing
    ns = ns < p.splits ? ns : p.splits;
    const int row = (int)(slot / p.heads), head = (int)(slot - (long)row * p.heads);
    const float s_v = p.kv_scale ? p.kv_scale[p.kv_heads + head / (p.heads / p.kv_heads)] : 1.0f;      // a 16-bit cache has no scales
    const float *ml = p.ws + (long)p.splits * rows * AD_D;
    float M = -1.0e30f;
    for (int s = 0; s < ns; ++s) M = fmaxf(M, ml[((long)s * rows + slot) * 2]);
    float L = 0.0f, acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = 0; s < ns; ++s) {
        const long at = (long)s * rows + slot;
        const float w = __builtin_amdgcn_exp2f(ml[at * 2] - M);
        L += ml[at * 2 + 1] * w;
        const v4f a = *reinterpret_cast<const v4f *>(p.ws + at * AD_D + d);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += a[e] * w;
    }
    const float f = L > 0.0f ? s_v / L : 0.0f;
    const unsigned sel = (p.qout && p.row_sel) ? p.row_sel[p.row0 + row] : 0;
    const float v4[4] = {acc[0] * f, acc[1] * f, acc[2] * f, acc[3] * f};
    decode_store4<DT>(p, p.row0 + row, (long)head * AD_D + d, v4, sel);
}

struct AttnDecPlan {
    int splits, kps, grid, passes;
    size_t ws_bytes;
};

}  // namespace mq

static thread_local int g_dec_splits = 0, g_dec_kps = 0;      // TEST-ONLY (mq_attn_decode_debug_force): 0 = the heuristic

// Everything the host decides for a call; the launch, the workspace query and mq_attn_decode_debug_plan all come here.
// Heuristic: two workgroups fit a CU (LDS), so 2 x CUs / (kv_heads x B) splits per sequence fill the chip; a split is never
// shorter than 128 keys -- one block for each of the workgroup's four waves: below that the critical path (one block) no longer
// shrinks and only the merge grows.  B enters nowhere else: splits and keys_per_split are per sequence, grid and ws_bytes are
// B times the single-sequence figures, and B = 1 is the single-sequence plan integer for integer.
static int attn_decode_plan(const char *who, int B, int R, long T, int heads, int kv_heads, int cus, mq::AttnDecPlan &pl)
{
    using namespace mq;
    MQ_REQUIRE(B >= 1 && B <= 65535, "%s: B = %d sequences (1 .. 65535: the second grid dimension)", who, B);
    MQ_REQUIRE(R >= 1 && R <= 8, "%s: R = %d query rows (1 .. 8)", who, R);
    MQ_REQUIRE(heads >= 1 && kv_heads >= 1 && heads % kv_heads == 0, "%s: bad head counts %d / %d", who, heads, kv_heads);
    MQ_REQUIRE(T >= R, "%s: T = %ld keys for R = %d rows (the rows are the last R positions: T >= R)", who, T, R);
    MQ_REQUIRE(T <= (1L << 30), "%s: T = %ld exceeds 2^30 keys", who, T);
    long kps, splits;
    if (g_dec_kps > 0) {
        MQ_REQUIRE(g_dec_kps % AD_KB == 0, "%s: forced keys_per_split %d is no multiple of the %d-key block", who, g_dec_kps, AD_KB);
        kps = g_dec_kps;
        splits = g_dec_splits > 0 ? g_dec_splits : ceil_div(T, kps);
    } else if (g_dec_splits > 0) {
        splits = g_dec_splits;
        kps = ceil_div(ceil_div(T, splits), AD_KB) * AD_KB;
    } else {
        const long per = (long)kv_heads * B, want = 2L * cus / per > 1 ? 2L * cus / per : 1;
        kps = ceil_div(ceil_div(T, want), AD_KB) * AD_KB;
        if (kps < AD_NW * AD_KB) kps = AD_NW * AD_KB;
        splits = ceil_div(T, kps);
    }
    MQ_REQUIRE(splits * kps >= T && T > (splits - 1) * kps, "%s: forced plan of %ld splits of %ld keys does not cut T = %ld keys into non-empty ranges",
               who, splits, kps, T);
    MQ_REQUIRE(splits * kv_heads < (1L << 31), "%s: %ld splits of %d kv heads exceed the grid", who, splits, kv_heads);
    MQ_REQUIRE(splits * kv_heads * B < (1L << 31) && (long)B * R * heads < (1L << 31),
               "%s: B = %d sequences of %ld splits x %d kv heads, or of %d x %d (row, head) pairs, do not fit an int", who, B, splits, kv_heads, R, heads);
    pl.splits = (int)splits;
    pl.kps = (int)kps;
    pl.grid = (int)(splits * kv_heads * B);
    pl.passes = (R * (heads / kv_heads) + AD_M - 1) / AD_M;
    pl.ws_bytes = splits > 1 ? (size_t)B * splits * R * heads * AD_PART * sizeof(float) : 0;
    return MQ_OK;
}

extern "C" int mq_attn_decode_debug_force(int splits, int keys_per_split)
{
    MQ_REQUIRE(splits >= 0 && keys_per_split >= 0, "mq_attn_decode_debug_force: negative value");
    g_dec_splits = splits;
    g_dec_kps = keys_per_split;
    return MQ_OK;
}

static int attn_decode_debug_plan(const char *who, int B, int R, long T, int heads, int kv_heads, int *plan)
{
    MQ_REQUIRE(plan, "%s: null pointer", who);
    mq::AttnDecPlan pl;
    const int rc = attn_decode_plan(who, B, R, T, heads, kv_heads, mq::device_cu_count(), pl);
    if (rc != MQ_OK) return rc;
    MQ_REQUIRE(pl.ws_bytes < (1UL << 31), "%s: workspace of %zu bytes does not fit the plan's int", who, pl.ws_bytes);
    plan[MQ_ATTN_DECODE_PLAN_SPLITS] = pl.splits;
    plan[MQ_ATTN_DECODE_PLAN_KEYS_PER_SPLIT] = pl.kps;
    plan[MQ_ATTN_DECODE_PLAN_GRID] = pl.grid;
    plan[MQ_ATTN_DECODE_PLAN_PASSES] = pl.passes;
    plan[MQ_ATTN_DECODE_PLAN_WORKSPACE] = (int)pl.ws_bytes;
    return MQ_OK;
}

extern "C" int mq_attn_decode_debug_plan(int R, long T, int heads, int kv_heads, int *plan)
{
    return attn_decode_debug_plan("mq_attn_decode_debug_plan", 1, R, T, heads, kv_heads, plan);
}

extern "C" int mq_attn_decode_batch_debug_plan(int B, int R, long T, int heads, int kv_heads, int *plan)
{
    return attn_decode_debug_plan("mq_attn_decode_batch_debug_plan", B, R, T, heads, kv_heads, plan);
}

extern "C" size_t mq_attn_decode_workspace_bytes(int R, long T, int heads, int kv_heads)
{
    mq::AttnDecPlan pl;
    if (attn_decode_plan("mq_attn_decode_workspace_bytes", 1, R, T, heads, kv_heads, mq::device_cu_count(), pl) != MQ_OK) return 0;
    return pl.ws_bytes;
}

extern "C" size_t mq_attn_decode_batch_workspace_bytes(int B, int R, long T, int heads, int kv_heads)
{
    mq::AttnDecPlan pl;
    if (attn_decode_plan("mq_attn_decode_batch_workspace_bytes", B, R, T, heads, kv_heads, mq::device_cu_count(), pl) != MQ_OK) return 0;
    return pl.ws_bytes;
}

// the checks the two entry points share (the rules of mq_attn_prefill_fp8kv), then the plan and the launches
// kvb = bytes of a cache element: 1 = e4m3 with scales, 2 = q's dtype without
static int attn_decode_run(const char *who, mq::AttnDecArgs &a, int kvb, int dtype, int head_dim, void *workspace, size_t workspace_bytes, void *stream)
{
    using namespace mq;
    constexpr int D = AD_D;
    MQ_REQUIRE(dtype == MQ_F16 || dtype == MQ_BF16, "%s: q / out dtype must be fp16 or bf16 (got %d)", who, dtype);
    MQ_REQUIRE(head_dim == D, "%s: head_dim %d (built for 128)", who, head_dim);
    // the running maximum is taken over RAW scores and the (positive) scale applied afterwards (attn_prefill.hip)
    MQ_REQUIRE(a.softmax_scale > 0.0f && a.softmax_scale < 3.0e38f, "%s: softmax_scale must be positive and finite (got %g)", who, (double)a.softmax_scale);
    AttnDecPlan pl;
    const int rc = attn_decode_plan(who, a.B, a.R, a.T, a.heads, a.kv_heads, device_cu_count(), pl);
    if (rc != MQ_OK) return rc;
    MQ_REQUIRE(a.q && a.kv && (a.kv_scale || kvb == 2) && (a.out || a.qout), "%s: null pointer", who);
    MQ_REQUIRE(a.ldq >= (long)a.heads * D && a.ldkv >= 2L * a.kv_heads * D && (a.qout || a.ldo >= (long)a.heads * D), "%s: row strides too short", who);
    MQ_REQUIRE(((uintptr_t)a.q) % 16 == 0 && (a.ldq * 2) % 16 == 0 && ((uintptr_t)a.kv) % 16 == 0 && (a.ldkv * kvb) % 16 == 0 &&
                   (a.qout || (((uintptr_t)a.out) % 8 == 0 && (a.ldo * 2) % 8 == 0)),
               "%s: q / cache rows must be 16-byte aligned, out rows 8-byte aligned", who);
    MQ_REQUIRE(((uintptr_t)a.n_dev) % 4 == 0, "%s: n_keys_dev must be 4-byte aligned", who);
    // K / V are addressed through 32-bit buffer offsets (one block past the last row included)
    MQ_REQUIRE(a.ldkv < (1L << 32) && (a.T + AD_KB) * a.ldkv * kvb < (1L << 32),
               "%s: (T + 32) x the cache row stride in bytes must stay below 4 GiB (T %ld, stride %ld bytes)", who, a.T, a.ldkv * kvb);
    if (a.B > 1) {                                                    // sequence b's cache: kv + b * seq_stride (64-bit), rows as above
        MQ_REQUIRE(a.seq_stride >= a.T * a.ldkv, "%s: seq_stride %ld shorter than one sequence's T * ldkv = %ld elements", who, a.seq_stride,
                   a.T * a.ldkv);
        MQ_REQUIRE((a.seq_stride * kvb) % 16 == 0, "%s: seq_stride must be a multiple of 16 bytes (got %ld bytes)", who, a.seq_stride * kvb);
    } else {
        a.seq_stride = 0;
    }
    if (pl.ws_bytes) {
        MQ_REQUIRE(workspace && workspace_bytes >= pl.ws_bytes, "%s: %d key splits need a workspace of %zu bytes (got %zu)", who, pl.splits, pl.ws_bytes,
                   workspace ? workspace_bytes : (size_t)0);
        MQ_REQUIRE(((uintptr_t)workspace) % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    }
    a.ws = reinterpret_cast<float *>(workspace);
    a.splits = pl.splits;
    a.kps = pl.kps;
    a.passes = pl.passes;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(pl.grid / a.B), (unsigned)a.B), block(AD_NW * 64);
    if (kvb == 1) {
        if (dtype == MQ_F16) hipLaunchKernelGGL((attn_decode_kernel<MQ_F16, 1>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((attn_decode_kernel<MQ_BF16, 1>), grid, block, 0, st, a);
    } else {
        if (dtype == MQ_F16) hipLaunchKernelGGL((attn_decode_kernel<MQ_F16, 2>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((attn_decode_kernel<MQ_BF16, 2>), grid, block, 0, st, a);
    }
    int lrc = check_launch("attn_decode");
    if (lrc != MQ_OK || pl.splits == 1) return lrc;
    const dim3 mgrid((unsigned)((a.R * a.heads + 7) / 8), (unsigned)a.B);
    if (dtype == MQ_F16) hipLaunchKernelGGL(attn_decode_merge_kernel<MQ_F16>, mgrid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(attn_decode_merge_kernel<MQ_BF16>, mgrid, dim3(256), 0, st, a);
    return check_launch("attn_decode_merge");
}

// the arguments the entry points share, and those of the fused quantizer (checked under the entry point's name)
static mq::AttnDecArgs attn_decode_args(const void *q, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads, long ldq, const void *kv_cache,
                                        long ldkv, const float *kv_scale, float softmax_scale, int causal, void *out, long ldo)
{
    mq::AttnDecArgs a{};
    a.q = q; a.kv = reinterpret_cast<const uint8_t *>(kv_cache); a.kv_scale = kv_scale; a.n_dev = n_keys_dev; a.out = out; a.T = T; a.ldq = ldq;
    a.ldkv = ldkv; a.ldo = ldo; a.R = R; a.heads = heads; a.kv_heads = kv_heads; a.causal = causal ? 1 : 0; a.softmax_scale = softmax_scale;
    a.qs0 = a.qs1 = a.qi0 = a.qi1 = 1.0f;
    a.B = 1;
    return a;
}

static int attn_decode_quant_args(const char *who, mq::AttnDecArgs &a, float scale0, float scale1, const uint8_t *row_sel, int8_t *out, long K_pad, long ldo)
{
    using namespace mq;
    a.qout = out; a.q_kpad = K_pad; a.q_ld = ldo; a.qs0 = scale0; a.qs1 = scale1; a.row_sel = row_sel;
    MQ_REQUIRE(a.heads >= 1 && K_pad == (long)a.heads * AD_D && K_pad % 64 == 0 && ((uintptr_t)out) % 16 == 0 && (ldo == MQ_LD_TILED || (ldo >= K_pad && ldo % 4 == 0)),
               "%s: out must hold exactly heads * head_dim = %ld columns (K_pad %ld, a multiple of 64), ldo = MQ_LD_TILED or a row stride", who,
               (long)a.heads * AD_D, K_pad);
    MQ_REQUIRE(scale0 > 0.0f && scale1 > 0.0f, "%s: scales must be positive", who);
    a.qi0 = 1.0f / scale0; a.qi1 = 1.0f / scale1; a.qr0 = quant_rcp_ok(scale0) ? 1 : 0; a.qr1 = quant_rcp_ok(scale1) ? 1 : 0;
    return MQ_OK;
}

extern "C" int mq_attn_decode_fp8kv(const void *q, int dtype, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads, int head_dim,
                                    long ldq, const uint8_t *kv_cache, long ldkv, const float *kv_scale, float softmax_scale, int causal,
                                    void *out, long ldo, void *workspace, size_t workspace_bytes, void *stream)
{
    mq::AttnDecArgs a = attn_decode_args(q, R, T, n_keys_dev, heads, kv_heads, ldq, kv_cache, ldkv, kv_scale, softmax_scale, causal, out, ldo);
    return attn_decode_run("mq_attn_decode_fp8kv", a, 1, dtype, head_dim, workspace, workspace_bytes, stream);
}

extern "C" int mq_attn_decode_fp8kv_quant_i8(const void *q, int dtype, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads, int head_dim,
                                             long ldq, const uint8_t *kv_cache, long ldkv, const float *kv_scale, float softmax_scale, int causal,
                                             float scale0, float scale1, const uint8_t *row_sel, int8_t *out, long K_pad, long ldo,
                                             void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "mq_attn_decode_fp8kv_quant_i8";
    mq::AttnDecArgs a = attn_decode_args(q, R, T, n_keys_dev, heads, kv_heads, ldq, kv_cache, ldkv, kv_scale, softmax_scale, causal, nullptr, 0);
    const int rc = attn_decode_quant_args(who, a, scale0, scale1, row_sel, out, K_pad, ldo);
    return rc != MQ_OK ? rc : attn_decode_run(who, a, 1, dtype, head_dim, workspace, workspace_bytes, stream);
}

// ---- the same two calls over a 16-bit cache: kv_cache in q's dtype, ldkv in elements, no scales ----
extern "C" int mq_attn_decode(const void *q, int dtype, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads, int head_dim, long ldq,
                              const void *kv_cache, long ldkv, float softmax_scale, int causal, void *out, long ldo, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    mq::AttnDecArgs a = attn_decode_args(q, R, T, n_keys_dev, heads, kv_heads, ldq, kv_cache, ldkv, nullptr, softmax_scale, causal, out, ldo);
    return attn_decode_run("mq_attn_decode", a, 2, dtype, head_dim, workspace, workspace_bytes, stream);
}

extern "C" int mq_attn_decode_quant_i8(const void *q, int dtype, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads, int head_dim,
                                       long ldq, const void *kv_cache, long ldkv, float softmax_scale, int causal, float scale0, float scale1,
                                       const uint8_t *row_sel, int8_t *out, long K_pad, long ldo, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    const char *who = "mq_attn_decode_quant_i8";
    mq::AttnDecArgs a = attn_decode_args(q, R, T, n_keys_dev, heads, kv_heads, ldq, kv_cache, ldkv, nullptr, softmax_scale, causal, nullptr, 0);
    const int rc = attn_decode_quant_args(who, a, scale0, scale1, row_sel, out, K_pad, ldo);
    return rc != MQ_OK ? rc : attn_decode_run(who, a, 2, dtype, head_dim, workspace, workspace_bytes, stream);
}

// ---- the four calls over a batch: B sequences of R rows each, sequence b's cache at kv_cache + b * seq_stride elements, its key
// count at n_keys_dev[b].  B = 1 is the sibling (seq_stride is ignored).
static void attn_decode_batch(mq::AttnDecArgs &a, int B, long seq_stride)
{
    a.B = B;
    a.seq_stride = seq_stride;
}

extern "C" int mq_attn_decode_fp8kv_batch(const void *q, int dtype, int B, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads,
                                          int head_dim, long ldq, const uint8_t *kv_cache, long ldkv, long seq_stride, const float *kv_scale,
                                          float softmax_scale, int causal, void *out, long ldo, void *workspace, size_t workspace_bytes,
                                          void *stream)
{
    mq::AttnDecArgs a = attn_decode_args(q, R, T, n_keys_dev, heads, kv_heads, ldq, kv_cache, ldkv, kv_scale, softmax_scale, causal, out, ldo);
    attn_decode_batch(a, B, seq_stride);
    return attn_decode_run("mq_attn_decode_fp8kv_batch", a, 1, dtype, head_dim, workspace, workspace_bytes, stream);
}

extern "C" int mq_attn_decode_fp8kv_quant_i8_batch(const void *q, int dtype, int B, int R, long T, const int32_t *n_keys_dev, int heads,
                                                   int kv_heads, int head_dim, long ldq, const uint8_t *kv_cache, long ldkv, long seq_stride,
                                                   const float *kv_scale, float softmax_scale, int causal, float scale0, float scale1,
                                                   const uint8_t *row_sel, int8_t *out, long K_pad, long ldo, void *workspace,
                                                   size_t workspace_bytes, void *stream)
{
    const char *who = "mq_attn_decode_fp8kv_quant_i8_batch";
    mq::AttnDecArgs a = attn_decode_args(q, R, T, n_keys_dev, heads, kv_heads, ldq, kv_cache, ldkv, kv_scale, softmax_scale, causal, nullptr, 0);
    attn_decode_batch(a, B, seq_stride);
    const int rc = attn_decode_quant_args(who, a, scale0, scale1, row_sel, out, K_pad, ldo);
    return rc != MQ_OK ? rc : attn_decode_run(who, a, 1, dtype, head_dim, workspace, workspace_bytes, stream);
}

extern "C" int mq_attn_decode_batch(const void *q, int dtype, int B, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads,
                                    int head_dim, long ldq, const void *kv_cache, long ldkv, long seq_stride, float softmax_scale, int causal,
                                    void *out, long ldo, void *workspace, size_t workspace_bytes, void *stream)
{
    mq::AttnDecArgs a = attn_decode_args(q, R, T, n_keys_dev, heads, kv_heads, ldq, kv_cache, ldkv, nullptr, softmax_scale, causal, out, ldo);
    attn_decode_batch(a, B, seq_stride);
    return attn_decode_run("mq_attn_decode_batch", a, 2, dtype, head_dim, workspace, workspace_bytes, stream);
}

extern "C" int mq_attn_decode_quant_i8_batch(const void *q, int dtype, int B, int R, long T, const int32_t *n_keys_dev, int heads, int kv_heads,
                                             int head_dim, long ldq, const void *kv_cache, long ldkv, long seq_stride, float softmax_scale,
                                             int causal, float scale0, float scale1, const uint8_t *row_sel, int8_t *out, long K_pad, long ldo,
                                             void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "mq_attn_decode_quant_i8_batch";
    mq::AttnDecArgs a = attn_decode_args(q, R, T, n_keys_dev, heads, kv_heads, ldq, kv_cache, ldkv, nullptr, softmax_scale, causal, nullptr, 0);
    attn_decode_batch(a, B, seq_stride);
    const int rc = attn_decode_quant_args(who, a, scale0, scale1, row_sel, out, K_pad, ldo);
    return rc != MQ_OK ? rc : attn_decode_run(who, a, 2, dtype, head_dim, workspace, workspace_bytes, stream);
}
