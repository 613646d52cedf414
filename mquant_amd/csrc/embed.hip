// embed.hip -- the first launch of a captured generation step: hidden = embed_tokens[token], with the token id(s) read from
// DEVICE memory (what mq_gemv_f16_argmax wrote at the end of the previous step), so that the step feeds itself and one graph is
// replayed N times for N tokens:
//
//     id_r = clamp(ids_dev[r], 0, vocab - 1)                  r = 0 .. R - 1
//     out[r][0 .. dim) = table[id_r][0 .. dim)                a bit copy, 16 bytes per lane
//     id_log[n - R + r] = id_r                                optional; n = n_keys_dev ? clamp(*n_keys_dev, R, log_rows) : log_rows
//
// n is the integer and the clamp of mq_kv_append_rope_fp8 -- the key count AFTER this step's append -- so the log is indexed by
// cache position and the host reads N generated ids after N replays, in one copy.  Both clamps are MEMORY SAFETY, not semantics:
// the host checks every buffer against R, vocab, dim and log_rows, and whatever the device integers hold, every access stays
// inside those buffers.  No reference counterpart (the reference generates through HF's host loop).
//
// The cost is one dispatch: the argument block is pulled in one round trip, the ids and the count arrive through the vector memory
// path (load_device_int), the log entry leaves with an ordinary vector store.  One workgroup = 256 16-byte chunks of ONE row (the id
// is uniform in it); the grid depends on R and dim only.
//
// mq_embed_gather_batch is the same launch for B <= 8 SEQUENCES of one new row each: row b takes ids_dev[b], and its id is logged
// in sequence b's own log at its own position, id_log[b * ld_log + n_b - 1], n_b = clamp(n_keys_dev[b], 1, log_rows).
#include "mq_common.h"

namespace mq {

struct EmbedArgs {
    const void *table;         // [vocab][ldt] 16-bit elements
    const int32_t *ids;        // [R], device
    void *out;                 // [R][ldo]
    int32_t *log;              // optional [log_rows]
    const int32_t *n_dev;      // optional device-side key count
    long vocab, dim, ldt, ldo, log_rows;
    int R;
    int batch;                 // != 0: the R rows are R sequences of one row each, with a key count and a log (ld_log apart) each
    long ld_log;
};

__global__ __launch_bounds__(256) void embed_gather_kernel(EmbedArgs p)
{
    kernarg_warm<sizeof(EmbedArgs)>();
    const int r = blockIdx.y;
    long id = load_device_int(p.ids + r);
    id = id < 0 ? 0 : id;                                             // memory safety: the row lies inside the table
    id = id > p.vocab - 1 ? p.vocab - 1 : id;
    const long seq = p.batch ? r : 0, rows = p.batch ? 1 : p.R;       // this row's sequence, and the new rows of a sequence
    long n = p.log_rows;
    if (p.log && p.n_dev) {
        n = load_device_int(p.n_dev + seq);
        n = n < rows ? rows : n;                                      // memory safety: entries [n - rows, n) lie inside [0, log_rows)
        n = n > p.log_rows ? p.log_rows : n;
    }
    const long c = (long)blockIdx.x * 256 + threadIdx.x;              // 16-byte chunk of the row
    if (c < p.dim / 8)
        *reinterpret_cast<v4i *>(reinterpret_cast<unsigned short *>(p.out) + (long)r * p.ldo + c * 8) =
            *reinterpret_cast<const v4i *>(reinterpret_cast<const unsigned short *>(p.table) + id * p.ldt + c * 8);
    if (p.log && c == 0) p.log[seq * p.ld_log + n - rows + (r - seq)] = (int32_t)id;
}

}  // namespace mq

// the checks and the launch of both entry points; batch != 0: R is the number of sequences
static int embed_gather_run(const char *who, int batch, const void *table, int dtype, long vocab, long dim, long ldt, const int32_t *ids_dev, int R,
                            void *out, long ldo, int32_t *id_log, long ld_log, long log_rows, const int32_t *n_keys_dev, void *stream)
{
    using namespace mq;
    MQ_REQUIRE(table && ids_dev && out, "%s: null pointer", who);
    MQ_REQUIRE(dtype == MQ_F16 || dtype == MQ_BF16, "%s: dtype must be fp16 or bf16 (got %d)", who, dtype);
    if (batch) MQ_REQUIRE(R >= 1 && R <= 8, "%s: B = %d sequences (1 .. 8)", who, R);
    else MQ_REQUIRE(R >= 1 && R <= 8, "%s: R = %d rows (1 .. 8)", who, R);
    MQ_REQUIRE(vocab >= 1 && vocab <= 0x7fffffffL, "%s: vocab = %ld table rows (1 .. 2^31 - 1: the ids are int32)", who, vocab);
    MQ_REQUIRE(dim >= 8 && dim % 8 == 0 && dim <= (1L << 31), "%s: dim = %ld (a positive multiple of 8, at most 2^31)", who, dim);
    MQ_REQUIRE(ldt >= dim, "%s: table row stride %ld shorter than dim = %ld", who, ldt, dim);
    MQ_REQUIRE(ldo >= dim, "%s: out row stride %ld shorter than dim = %ld", who, ldo, dim);
    MQ_REQUIRE(((uintptr_t)table) % 16 == 0 && (ldt * 2) % 16 == 0, "%s: table rows must be 16-byte aligned", who);
    MQ_REQUIRE(((uintptr_t)out) % 16 == 0 && (ldo * 2) % 16 == 0, "%s: out rows must be 16-byte aligned", who);
    MQ_REQUIRE(((uintptr_t)ids_dev) % 4 == 0, "%s: ids_dev must be 4-byte aligned", who);
    if (id_log) {
        if (batch) {
            MQ_REQUIRE(log_rows >= 1, "%s: log_rows = %ld entries (every sequence logs one row: log_rows >= 1)", who, log_rows);
            MQ_REQUIRE(R == 1 || ld_log >= log_rows, "%s: ld_log %ld shorter than one sequence's log_rows = %ld entries", who, ld_log, log_rows);
        } else {
            MQ_REQUIRE(log_rows >= R, "%s: log_rows = %ld entries for R = %d rows (the rows are the last R positions: log_rows >= R)", who, log_rows, R);
        }
        MQ_REQUIRE(((uintptr_t)id_log) % 4 == 0, "%s: id_log must be 4-byte aligned", who);
    }
    MQ_REQUIRE(((uintptr_t)n_keys_dev) % 4 == 0, "%s: n_keys_dev must be 4-byte aligned", who);

    EmbedArgs a{table, ids_dev, out, id_log, n_keys_dev, vocab, dim, ldt, ldo, log_rows, R, batch, batch && R > 1 ? ld_log : 0};
    const dim3 grid((unsigned)((dim / 8 + 255) / 256), (unsigned)R);
    hipLaunchKernelGGL(embed_gather_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return check_launch("embed_gather");
}

extern "C" int mq_embed_gather(const void *table, int dtype, long vocab, long dim, long ldt, const int32_t *ids_dev, int R, void *out, long ldo,
                               int32_t *id_log, long log_rows, const int32_t *n_keys_dev, void *stream)
{
    return embed_gather_run("mq_embed_gather", 0, table, dtype, vocab, dim, ldt, ids_dev, R, out, ldo, id_log, 0, log_rows, n_keys_dev, stream);
}

extern "C" int mq_embed_gather_batch(const void *table, int dtype, long vocab, long dim, long ldt, const int32_t *ids_dev, int B, void *out,
                                     long ldo, int32_t *id_log, long ld_log, long log_rows, const int32_t *n_keys_dev, void *stream)
{
    return embed_gather_run("mq_embed_gather_batch", 1, table, dtype, vocab, dim, ldt, ids_dev, B, out, ldo, id_log, ld_log, log_rows, n_keys_dev,
                            stream);
}
