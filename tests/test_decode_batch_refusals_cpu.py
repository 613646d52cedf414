"""What the batched entry points of a generation step refuse, and in which words (csrc/attn_decode.hip, kv_append.hip, embed.hip),
in the style of tests/test_attn_decode_refusals_cpu.py: the host checks run before anything touches a device, so every call here
is made with dummy addresses on any machine -- a table of violating calls, each with the status and the mq_last_error() text it
must produce.  Nothing in the table may reach a launch."""

import pytest

from mquant_amd import _lib

EINVAL = -1
F16, BF16, F32 = _lib.MQ_F16, _lib.MQ_BF16, _lib.MQ_F32
P = 0x7F0000001000             # a 16-byte aligned address nobody dereferences: every call is refused first
DEC8, DEC8Q = "mq_attn_decode_fp8kv_batch", "mq_attn_decode_fp8kv_quant_i8_batch"
DEC, DECQ = "mq_attn_decode_batch", "mq_attn_decode_quant_i8_batch"
APP8, APP = "mq_kv_append_rope_fp8_batch", "mq_kv_append_rope_batch"
EMB = "mq_embed_gather_batch"
ATTN = (DEC8, DEC8Q, DEC, DECQ)
APPEND = (APP8, APP)
CACHE = ATTN + APPEND

# the parameter names of include/mquant_hip.h, in order
PARAMS = {
    DEC8: "q dtype B R T n_keys_dev heads kv_heads head_dim ldq kv_cache ldkv seq_stride kv_scale softmax_scale causal out ldo workspace "
          "workspace_bytes stream",
    DEC8Q: "q dtype B R T n_keys_dev heads kv_heads head_dim ldq kv_cache ldkv seq_stride kv_scale softmax_scale causal scale0 scale1 row_sel "
           "out K_pad ldo workspace workspace_bytes stream",
    DEC: "q dtype B R T n_keys_dev heads kv_heads head_dim ldq kv_cache ldkv seq_stride softmax_scale causal out ldo workspace workspace_bytes "
         "stream",
    DECQ: "q dtype B R T n_keys_dev heads kv_heads head_dim ldq kv_cache ldkv seq_stride softmax_scale causal scale0 scale1 row_sel out K_pad "
          "ldo workspace workspace_bytes stream",
    APP8: "qkv dtype B R T n_keys_dev rope_delta_dev heads kv_heads head_dim ldqkv cos sin table_rows kv_cache ldkv seq_stride kv_scale stream",
    APP: "qkv dtype B R T n_keys_dev rope_delta_dev heads kv_heads head_dim ldqkv cos sin table_rows kv_cache ldkv seq_stride stream",
    EMB: "table dtype vocab dim ldt ids_dev B out ldo id_log ld_log log_rows n_keys_dev stream",
}
# well-formed calls: two sequences of one row of the 7B geometry over 64 keys (one key range: no workspace), the caches back to
# back; a table row overrides what it violates
BASE = dict(q=P, qkv=P, dtype=F16, B=2, R=1, T=64, n_keys_dev=P, rope_delta_dev=None, heads=28, kv_heads=4, head_dim=128, ldq=28 * 128,
            ldqkv=36 * 128, kv_cache=P, ldkv=1024, seq_stride=64 * 1024, kv_scale=P, softmax_scale=0.088, causal=1, out=P, ldo=28 * 128,
            workspace=None, workspace_bytes=0, stream=None, cos=P, sin=P, table_rows=64)
PER_FN = {DEC8Q: dict(scale0=0.5, scale1=0.5, row_sel=None, K_pad=28 * 128, ldo=28 * 128),
          DECQ: dict(scale0=0.5, scale1=0.5, row_sel=None, K_pad=28 * 128, ldo=28 * 128),
          EMB: dict(table=P, vocab=1000, dim=512, ldt=512, ids_dev=P, B=2, out=P, ldo=512, id_log=P, ld_log=64, log_rows=64)}
# T = 4096 at (28, 4) and B = 2: 256 CUs / (4 x 2) x 2 = 64 ranges wanted, 128 keys at the least -> 32 ranges, per sequence
WS_ONE = 32 * 28 * 130 * 4
WS_4096 = dict(T=4096, seq_stride=4096 * 1024)

# (entry point, what the call violates, overrides of the well-formed call, (splits, keys_per_split) for mq_attn_decode_debug_force or None)
CALLS = (
    [(f, "no sequences", dict(B=0), None) for f in CACHE]
    + [(f, "too many sequences", dict(B=65536), None) for f in CACHE]
    + [(EMB, "no sequences", dict(B=0), None), (EMB, "nine sequences", dict(B=9), None)]
    + [(f, "caches that overlap", dict(seq_stride=64 * 1024 - 16), None) for f in CACHE]
    + [(f, "seq_stride % 16 bytes", dict(seq_stride=64 * 1024 + 8), None) for f in (DEC8, DEC8Q, APP8)]
    + [(f, "seq_stride % 16 bytes", dict(seq_stride=64 * 1024 + 4), None) for f in (DEC, DECQ, APP)]
    + [(f, "no workspace", WS_4096, None) for f in ATTN]
    + [(f, "a workspace for one sequence", dict(WS_4096, workspace=P, workspace_bytes=WS_ONE), None) for f in ATTN]
    + [(f, "forced ranges, a workspace for one sequence", dict(workspace=P, workspace_bytes=2 * 28 * 130 * 4), (2, 32)) for f in ATTN]
    + [(f, "misaligned key counts", dict(n_keys_dev=P + 2), None) for f in CACHE + (EMB,)]
    + [(f, "misaligned offsets", dict(rope_delta_dev=P + 2), None) for f in APPEND]
    + [(f, "null q", dict(q=None), None) for f in ATTN]
    + [(f, "null qkv", dict(qkv=None), None) for f in APPEND]
    + [(f, "null cache", dict(kv_cache=None), None) for f in CACHE]
    + [(f, "null scales", dict(kv_scale=None), None) for f in (DEC8, DEC8Q, APP8)]
    + [(f, "null out", dict(out=None), None) for f in ATTN + (EMB,)]
    + [(EMB, "null table", dict(table=None), None), (EMB, "null ids", dict(ids_dev=None), None)]
    + [(f, "head_dim 64", dict(head_dim=64), None) for f in ATTN]
    + [(f, "head_dim 24", dict(head_dim=24), None) for f in APPEND]
    + [(f, "nine rows", dict(R=9), None) for f in CACHE]
    + [(f, "fp32", dict(dtype=F32), None) for f in CACHE + (EMB,)]
    + [(f, "only cos", dict(sin=None), None) for f in APPEND]
    + [(EMB, "logs that overlap", dict(ld_log=63), None), (EMB, "no log rows", dict(log_rows=0, ld_log=0), None),
       (EMB, "dim % 8", dict(dim=508), None)]
)


def _each(fns, text):
    return [(EINVAL, f"{f}: {text}") for f in fns]


# (status, mq_last_error()) of every row of CALLS, in order
EXPECTED = (
    _each(CACHE, "B = 0 sequences (1 .. 65535: the second grid dimension)")
    + _each(CACHE, "B = 65536 sequences (1 .. 65535: the second grid dimension)")
    + _each([EMB], "B = 0 sequences (1 .. 8)") + _each([EMB], "B = 9 sequences (1 .. 8)")
    + _each(CACHE, "seq_stride 65520 shorter than one sequence's T * ldkv = 65536 elements")
    + _each((DEC8, DEC8Q, APP8), "seq_stride must be a multiple of 16 bytes (got 65544 bytes)")
    + _each((DEC, DECQ, APP), "seq_stride must be a multiple of 16 bytes (got 131080 bytes)")
    + _each(ATTN, f"32 key splits need a workspace of {2 * WS_ONE} bytes (got 0)")
    + _each(ATTN, f"32 key splits need a workspace of {2 * WS_ONE} bytes (got {WS_ONE})")
    + _each(ATTN, f"2 key splits need a workspace of {2 * 2 * 28 * 130 * 4} bytes (got {2 * 28 * 130 * 4})")
    + _each(CACHE + (EMB,), "n_keys_dev must be 4-byte aligned")
    + _each(APPEND, "rope_delta_dev must be 4-byte aligned")
    + _each(ATTN, "null pointer")
    + _each(APPEND, "null pointer")
    + _each(CACHE, "null pointer")
    + _each((DEC8, DEC8Q, APP8), "null pointer")
    + _each(ATTN + (EMB,), "null pointer")
    + _each([EMB], "null pointer") * 2
    + _each(ATTN, "head_dim 64 (built for 128)")
    + _each(APPEND, "head_dim 24 (a multiple of 16)")
    + _each(ATTN, "R = 9 query rows (1 .. 8)") + _each(APPEND, "R = 9 new rows (1 .. 8)")
    + _each(ATTN, "q / out dtype must be fp16 or bf16 (got 2)") + _each(APPEND, "qkv dtype must be fp16 or bf16 (got 2)")
    + _each([EMB], "dtype must be fp16 or bf16 (got 2)")
    + _each(APPEND, "cos and sin must both be given or both be null (append only)")
    + _each([EMB], "ld_log 63 shorter than one sequence's log_rows = 64 entries")
    + _each([EMB], "log_rows = 0 entries (every sequence logs one row: log_rows >= 1)")
    + _each([EMB], "dim = 508 (a positive multiple of 8, at most 2^31)")
)


def refusal(fn, overrides, force):
    """(status, message) of one call"""
    lib = _lib.load()
    values = {**BASE, **PER_FN.get(fn, {}), **overrides}
    args = [values[name] for name in PARAMS[fn].split()]
    if force is not None:
        lib.mq_attn_decode_debug_force(*force)
    try:
        rc = getattr(lib, fn)(*args)
    finally:
        lib.mq_attn_decode_debug_force(0, 0)
    return rc, lib.mq_last_error().decode()


def test_the_table_and_its_expectations_line_up():
    assert len(CALLS) == len(EXPECTED)
    assert set(PARAMS) == {s for s in _lib.SIGNATURES if s.endswith("_batch")}      # every new entry point that launches is here
    for fn, names in PARAMS.items():
        assert len(names.split()) == len(_lib.SIGNATURES[fn][1]), fn
    for (fn, what, _, _), (rc, msg) in zip(CALLS, EXPECTED):
        assert rc != 0 and msg.startswith(fn + ": "), (fn, what)      # nothing in the table may get as far as a launch
    for what in ("no sequences", "too many sequences", "caches that overlap", "seq_stride % 16 bytes", "misaligned key counts", "nine rows"):
        assert {f for f, w, _, _ in CALLS if w == what} >= set(CACHE), what
    for what in ("a workspace for one sequence", "head_dim 64", "null q"):
        assert {f for f, w, _, _ in CALLS if w == what} == set(ATTN), what


@pytest.mark.parametrize("i", range(len(CALLS)), ids=[f"{f[len('mq_'):]}-{what}".replace(" ", "_") for f, what, _, _ in CALLS])
def test_refusal(i):
    fn, what, overrides, force = CALLS[i]
    assert refusal(fn, overrides, force) == EXPECTED[i], (fn, what)


def test_a_batch_of_one_ignores_seq_stride():
    """B = 1 is the sibling: a stride no batch could use is not looked at, and the first thing refused is what the sibling refuses"""
    for fn in CACHE:
        rc, msg = refusal(fn, dict(B=1, seq_stride=7, R=9), None)
        assert rc == EINVAL and "R = 9" in msg, (fn, msg)
