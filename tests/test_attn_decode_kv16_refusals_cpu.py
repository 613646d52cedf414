"""What the 16-bit-cache entry points of the generation step refuse, and in which words: mq_attn_decode and mq_attn_decode_quant_i8
(csrc/attn_decode.hip) with the table of tests/test_attn_decode_refusals_cpu.py minus its scale rows, plus a cache stride that
brings (T + 32) x the row stride IN BYTES to 2^32; mq_kv_append_rope (csrc/kv_append.hip) with the table of
tests/test_kv_append_refusals_cpu.py, its cache rows 16-byte aligned.  The host checks run before anything touches a device: every
call is made with dummy addresses on any machine, and nothing in the tables may reach a launch.  The plan is shared with the e4m3
entry points and does not depend on the storage: its values for two shapes are pinned here."""

import ctypes

import pytest

from mquant_amd import _lib

EINVAL = -1
F16, BF16, F32 = _lib.MQ_F16, _lib.MQ_BF16, _lib.MQ_F32
P = 0x7F0000001000             # a 16-byte aligned address nobody dereferences: every call is refused first
DEC, DECQ, APP = "mq_attn_decode", "mq_attn_decode_quant_i8", "mq_kv_append_rope"

# the parameter names of include/mquant_hip.h, in order
PARAMS = {
    DEC: "q dtype R T n_keys_dev heads kv_heads head_dim ldq kv_cache ldkv softmax_scale causal out ldo workspace workspace_bytes stream",
    DECQ: "q dtype R T n_keys_dev heads kv_heads head_dim ldq kv_cache ldkv softmax_scale causal scale0 scale1 row_sel out K_pad ldo "
          "workspace workspace_bytes stream",
    APP: "qkv dtype R T n_keys_dev rope_delta_dev heads kv_heads head_dim ldqkv cos sin table_rows kv_cache ldkv stream",
}
# well-formed calls: one row of the 7B geometry over 64 keys (one key range: no workspace); a table row overrides what it violates
BASE = {
    DEC: dict(q=P, dtype=F16, R=1, T=64, n_keys_dev=None, heads=28, kv_heads=4, head_dim=128, ldq=28 * 128, kv_cache=P, ldkv=1024,
              softmax_scale=0.088, causal=1, out=P, ldo=28 * 128, workspace=None, workspace_bytes=0, stream=None),
    APP: dict(qkv=P, dtype=F16, R=1, T=64, n_keys_dev=None, rope_delta_dev=None, heads=28, kv_heads=4, head_dim=128, ldqkv=36 * 128,
              cos=P, sin=P, table_rows=64, kv_cache=P, ldkv=1024, stream=None),
}
BASE[DECQ] = dict(BASE[DEC], scale0=0.5, scale1=0.5, row_sel=None, K_pad=28 * 128, ldo=28 * 128)
WS_4096 = 32 * 28 * 130 * 4     # T = 4096 at (28, 4): 32 ranges of 128 keys, one fp32 state (acc[128], m, l) per range and (row, head)
LD_4G = -(-(1 << 32) // ((64 + 32) * 2 * 8)) * 8      # the smallest 16-byte aligned stride with (64 + 32) * ldkv * 2 >= 2^32
assert LD_4G % 8 == 0 and (64 + 32) * LD_4G * 2 >= 1 << 32 > (64 + 32) * (LD_4G - 8) * 2

BOTH = (DEC, DECQ)
# (entry point, what the call violates, overrides of the well-formed call, (splits, keys_per_split) for mq_attn_decode_debug_force or None)
CALLS = (
    [(f, "fp32 q", dict(dtype=F32), None) for f in BOTH]
    + [(f, "unknown dtype", dict(dtype=5), None) for f in BOTH]
    + [(f, "head_dim 64", dict(head_dim=64), None) for f in BOTH]
    + [(f, "no rows", dict(R=0), None) for f in BOTH]
    + [(f, "nine rows", dict(R=9, T=64), None) for f in BOTH]
    + [(f, "fewer keys than rows", dict(R=3, T=2), None) for f in BOTH]
    + [(f, "no keys", dict(T=0), None) for f in BOTH]
    + [(f, "heads % kv_heads", dict(heads=28, kv_heads=8), None) for f in BOTH]
    + [(f, "no kv heads", dict(kv_heads=0), None) for f in BOTH]
    + [(f, "null q", dict(q=None), None) for f in BOTH]
    + [(f, "null cache", dict(kv_cache=None), None) for f in BOTH]
    + [(f, "null out", dict(out=None), None) for f in BOTH]
    + [(f, "ldq < heads * 128", dict(ldq=27 * 128), None) for f in BOTH]
    + [(f, "ldkv < 2 kv_heads * 128", dict(ldkv=1008), None) for f in BOTH]
    + [(DEC, "ldo < heads * 128", dict(ldo=28 * 128 - 4), None)]
    + [(f, "misaligned q", dict(q=P + 8), None) for f in BOTH]
    + [(f, "ldq * 2 % 16", dict(ldq=28 * 128 + 4), None) for f in BOTH]
    + [(f, "misaligned cache", dict(kv_cache=P + 8), None) for f in BOTH]
    + [(f, "ldkv * 2 % 16", dict(ldkv=1028), None) for f in BOTH]
    + [(DEC, "misaligned out", dict(out=P + 4), None),
       (DEC, "ldo * 2 % 8", dict(ldo=28 * 128 + 2), None)]
    + [(f, "misaligned key count", dict(n_keys_dev=P + 2), None) for f in BOTH]
    + [(f, "zero softmax_scale", dict(softmax_scale=0.0), None) for f in BOTH]
    + [(f, "negative softmax_scale", dict(softmax_scale=-0.1), None) for f in BOTH]
    + [(f, "infinite softmax_scale", dict(softmax_scale=float("inf")), None) for f in BOTH]
    + [(f, "NaN softmax_scale", dict(softmax_scale=float("nan")), None) for f in BOTH]
    + [(f, "a stride that reaches 4 GiB", dict(ldkv=LD_4G), None) for f in BOTH]
    + [(f, "no workspace", dict(T=4096), None) for f in BOTH]
    + [(f, "small workspace", dict(T=4096, workspace=P, workspace_bytes=WS_4096 - 1), None) for f in BOTH]
    + [(f, "misaligned workspace", dict(T=4096, workspace=P + 8, workspace_bytes=WS_4096), None) for f in BOTH]
    + [(f, "forced ranges, no workspace", {}, (2, 32)) for f in BOTH]
    + [(f, "forced keys per range 48", {}, (0, 48)) for f in BOTH]
    + [(f, "forced ranges that leave one empty", {}, (3, 32)) for f in BOTH]
    + [(DECQ, "K_pad != heads * 128", dict(K_pad=28 * 128 + 64), None),
       (DECQ, "row stride < K_pad", dict(ldo=28 * 128 - 4), None),
       (DECQ, "row stride % 4", dict(ldo=28 * 128 + 2), None),
       (DECQ, "misaligned out", dict(out=P + 8), None),
       (DECQ, "zero scale", dict(scale0=0.0), None),
       (DECQ, "negative second scale", dict(scale1=-1.0), None)]
    # mq_kv_append_rope: one row per host check
    + [(APP, what, over, None) for what, over in [
        ("null qkv", dict(qkv=None)),
        ("null cache", dict(kv_cache=None)),
        ("fp32 qkv", dict(dtype=F32)),
        ("unknown dtype", dict(dtype=5)),
        ("no rows", dict(R=0)),
        ("nine rows", dict(R=9)),
        ("capacity below the rows", dict(R=3, T=2)),
        ("no capacity", dict(T=0)),
        ("no heads", dict(heads=0)),
        ("no kv heads", dict(kv_heads=0)),
        ("heads % kv_heads", dict(kv_heads=8)),
        ("head_dim 8", dict(head_dim=8)),
        ("head_dim 72", dict(head_dim=72)),
        ("more columns than the grid serves", dict(heads=1 << 22, kv_heads=1, ldqkv=1 << 40)),
        ("ldqkv < (heads + 2 kv_heads) * head_dim", dict(ldqkv=36 * 128 - 8)),
        ("misaligned qkv", dict(qkv=P + 8)),
        ("ldqkv * 2 % 16", dict(ldqkv=36 * 128 + 4)),
        ("ldkv < 2 kv_heads * head_dim", dict(ldkv=1016)),
        ("misaligned cache", dict(kv_cache=P + 8)),
        ("ldkv * 2 % 16", dict(ldkv=1028)),
        ("cos without sin", dict(sin=None)),
        ("sin without cos", dict(cos=None)),
        ("an empty table", dict(table_rows=0)),
        ("misaligned cos", dict(cos=P + 8)),
        ("misaligned sin", dict(sin=P + 8)),
        ("misaligned key count", dict(n_keys_dev=P + 2)),
        ("misaligned position offset", dict(rope_delta_dev=P + 2))]]
)

Q_OUT = f"{DECQ}: out must hold exactly heads * head_dim = 3584 columns (K_pad %d, a multiple of 64), ldo = MQ_LD_TILED or a row stride"


def _both(text):
    return [(EINVAL, f"{f}: {text}") for f in BOTH]


# (status, mq_last_error()) of every row of CALLS, in order
EXPECTED = (
    _both("q / out dtype must be fp16 or bf16 (got 2)")
    + _both("q / out dtype must be fp16 or bf16 (got 5)")
    + _both("head_dim 64 (built for 128)")
    + _both("R = 0 query rows (1 .. 8)")
    + _both("R = 9 query rows (1 .. 8)")
    + _both("T = 2 keys for R = 3 rows (the rows are the last R positions: T >= R)")
    + _both("T = 0 keys for R = 1 rows (the rows are the last R positions: T >= R)")
    + _both("bad head counts 28 / 8")
    + _both("bad head counts 28 / 0")
    + _both("null pointer") * 3
    + _both("row strides too short") * 2
    + [(EINVAL, f"{DEC}: row strides too short")]
    + _both("q / cache rows must be 16-byte aligned, out rows 8-byte aligned") * 4
    + [(EINVAL, f"{DEC}: q / cache rows must be 16-byte aligned, out rows 8-byte aligned")] * 2
    + _both("n_keys_dev must be 4-byte aligned")
    + _both("softmax_scale must be positive and finite (got 0)")
    + _both("softmax_scale must be positive and finite (got -0.1)")
    + _both("softmax_scale must be positive and finite (got inf)")
    + _both("softmax_scale must be positive and finite (got nan)")
    + _both(f"(T + 32) x the cache row stride in bytes must stay below 4 GiB (T 64, stride {LD_4G * 2} bytes)")
    + _both(f"32 key splits need a workspace of {WS_4096} bytes (got 0)")
    + _both(f"32 key splits need a workspace of {WS_4096} bytes (got {WS_4096 - 1})")
    + _both("workspace must be 16-byte aligned")
    + _both(f"2 key splits need a workspace of {2 * 28 * 130 * 4} bytes (got 0)")
    + _both("forced keys_per_split 48 is no multiple of the 32-key block")
    + _both("forced plan of 3 splits of 32 keys does not cut T = 64 keys into non-empty ranges")
    + [(EINVAL, Q_OUT % (28 * 128 + 64)), (EINVAL, Q_OUT % (28 * 128)), (EINVAL, Q_OUT % (28 * 128)), (EINVAL, Q_OUT % (28 * 128)),
       (EINVAL, f"{DECQ}: scales must be positive"), (EINVAL, f"{DECQ}: scales must be positive")]
    + [(EINVAL, f"{APP}: {msg}") for msg in [
        "null pointer",
        "null pointer",
        "qkv dtype must be fp16 or bf16 (got 2)",
        "qkv dtype must be fp16 or bf16 (got 5)",
        "R = 0 new rows (1 .. 8)",
        "R = 9 new rows (1 .. 8)",
        "T = 2 cache rows for R = 3 new rows (the rows are the last R positions: T >= R)",
        "T = 0 cache rows for R = 1 new rows (the rows are the last R positions: T >= R)",
        "bad head counts 0 / 4",
        "bad head counts 28 / 0",
        "bad head counts 28 / 8",
        "head_dim 8 (a multiple of 16)",
        "head_dim 72 (a multiple of 16)",
        f"{((1 << 22) + 2) * 128} columns per row exceed the grid",
        "qkv row stride 4600 shorter than (heads + 2 kv_heads) * head_dim = 4608",
        "qkv rows must be 16-byte aligned",
        "qkv rows must be 16-byte aligned",
        "cache row stride 1016 shorter than 2 kv_heads * head_dim = 1024",
        "cache rows must be 16-byte aligned",
        "cache rows must be 16-byte aligned",
        "cos and sin must both be given or both be null (append only)",
        "cos and sin must both be given or both be null (append only)",
        "table_rows = 0 (at least one row of cos / sin)",
        "cos / sin tables must be 16-byte aligned",
        "cos / sin tables must be 16-byte aligned",
        "n_keys_dev must be 4-byte aligned",
        "rope_delta_dev must be 4-byte aligned"]]
)


def refusal(fn, overrides, force):
    """(status, message) of one call"""
    lib = _lib.load()
    values = {**BASE[fn], **overrides}
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
    for fn, names in PARAMS.items():
        assert len(names.split()) == len(_lib.SIGNATURES[fn][1]) and set(BASE[fn]) == set(names.split()), fn
    for (fn, what, overrides, force), (rc, msg) in zip(CALLS, EXPECTED):
        assert rc != 0 and msg.startswith(fn + ": "), (fn, what)      # nothing in the table may get as far as a launch
        assert (overrides or force) and set(overrides) <= set(BASE[fn]), (fn, what)


@pytest.mark.parametrize("i", range(len(CALLS)), ids=[f"{f[len('mq_'):]}-{what}".replace(" ", "_") for f, what, _, _ in CALLS])
def test_refusal(i):
    fn, what, overrides, force = CALLS[i]
    assert refusal(fn, overrides, force) == EXPECTED[i], (fn, what)


def test_the_largest_stride_below_4_gib_passes_that_check():
    """(T + 32) x stride x 2 one step below 2^32: the call gets past the range check and is refused by the NEXT one (no workspace
    for the forced two ranges) -- the limit is where the table says it is, not below."""
    rc, msg = refusal(DEC, dict(ldkv=LD_4G - 8), (2, 32))
    assert (rc, msg) == (EINVAL, f"{DEC}: 2 key splits need a workspace of {2 * 28 * 130 * 4} bytes (got 0)")


# what mq_attn_decode_debug_plan and mq_attn_decode_workspace_bytes returned before the 16-bit entry points existed (no device: 256
# CUs): (splits, keys_per_split, grid, passes, workspace bytes)
PLANS = {(1, 4096, 28, 4): (32, 128, 128, 1, WS_4096),
         (3, 300, 64, 8): (3, 128, 24, 2, 3 * 3 * 64 * 130 * 4)}


@pytest.mark.parametrize("shape", sorted(PLANS), ids=lambda s: "R%d-T%d-h%dx%d" % s)
def test_the_plan_has_not_moved(shape):
    lib = _lib.load()
    plan = (ctypes.c_int * 5)()
    assert lib.mq_attn_decode_debug_plan(*shape, ctypes.cast(plan, ctypes.c_void_p)) == 0
    assert tuple(plan) == PLANS[shape]
    assert lib.mq_attn_decode_workspace_bytes(*shape) == PLANS[shape][4]
