"""What the decode attention entry points refuse, and in which words (csrc/attn_decode.hip), in the style of
tests/test_gemm_refusals_cpu.py: the host checks run before anything touches a device, so every call here is made with dummy
addresses on any machine -- a table of violating calls, each with the status and the mq_last_error() text it must produce.
Nothing in the table may reach a launch."""

import pytest

from mquant_amd import _lib

EINVAL = -1
F16, BF16, F32 = _lib.MQ_F16, _lib.MQ_BF16, _lib.MQ_F32
TILED = 0                      # MQ_LD_TILED
P = 0x7F0000001000             # a 16-byte aligned address nobody dereferences: every call is refused first
DEC, DECQ = "mq_attn_decode_fp8kv", "mq_attn_decode_fp8kv_quant_i8"

# the parameter names of include/mquant_hip.h, in order
PARAMS = {
    DEC: "q dtype R T n_keys_dev heads kv_heads head_dim ldq kv_cache ldkv kv_scale softmax_scale causal out ldo workspace workspace_bytes stream",
    DECQ: "q dtype R T n_keys_dev heads kv_heads head_dim ldq kv_cache ldkv kv_scale softmax_scale causal scale0 scale1 row_sel out K_pad ldo "
          "workspace workspace_bytes stream",
}
# a well-formed call: one row of the 7B geometry over 64 keys (one key range: no workspace); a table row overrides what it violates
BASE = dict(q=P, dtype=F16, R=1, T=64, n_keys_dev=None, heads=28, kv_heads=4, head_dim=128, ldq=28 * 128, kv_cache=P, ldkv=1024, kv_scale=P,
            softmax_scale=0.088, causal=1, out=P, ldo=28 * 128, workspace=None, workspace_bytes=0, stream=None)
PER_FN = {DECQ: dict(scale0=0.5, scale1=0.5, row_sel=None, K_pad=28 * 128, ldo=28 * 128)}
WS_4096 = 32 * 28 * 130 * 4     # T = 4096 at (28, 4): 32 ranges of 128 keys, one fp32 state (acc[128], m, l) per range and (row, head)

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
    + [(f, "null scales", dict(kv_scale=None), None) for f in BOTH]
    + [(f, "null out", dict(out=None), None) for f in BOTH]
    + [(f, "ldq < heads * 128", dict(ldq=27 * 128), None) for f in BOTH]
    + [(f, "ldkv < 2 kv_heads * 128", dict(ldkv=1008), None) for f in BOTH]
    + [(DEC, "ldo < heads * 128", dict(ldo=28 * 128 - 4), None)]
    + [(f, "misaligned q", dict(q=P + 8), None) for f in BOTH]
    + [(f, "ldq * 2 % 16", dict(ldq=28 * 128 + 4), None) for f in BOTH]
    + [(f, "misaligned cache", dict(kv_cache=P + 8), None) for f in BOTH]
    + [(f, "ldkv % 16", dict(ldkv=1032), None) for f in BOTH]
    + [(DEC, "misaligned out", dict(out=P + 4), None),
       (DEC, "ldo * 2 % 8", dict(ldo=28 * 128 + 2), None)]
    + [(f, "misaligned key count", dict(n_keys_dev=P + 2), None) for f in BOTH]
    + [(f, "zero softmax_scale", dict(softmax_scale=0.0), None) for f in BOTH]
    + [(f, "negative softmax_scale", dict(softmax_scale=-0.1), None) for f in BOTH]
    + [(f, "infinite softmax_scale", dict(softmax_scale=float("inf")), None) for f in BOTH]
    + [(f, "NaN softmax_scale", dict(softmax_scale=float("nan")), None) for f in BOTH]
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
    + _both("null pointer") * 4
    + _both("row strides too short") * 2
    + [(EINVAL, f"{DEC}: row strides too short")]
    + _both("q / cache rows must be 16-byte aligned, out rows 8-byte aligned") * 4
    + [(EINVAL, f"{DEC}: q / cache rows must be 16-byte aligned, out rows 8-byte aligned")] * 2
    + _both("n_keys_dev must be 4-byte aligned")
    + _both("softmax_scale must be positive and finite (got 0)")
    + _both("softmax_scale must be positive and finite (got -0.1)")
    + _both("softmax_scale must be positive and finite (got inf)")
    + _both("softmax_scale must be positive and finite (got nan)")
    + _both(f"32 key splits need a workspace of {WS_4096} bytes (got 0)")
    + _both(f"32 key splits need a workspace of {WS_4096} bytes (got {WS_4096 - 1})")
    + _both("workspace must be 16-byte aligned")
    + _both(f"2 key splits need a workspace of {2 * 28 * 130 * 4} bytes (got 0)")
    + _both("forced keys_per_split 48 is no multiple of the 32-key block")
    + _both("forced plan of 3 splits of 32 keys does not cut T = 64 keys into non-empty ranges")
    + [(EINVAL, Q_OUT % (28 * 128 + 64)), (EINVAL, Q_OUT % (28 * 128)), (EINVAL, Q_OUT % (28 * 128)), (EINVAL, Q_OUT % (28 * 128)),
       (EINVAL, f"{DECQ}: scales must be positive"), (EINVAL, f"{DECQ}: scales must be positive")]
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
    for fn, names in PARAMS.items():
        assert len(names.split()) == len(_lib.SIGNATURES[fn][1]), fn
    for (fn, what, _, _), (rc, msg) in zip(CALLS, EXPECTED):
        assert rc != 0 and msg.startswith(fn + ": "), (fn, what)      # nothing in the table may get as far as a launch


@pytest.mark.parametrize("i", range(len(CALLS)), ids=[f"{f[len('mq_attn_'):]}-{what}".replace(" ", "_") for f, what, _, _ in CALLS])
def test_refusal(i):
    fn, what, overrides, force = CALLS[i]
    assert refusal(fn, overrides, force) == EXPECTED[i], (fn, what)


def test_the_workspace_query_and_the_plan_refuse_without_a_device():
    lib = _lib.load()
    assert lib.mq_attn_decode_workspace_bytes(1, 64, 28, 4) == 0
    assert lib.mq_attn_decode_workspace_bytes(1, 4096, 28, 4) == WS_4096
    assert lib.mq_attn_decode_workspace_bytes(9, 4096, 28, 4) == 0          # what the call refuses needs no workspace
    assert lib.mq_attn_decode_debug_plan(1, 64, 28, 4, None) == EINVAL
    assert lib.mq_last_error().decode() == "mq_attn_decode_debug_plan: null pointer"
    assert lib.mq_attn_decode_debug_force(-1, 0) == EINVAL
