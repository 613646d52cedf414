"""What mq_kv_append_rope_fp8 refuses, and in which words (csrc/kv_append.hip), in the style of
tests/test_attn_decode_refusals_cpu.py: the host checks run before anything touches a device, so every call here is made with
dummy addresses on any machine -- a table with one violating call per host check, each with the status and the mq_last_error()
text it must produce.  Nothing in the table may reach a launch, and the well-formed call itself is never made."""

import pytest

from mquant_amd import _lib

EINVAL = -1
F16, BF16, F32 = _lib.MQ_F16, _lib.MQ_BF16, _lib.MQ_F32
P = 0x7F0000001000             # a 16-byte aligned address nobody dereferences: every call is refused first
FN = "mq_kv_append_rope_fp8"

# the parameter names of include/mquant_hip.h, in order
PARAMS = "qkv dtype R T n_keys_dev rope_delta_dev heads kv_heads head_dim ldqkv cos sin table_rows kv_cache ldkv kv_scale stream"
# a well-formed call: one row of the 7B geometry into a cache of 64 rows; a table row overrides what it violates
BASE = dict(qkv=P, dtype=F16, R=1, T=64, n_keys_dev=None, rope_delta_dev=None, heads=28, kv_heads=4, head_dim=128, ldqkv=36 * 128,
            cos=P, sin=P, table_rows=64, kv_cache=P, ldkv=1024, kv_scale=P, stream=None)

# (what the call violates, overrides of the well-formed call, mq_last_error() without the entry point's name)
TABLE = [
    ("null qkv", dict(qkv=None), "null pointer"),
    ("null cache", dict(kv_cache=None), "null pointer"),
    ("null scales", dict(kv_scale=None), "null pointer"),
    ("fp32 qkv", dict(dtype=F32), "qkv dtype must be fp16 or bf16 (got 2)"),
    ("unknown dtype", dict(dtype=5), "qkv dtype must be fp16 or bf16 (got 5)"),
    ("no rows", dict(R=0), "R = 0 new rows (1 .. 8)"),
    ("nine rows", dict(R=9), "R = 9 new rows (1 .. 8)"),
    ("capacity below the rows", dict(R=3, T=2), "T = 2 cache rows for R = 3 new rows (the rows are the last R positions: T >= R)"),
    ("no capacity", dict(T=0), "T = 0 cache rows for R = 1 new rows (the rows are the last R positions: T >= R)"),
    ("no heads", dict(heads=0), "bad head counts 0 / 4"),
    ("no kv heads", dict(kv_heads=0), "bad head counts 28 / 0"),
    ("heads % kv_heads", dict(kv_heads=8), "bad head counts 28 / 8"),
    ("head_dim 8", dict(head_dim=8), "head_dim 8 (a multiple of 16)"),
    ("head_dim 72", dict(head_dim=72), "head_dim 72 (a multiple of 16)"),
    ("more columns than the grid serves", dict(heads=1 << 22, kv_heads=1, ldqkv=1 << 40),
     f"{((1 << 22) + 2) * 128} columns per row exceed the grid"),
    ("ldqkv < (heads + 2 kv_heads) * head_dim", dict(ldqkv=36 * 128 - 8),
     "qkv row stride 4600 shorter than (heads + 2 kv_heads) * head_dim = 4608"),
    ("misaligned qkv", dict(qkv=P + 8), "qkv rows must be 16-byte aligned"),
    ("ldqkv * 2 % 16", dict(ldqkv=36 * 128 + 4), "qkv rows must be 16-byte aligned"),
    ("ldkv < 2 kv_heads * head_dim", dict(ldkv=1016), "cache row stride 1016 shorter than 2 kv_heads * head_dim = 1024"),
    ("misaligned cache", dict(kv_cache=P + 4), "cache rows must be 8-byte aligned"),
    ("ldkv % 8", dict(ldkv=1028), "cache rows must be 8-byte aligned"),
    ("cos without sin", dict(sin=None), "cos and sin must both be given or both be null (append only)"),
    ("sin without cos", dict(cos=None), "cos and sin must both be given or both be null (append only)"),
    ("an empty table", dict(table_rows=0), "table_rows = 0 (at least one row of cos / sin)"),
    ("misaligned cos", dict(cos=P + 8), "cos / sin tables must be 16-byte aligned"),
    ("misaligned sin", dict(sin=P + 8), "cos / sin tables must be 16-byte aligned"),
    ("misaligned key count", dict(n_keys_dev=P + 2), "n_keys_dev must be 4-byte aligned"),
    ("misaligned position offset", dict(rope_delta_dev=P + 2), "rope_delta_dev must be 4-byte aligned"),
]


def refusal(overrides):
    """(status, message) of one call"""
    lib = _lib.load()
    values = {**BASE, **overrides}
    rc = getattr(lib, FN)(*[values[name] for name in PARAMS.split()])
    return rc, lib.mq_last_error().decode()


def test_the_table_lines_up_with_the_binding():
    assert len(PARAMS.split()) == len(_lib.SIGNATURES[FN][1])
    assert set(BASE) == set(PARAMS.split())
    for what, overrides, msg in TABLE:
        assert overrides and set(overrides) <= set(BASE) and msg, what      # every row violates something: none gets as far as a launch


@pytest.mark.parametrize("i", range(len(TABLE)), ids=[what.replace(" ", "_") for what, _, _ in TABLE])
def test_refusal(i):
    what, overrides, msg = TABLE[i]
    assert refusal(overrides) == (EINVAL, f"{FN}: {msg}"), what
