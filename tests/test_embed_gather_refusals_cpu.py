"""What mq_embed_gather refuses, and in which words (csrc/embed.hip), in the table form of tests/test_kv_append_refusals_cpu.py: the
host checks run before anything touches a device, so every call here is made with dummy addresses on any machine -- one violating
call per host check, each with the status and the mq_last_error() text it must produce.  Nothing in the table may reach a launch,
and the well-formed call itself is never made."""

import pytest

from mquant_amd import _lib

EINVAL = -1
F16, BF16, F32 = _lib.MQ_F16, _lib.MQ_BF16, _lib.MQ_F32
P = 0x7F0000001000             # a 16-byte aligned address nobody dereferences: every call is refused first
FN = "mq_embed_gather"

# the parameter names of include/mquant_hip.h, in order
PARAMS = "table dtype vocab dim ldt ids_dev R out ldo id_log log_rows n_keys_dev stream"
# a well-formed call: one row of the 7B embedding, logged at a device-side position; a table row overrides what it violates
BASE = dict(table=P, dtype=F16, vocab=152064, dim=3584, ldt=3584, ids_dev=P, R=1, out=P, ldo=3584, id_log=P, log_rows=64, n_keys_dev=P,
            stream=None)

# (what the call violates, overrides of the well-formed call, mq_last_error() without the entry point's name)
TABLE = [
    ("null table", dict(table=None), "null pointer"),
    ("null ids", dict(ids_dev=None), "null pointer"),
    ("null out", dict(out=None), "null pointer"),
    ("fp32 table", dict(dtype=F32), "dtype must be fp16 or bf16 (got 2)"),
    ("unknown dtype", dict(dtype=-3), "dtype must be fp16 or bf16 (got -3)"),
    ("no rows", dict(R=0), "R = 0 rows (1 .. 8)"),
    ("nine rows", dict(R=9, log_rows=64), "R = 9 rows (1 .. 8)"),
    ("an empty table", dict(vocab=0), "vocab = 0 table rows (1 .. 2^31 - 1: the ids are int32)"),
    ("more rows than an int32 names", dict(vocab=1 << 31), f"vocab = {1 << 31} table rows (1 .. 2^31 - 1: the ids are int32)"),
    ("no columns", dict(dim=0), "dim = 0 (a positive multiple of 8, at most 2^31)"),
    ("dim % 8", dict(dim=3580), "dim = 3580 (a positive multiple of 8, at most 2^31)"),
    ("more columns than the grid serves", dict(dim=(1 << 31) + 8, ldt=1 << 40, ldo=1 << 40),
     f"dim = {(1 << 31) + 8} (a positive multiple of 8, at most 2^31)"),
    ("ldt < dim", dict(ldt=3576), "table row stride 3576 shorter than dim = 3584"),
    ("ldo < dim", dict(ldo=3576), "out row stride 3576 shorter than dim = 3584"),
    ("misaligned table", dict(table=P + 8), "table rows must be 16-byte aligned"),
    ("ldt * 2 % 16", dict(ldt=3588), "table rows must be 16-byte aligned"),
    ("misaligned out", dict(out=P + 4), "out rows must be 16-byte aligned"),
    ("ldo * 2 % 16", dict(R=2, ldo=3588), "out rows must be 16-byte aligned"),
    ("misaligned ids", dict(ids_dev=P + 2), "ids_dev must be 4-byte aligned"),
    ("a log shorter than the rows", dict(R=3, log_rows=2),
     "log_rows = 2 entries for R = 3 rows (the rows are the last R positions: log_rows >= R)"),
    ("an empty log", dict(log_rows=0), "log_rows = 0 entries for R = 1 rows (the rows are the last R positions: log_rows >= R)"),
    ("misaligned log", dict(id_log=P + 2), "id_log must be 4-byte aligned"),
    ("misaligned key count", dict(n_keys_dev=P + 2), "n_keys_dev must be 4-byte aligned"),
    ("misaligned key count without a log", dict(id_log=None, n_keys_dev=P + 1), "n_keys_dev must be 4-byte aligned"),
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
