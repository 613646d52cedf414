"""What mq_gemv_f16_argmax refuses, and in which words (csrc/gemv_f16.hip), in the table form of
tests/test_kv_append_refusals_cpu.py: the host checks run before anything touches a device, so every call here is made with dummy
addresses on any machine -- one violating call per host check, each with the status and the mq_last_error() text it must produce.
Nothing in the table may reach a launch, and the well-formed call itself is never made.  Then mq_gemv_argmax_workspace_bytes, which
is host arithmetic only."""

import pytest

from mquant_amd import _lib

EINVAL = -1
F16, BF16, F32 = _lib.MQ_F16, _lib.MQ_BF16, _lib.MQ_F32
P = 0x7F0000001000             # a 16-byte aligned address nobody dereferences: every call is refused first
FN = "mq_gemv_f16_argmax"

# the parameter names of include/mquant_hip.h, in order
PARAMS = "x dtype M K ldx w N ldw logits ldo token_out workspace workspace_bytes stream"
# a well-formed call: one row against the 7B lm_head, no logits; a table row overrides what it violates
BASE = dict(x=P, dtype=F16, M=1, K=3584, ldx=3584, w=P, N=152064, ldw=3584, logits=None, ldo=0, token_out=P, workspace=P,
            workspace_bytes=1 << 20, stream=None)
COLUMNS = "columns (1 .. 2^31 - 1: an argmax over nothing has no token, and the token is an int32)"

# (what the call violates, overrides of the well-formed call, mq_last_error() without the entry point's name)
TABLE = [
    ("fp32 operands", dict(dtype=F32), "dtype must be fp16 or bf16 (got 2)"),
    ("unknown dtype", dict(dtype=7), "dtype must be fp16 or bf16 (got 7)"),
    ("nine rows", dict(M=9), "M must be 0..8 and K a positive multiple of 8 (M 9, N 152064, K 3584)"),
    ("negative rows", dict(M=-1), "M must be 0..8 and K a positive multiple of 8 (M -1, N 152064, K 3584)"),
    ("K % 8", dict(K=60, ldx=64, ldw=64), "M must be 0..8 and K a positive multiple of 8 (M 1, N 152064, K 60)"),
    ("no K", dict(K=0), "M must be 0..8 and K a positive multiple of 8 (M 1, N 152064, K 0)"),
    ("negative N", dict(N=-4), "M must be 0..8 and K a positive multiple of 8 (M 1, N -4, K 3584)"),
    ("null x", dict(x=None), "null pointer"),
    ("null W", dict(w=None), "null pointer"),
    ("ldx < K", dict(ldx=3576), "row strides too short"),
    ("ldw < K", dict(ldw=3576), "row strides too short"),
    ("ldo < N with logits", dict(logits=P, ldo=152063), "row strides too short"),
    ("misaligned x", dict(x=P + 8), "x / W rows must be 16-byte aligned"),
    ("ldx * 2 % 16", dict(M=2, ldx=3588), "x / W rows must be 16-byte aligned"),
    ("misaligned W", dict(w=P + 2), "x / W rows must be 16-byte aligned"),
    ("ldw * 2 % 16", dict(ldw=3588), "x / W rows must be 16-byte aligned"),
    ("x beyond the LDS", dict(M=8, K=8192, ldx=8192, ldw=8192), "x (8 x 8192) must fit 64 KiB of LDS"),
    ("an argmax over nothing", dict(N=0), f"N = 0 {COLUMNS}"),
    ("an argmax over nothing, logits given", dict(N=0, logits=P), f"N = 0 {COLUMNS}"),
    ("more columns than an int32 names", dict(N=1 << 31), f"N = {1 << 31} {COLUMNS}"),
    ("null token_out", dict(token_out=None), "token_out is null"),
    ("misaligned token_out", dict(token_out=P + 2), "token_out must be 4-byte aligned"),
    ("null workspace", dict(workspace=None), "workspace is null (16384 bytes needed)"),
    ("misaligned workspace", dict(workspace=P + 8), "workspace must be 16-byte aligned"),
    ("a workspace one byte short", dict(workspace_bytes=16383), "the workspace needs 16384 bytes (got 16383)"),
    ("a workspace sized for fewer rows", dict(M=8, workspace_bytes=16384), "the workspace needs 131072 bytes (got 16384)"),
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


def test_no_rows_is_ok_and_touches_nothing():
    """M == 0 returns MQ_OK before any pointer is looked at (the addresses are dummies: a launch would fault)"""
    lib = _lib.load()
    values = {**BASE, "M": 0, "token_out": None, "workspace": None, "workspace_bytes": 0}
    assert getattr(lib, FN)(*[values[name] for name in PARAMS.split()]) == 0


# ---- mq_gemv_argmax_workspace_bytes: workgroups of the launch plan x M x 8, rounded up to 16
def ws(M, N):
    return int(_lib.load().mq_gemv_argmax_workspace_bytes(M, N))


@pytest.mark.parametrize("M,N", [(0, 100), (-1, 100), (9, 100), (1, 0), (1, -5), (8, 1 << 31), (0, 0)])
def test_workspace_is_zero_for_what_the_call_refuses(M, N):
    assert ws(M, N) == 0


@pytest.mark.parametrize("N", [1, 3, 5, 1001, 4099, 70001, 92553, 152064, (1 << 31) - 1])
def test_workspace_is_a_positive_multiple_of_16_and_grows_with_the_rows(N):
    sizes = [ws(M, N) for M in range(1, 9)]
    assert all(s > 0 and s % 16 == 0 for s in sizes), sizes
    assert sizes == sorted(sizes), sizes


@pytest.mark.parametrize("N,blocks", [(1, 1), (4, 1), (16, 1), (17, 2), (1001, 63), (4099, 257)])
def test_workspace_of_a_matrix_that_leaves_wave_slots_free(N, blocks):
    """below CUs x 8 workgroups the grid is one workgroup per four waves' rows, ceil(ceil(N / 4) / 4), whatever the chip's CU count"""
    for M in range(1, 9):
        assert ws(M, N) == (blocks * M * 8 + 15) // 16 * 16


def test_workspace_stops_growing_once_the_chip_is_full():
    """every wave slot taken: more rows of W do not add workgroups"""
    assert ws(1, 152064) == ws(1, 92553) == ws(1, (1 << 31) - 1)
