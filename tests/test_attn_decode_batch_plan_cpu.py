"""The host plan of the BATCHED decode attention (attn_decode_plan in mquant_amd/csrc/attn_decode.hip, through
mq_attn_decode_batch_debug_plan): B = 1 is the single-sequence plan slot for slot, B > 1 only divides the number of key ranges the
heuristic wants per sequence -- want = max(1, 2 CUs / (kv_heads B)) -- and multiplies the grid and the workspace; forced plans pass
through unchanged.  Host arithmetic only: without a device the CU count is taken as 256."""
import ctypes

import pytest

import attn_decode_cases as cases
from mquant_amd import _lib

CUS = 256
PART_BYTES = (128 + 2) * 4          # one partial state: acc[128], m, l in fp32
SLOTS = ("splits", "keys_per_split", "grid", "passes", "workspace_bytes")
SHAPES = sorted({(c["R"], c["n"], c["heads"], c["kv_heads"]) for c in cases.PARITY + cases.ROWS + cases.HEURISTIC}
                | {(1, 32768, 28, 4), (8, 4096, 64, 8)})


def ceil_div(a, b):
    return -(-a // b)


def single_plan(R, T, heads, kv_heads, force=(0, 0)):
    lib = _lib.load()
    out = (ctypes.c_int * 5)()
    lib.mq_attn_decode_debug_force(*force)
    try:
        rc = lib.mq_attn_decode_debug_plan(R, T, heads, kv_heads, ctypes.cast(out, ctypes.c_void_p))
    finally:
        lib.mq_attn_decode_debug_force(0, 0)
    return None if rc != 0 else dict(zip(SLOTS, out))


def batch_plan(B, R, T, heads, kv_heads, force=(0, 0)):
    """dict of the plan (and the workspace query's answer), or None where the call is refused"""
    lib = _lib.load()
    out = (ctypes.c_int * 5)()
    lib.mq_attn_decode_debug_force(*force)
    try:
        rc = lib.mq_attn_decode_batch_debug_plan(B, R, T, heads, kv_heads, ctypes.cast(out, ctypes.c_void_p))
        ws = lib.mq_attn_decode_batch_workspace_bytes(B, R, T, heads, kv_heads)
    finally:
        lib.mq_attn_decode_debug_force(0, 0)
    return None if rc != 0 else dict(zip(SLOTS, out), queried=ws)


def expected_splits(B, T, kv_heads):
    """the heuristic of the issue, restated: (splits, keys per split)"""
    want = max(1, 2 * CUS // (kv_heads * B))
    kps = max(ceil_div(ceil_div(T, want), cases.KEY_BLOCK) * cases.KEY_BLOCK, 4 * cases.KEY_BLOCK)
    return ceil_div(T, kps), kps


def test_the_shapes_cover_the_case_list_and_the_two_long_ones():
    assert (1, 32768, 28, 4) in SHAPES and (8, 4096, 64, 8) in SHAPES
    assert {(c["R"], c["n"], c["heads"], c["kv_heads"]) for c in cases.PARITY + cases.ROWS + [cases.LONG]} <= set(SHAPES)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R%d-T%d-h%dx%d" % s)
def test_a_batch_of_one_is_the_single_sequence_plan(shape):
    single = single_plan(*shape)
    assert single is not None
    got = batch_plan(1, *shape)
    assert {k: got[k] for k in SLOTS} == single
    assert got["queried"] == single["workspace_bytes"] == _lib.load().mq_attn_decode_workspace_bytes(*shape)
    for force in [(1, 0), (3, 0), (0, 32), (0, 128)]:
        a, b = single_plan(*shape, force), batch_plan(1, *shape, force)
        assert (a is None) == (b is None), force
        if a is not None:
            assert {k: b[k] for k in SLOTS} == a, force


@pytest.mark.parametrize("B", [2, 4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R%d-T%d-h%dx%d" % s)
def test_the_heuristic_divides_the_chip_among_the_sequences(shape, B):
    R, T, heads, kv_heads = shape
    p = batch_plan(B, *shape)
    splits, kps = expected_splits(B, T, kv_heads)
    assert (p["splits"], p["keys_per_split"]) == (splits, kps)
    assert p["grid"] == kv_heads * splits * B
    assert p["passes"] == ceil_div(R * heads // kv_heads, cases.ROWS_PER_PASS)
    assert p["workspace_bytes"] == p["queried"] == (B * splits * R * heads * PART_BYTES if splits > 1 else 0)
    assert splits * kps >= T > (splits - 1) * kps


def test_more_sequences_never_mean_more_ranges_per_sequence():
    for shape in [(1, 32768, 28, 4), (8, 4096, 64, 8), (1, 768, 28, 4)]:
        splits = [batch_plan(B, *shape)["splits"] for B in (1, 2, 4, 8, 64, 1024)]
        assert splits == sorted(splits, reverse=True) and splits[-1] >= 1, (shape, splits)
    # 28 / 4 at 32768 keys: 128 ranges of 256 keys alone, 16 ranges of 2048 keys at B = 8 -- 512 workgroups either way
    assert [batch_plan(B, 1, 32768, 28, 4)["grid"] for B in (1, 8)] == [512, 512]


@pytest.mark.parametrize("B", [1, 2, 6, 8])
def test_forced_plans_pass_through_unchanged(B):
    for shape in [(1, 320, 28, 4), (3, 320, 4, 2), (1, 4096, 64, 8)]:
        R, T, heads, kv_heads = shape
        for force in [(1, 0), (2, 0), (3, 0), (0, 32), (0, 128), (0, 4096), (8, 64)]:
            p = batch_plan(B, *shape, force)
            if cases.plan_is_refused(T, force):
                assert p is None, (shape, force)
                continue
            single = single_plan(*shape, force)
            assert (p["splits"], p["keys_per_split"], p["passes"]) == (single["splits"], single["keys_per_split"], single["passes"])
            assert p["grid"] == B * single["grid"] and p["workspace_bytes"] == p["queried"] == B * single["workspace_bytes"]
            if force[0]:
                assert p["splits"] == force[0]
            if force[1]:
                assert p["keys_per_split"] == force[1]
    assert batch_plan(B, 1, 64, 28, 4, (0, 48)) is None                  # no multiple of the key block


def test_what_the_plan_refuses():
    lib = _lib.load()
    out = (ctypes.c_int * 5)()
    ptr = ctypes.cast(out, ctypes.c_void_p)
    for B, text in [(0, "B = 0 sequences (1 .. 65535: the second grid dimension)"),
                    (65536, "B = 65536 sequences (1 .. 65535: the second grid dimension)")]:
        assert lib.mq_attn_decode_batch_debug_plan(B, 1, 64, 28, 4, ptr) == -1
        assert lib.mq_last_error().decode() == "mq_attn_decode_batch_debug_plan: " + text
        assert lib.mq_attn_decode_batch_workspace_bytes(B, 1, 4096, 28, 4) == 0
    assert lib.mq_attn_decode_batch_debug_plan(2, 1, 64, 28, 4, None) == -1
    assert lib.mq_last_error().decode() == "mq_attn_decode_batch_debug_plan: null pointer"
    assert lib.mq_attn_decode_batch_debug_plan(2, 9, 64, 28, 4, ptr) == -1
    assert lib.mq_last_error().decode() == "mq_attn_decode_batch_debug_plan: R = 9 query rows (1 .. 8)"
    assert lib.mq_attn_decode_batch_debug_plan(65535, 1, 64, 28, 4, ptr) == 0 and out[2] == 65535 * 4
