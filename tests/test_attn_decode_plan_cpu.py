"""The host plan of the decode attention (attn_decode_plan in mquant_amd/csrc/attn_decode.hip, through mq_attn_decode_debug_plan):
its invariants over a sweep of shapes, the forcing hook, the coverage of the GPU case list (tests/attn_decode_cases.py), and the
plan of the six benchmarked shapes.  Host arithmetic only: without a device the CU count is taken as 256."""
import ctypes

import pytest

import attn_decode_cases as cases
from mquant_amd import _lib

KEYS = list(range(1, 131)) + [1000, 4096, 32768, 131072]
PART_BYTES = (128 + 2) * 4          # one partial state: acc[128], m, l in fp32


def plan(R, T, heads, kv_heads, force=(0, 0)):
    """dict of the plan, or None where the call is refused"""
    lib = _lib.load()
    out = (ctypes.c_int * 5)()
    lib.mq_attn_decode_debug_force(*force)
    try:
        rc = lib.mq_attn_decode_debug_plan(R, T, heads, kv_heads, ctypes.cast(out, ctypes.c_void_p))
        ws = lib.mq_attn_decode_workspace_bytes(R, T, heads, kv_heads)
    finally:
        lib.mq_attn_decode_debug_force(0, 0)
    if rc != 0:
        return None
    return dict(zip(("splits", "keys_per_split", "grid", "passes", "workspace_bytes"), out), queried=ws)


def check_invariants(p, R, T, heads, kv_heads):
    assert p["splits"] >= 1
    assert p["keys_per_split"] >= cases.KEY_BLOCK and p["keys_per_split"] % cases.KEY_BLOCK == 0
    assert p["splits"] * p["keys_per_split"] >= T > (p["splits"] - 1) * p["keys_per_split"]
    assert p["grid"] == p["splits"] * kv_heads
    assert p["passes"] == -(-(R * heads // kv_heads) // cases.ROWS_PER_PASS)
    assert p["workspace_bytes"] == p["queried"]
    assert (p["workspace_bytes"] == 0) == (p["splits"] == 1)
    if p["splits"] > 1:
        assert p["workspace_bytes"] == p["splits"] * R * heads * PART_BYTES


@pytest.mark.parametrize("heads,kv_heads", cases.HEADS)
@pytest.mark.parametrize("R", [1, 2, 8])
def test_plan_invariants(R, heads, kv_heads):
    for T in KEYS:
        p = plan(R, T, heads, kv_heads)
        if T < R:
            assert p is None
            continue
        check_invariants(p, R, T, heads, kv_heads)


@pytest.mark.parametrize("heads,kv_heads", cases.HEADS)
def test_the_forcing_hook_is_honoured(heads, kv_heads):
    for T in KEYS:
        for force in [(1, 0), (2, 0), (3, 0), (7, 0), (0, 32), (0, 64), (0, 4096), (8, 64), (2, 32)]:
            p = plan(1, T, heads, kv_heads, force)
            if cases.plan_is_refused(T, force):
                assert p is None, (T, force)
                continue
            check_invariants(p, 1, T, heads, kv_heads)
            if force[0]:
                assert p["splits"] == force[0], (T, force)
            if force[1]:
                assert p["keys_per_split"] == force[1], (T, force)
    assert plan(1, 64, heads, kv_heads, (0, 48)) is None                 # no multiple of the key block
    assert plan(1, 64, heads, kv_heads) == plan(1, 64, heads, kv_heads)  # and the hook is reset: the heuristic again


def test_the_gpu_cases_reach_every_path_of_the_launch():
    plans = [plan(c["R"], c["n"], c["heads"], c["kv_heads"]) for c in cases.HEURISTIC]
    assert all(p is not None for p in plans)
    assert any(p["splits"] == 1 for p in plans) and any(p["splits"] > 1 for p in plans)
    assert any(p["passes"] == 1 for p in plans) and any(p["passes"] > 1 for p in plans)
    assert any(p["splits"] > 1 and p["passes"] > 1 for p in plans)
    long = plan(cases.LONG["R"], cases.LONG["n"], cases.LONG["heads"], cases.LONG["kv_heads"])
    assert long["splits"] > 8 and long["keys_per_split"] < cases.LONG["n"]
    # every case of the lists is accepted with its own plan, and the forced ones get what they ask for
    for c in cases.PARITY + cases.ROWS + [cases.LONG]:
        p = plan(c["R"], c["n"], c["heads"], c["kv_heads"], c["plan"])
        assert p is not None, cases.case_id(c)
        assert c["plan"][0] in (0, p["splits"]) and c["plan"][1] in (0, p["keys_per_split"])
    forced = {p["plan"] for p in cases.PARITY}
    assert {(0, 0), (1, 0), (2, 0), (3, 0), (0, cases.KEY_BLOCK)} <= forced
    assert any(c["R"] * c["heads"] // c["kv_heads"] > cases.ROWS_PER_PASS and c["plan"] == (3, 0) for c in cases.ROWS)


# The plans profiles/decode_attn_bench.txt was measured with (R = 1, 256 CUs): (heads, kv_heads, n) -> (splits, keys_per_split).
# A change of the heuristic shows here and asks for the measurement to be repeated.
BENCHMARKED = {
    (28, 4, 768): (6, 128), (28, 4, 4096): (32, 128), (28, 4, 32768): (128, 256),
    (64, 8, 768): (6, 128), (64, 8, 4096): (32, 128), (64, 8, 32768): (64, 512),
}


@pytest.mark.parametrize("shape", sorted(BENCHMARKED), ids=lambda s: f"h{s[0]}x{s[1]}-n{s[2]}")
def test_the_plan_of_the_benchmarked_shapes(shape):
    heads, kv_heads, n = shape
    p = plan(1, n, heads, kv_heads)
    assert (p["splits"], p["keys_per_split"]) == BENCHMARKED[shape]
    assert p["passes"] == 1
