"""The case list of the GEMM sweep (gemm_cases.py) against the default plan (csrc/gemm_w4a8.hip make_plan, host arithmetic): for
every activation layout, weight width and workspace presence the cases reach exactly the (tile, split-K?) pairs the plan can
return, so a plan change that leaves a kernel unswept -- or starts to select one the sweep does not know -- fails here."""
import pytest

import gemm_cases as gc

PIPE, WS64, WS96, WS128, WS192 = 20, 53, 54, 51, 52      # the 256 x 256 ping-pong tile; the wave-specialised tiles (slab-free epilogue)
SK, SK_WG = 60, 61                                      # weight-streaming kernels: one wave per pair / eight waves per pair
ONE, SPLIT = False, True

EXPECTED = {
    # (a_tiled, w_bits, workspace): {(tile, splits > 1)}
    (True, 4, True): {(SK, ONE), (SK, SPLIT), (SK_WG, ONE), (SK_WG, SPLIT), (WS64, ONE), (WS96, ONE), (WS128, ONE), (WS192, ONE),
                      (PIPE, ONE), (WS64, SPLIT), (3, SPLIT)},
    (True, 4, False): {(SK, ONE), (SK_WG, ONE), (WS64, ONE), (WS96, ONE), (WS128, ONE), (WS192, ONE), (PIPE, ONE)},
    (True, 8, True): {(WS64, ONE), (WS96, ONE), (WS128, ONE), (3, ONE), (WS64, SPLIT), (3, SPLIT)},
    (True, 8, False): {(WS64, ONE), (WS96, ONE), (WS128, ONE), (3, ONE)},
    (False, 4, True): {(10, ONE), (31, ONE), (26, ONE), (35, ONE), (2, ONE), (3, ONE), (3, SPLIT)},
    (False, 4, False): {(10, ONE), (31, ONE), (26, ONE), (35, ONE), (2, ONE), (3, ONE)},
    (False, 8, True): {(10, ONE), (31, ONE), (26, ONE), (2, ONE), (3, ONE), (3, SPLIT)},
    (False, 8, False): {(10, ONE), (31, ONE), (26, ONE), (2, ONE), (3, ONE)},
}


def kernel(c, have_ws):
    tile, splits = gc.plan(c.M, c.N, c.K_pad, c.w_bits, c.a_tiled, have_ws)
    return tile, splits > 1


def reached(cases, a_tiled, w_bits, have_ws):
    out = {}
    for c in cases:
        if (c.a_tiled, c.w_bits) == (a_tiled, w_bits):
            out.setdefault(kernel(c, have_ws), []).append(c.name)
    return out


@pytest.mark.parametrize("a_tiled,w_bits,have_ws", sorted(EXPECTED))
def test_the_cases_reach_every_kernel_the_plan_can_return(a_tiled, w_bits, have_ws):
    got = reached(gc.CASES, a_tiled, w_bits, have_ws)
    assert set(got) == EXPECTED[(a_tiled, w_bits, have_ws)], {k: v[:2] for k, v in got.items()}


def test_dropping_the_cases_of_one_kernel_is_noticed():
    """The check above is not vacuous: without the cases the plan sends to one kernel its set is incomplete."""
    for key, want in EXPECTED.items():
        a_tiled, w_bits, have_ws = key
        for target in want:
            kept = [c for c in gc.CASES if (c.a_tiled, c.w_bits) != (a_tiled, w_bits) or kernel(c, have_ws) != target]
            assert set(reached(kept, a_tiled, w_bits, have_ws)) != want, (key, target)


def test_both_sides_of_every_switch_are_present():
    """Each boundary of the plan has a case on either side (rows, reduction depth, channel count, tile counts, spill remainder)."""
    shapes = {(c.M, c.N, c.K_pad) for c in gc.CASES if c.a_tiled and c.w_bits == 4}
    for a, b in [((16, 200, 1280), (17, 200, 1280)), ((32, 2048, 512), (33, 2048, 512)), ((64, 520, 8192), (65, 520, 8192)),
                 ((20, 2048, 384), (20, 2048, 512)), ((24, 2056, 4096), (24, 2056, 4224)), ((40, 520, 8064), (40, 520, 8192)),
                 ((20, 2047, 512), (20, 2048, 512)), ((33, 16256, 8192), (33, 16257, 8192)), ((17, 48896, 128), (17, 49152, 128)),
                 ((33, 81664, 1408), (33, 81920, 1408)), ((33, 81664, 1280), (33, 81664, 1408)), ((97, 8064, 8192), (97, 8192, 8192)),
                 ((256, 769, 8192), (257, 769, 8192))]:
        assert a in shapes and b in shapes
        pa = gc.plan(*a, 4, True)
        pb = gc.plan(*b, 4, True)
        assert pa != pb, (a, pa, b, pb)


def test_ragged_shapes_and_bounded_oracle_cost():
    Ns = {c.N for c in gc.CASES}
    assert any(n % 4 for n in Ns) and any(n % 8 == 0 and (n // 8) % 2 for n in Ns) and any(n % 16 and n % 4 == 0 for n in Ns)
    assert any(c.M % 16 and c.M > 64 for c in gc.CASES)     # ragged against every row tile (16 ... 256)
    names = [c.name for c in gc.CASES]
    assert len(names) == len(set(names))
    for c in gc.CASES:
        # the whole oracle product stays bounded; larger cases are held to checksums and sampled columns
        assert gc.large(c) or gc.macs(c) <= gc.ORACLE_MACS
        assert c.K_pad % 128 == 0
