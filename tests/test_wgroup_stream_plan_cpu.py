"""Which kernel a weight-group GEMM call takes (mq_gemm_debug_group_plan: the host function the dispatcher itself calls, so a test
that reads 61 knows the streaming kernel of gemm_skinny.hip ran).  Host arithmetic only: no device."""
import ctypes
import itertools

from mquant_amd import _lib

STREAM, ROUND1 = 61, 26
WS_IDS = (45, 46, 47, 48, 51, 53)                       # wave-specialised ids a test or an A/B run may force

# The Qwen2-VL-7B decoder Linears, (N, K), at g = 128: the shape classes profiles/decode_wgroup_gemm_bench.txt measured faster on the
# streaming kernel than on the tiled kernels of the same call at M = 1, 8 and 16, symmetric and asymmetric (every class it measured:
# none was excluded).
DECODER = {"q|k|v": (4608, 3584), "o_proj": (3584, 3584), "gate|up": (37888, 3584), "down_proj": (3584, 19968)}

# (M, N, K, g) of the GPU sweep (tests/test_gpu_wstream_wgroup.py); K_pad = K rounded up to 128
SWEEP = [(1, 200, 1280, 128), (3, 72, 192, 64), (16, 48, 3584, 256), (5, 264, 1920, 64), (9, 520, 19968, 128), (2, 96, 2048, 512),
         (1, 136, 1024, 1024)]


def force(tile):
    assert _lib.load().mq_gemm_debug_force(tile, 0) == 0


def plan(M, N, K, g, *, w_bits=4, a_tiled=1, x_groups=0, asym=0, aligned=1):
    tile = ctypes.c_int(-1)
    K_pad = (K + 127) // 128 * 128
    rc = _lib.load().mq_gemm_debug_group_plan(M, N, K_pad, w_bits, a_tiled, g, K // g, x_groups, asym, aligned, ctypes.cast(ctypes.byref(tile), ctypes.c_void_p))
    assert rc == 0, _lib.load().mq_last_error()
    return tile.value


def test_the_symbol_exists_and_answers_without_a_device():
    force(-1)
    assert plan(1, 4608, 3584, 128) == STREAM or 40 <= plan(1, 4608, 3584, 128) < 60
    from mquant_amd import ops
    assert ops.gemm_group_plan(1, 4608, 3584, 128) == plan(1, 4608, 3584, 128)
    assert ops.gemm_group_plan(300, 4608, 3584, 128, asym=True) == ROUND1


def test_generation_steps_of_the_decoder_take_the_streaming_kernel():
    force(-1)
    bad = [(name, M, asym, xg) for (name, (N, K)), M, asym, xg in itertools.product(DECODER.items(), (1, 8, 16), (0, 1), (0, 1))
           if plan(M, N, K, 128, asym=asym, x_groups=xg) != STREAM]
    assert not bad, bad


def test_classes_that_were_not_measured_keep_the_tiled_kernels():
    """The plan selects the streaming kernel only where profiles/decode_wgroup_gemm_bench.txt shows it faster: 2 ... 312 groups of 64, 128
    or 256.  A single group and groups above 256 were not run."""
    force(-1)
    for asym in (0, 1):
        assert plan(1, 4608, 256, 128, asym=asym) == STREAM and plan(16, 3584, 19968, 64, asym=asym) == STREAM
        assert plan(1, 4608, 3584, 256, asym=asym) == STREAM
        assert plan(1, 4608, 128, 128, asym=asym) != STREAM and plan(1, 136, 1024, 1024, asym=asym) != STREAM
        assert plan(2, 96, 2048, 512, asym=asym) != STREAM


def test_prefill_shapes_keep_the_tiled_kernels():
    force(-1)
    for (N, K), M in itertools.product(DECODER.values(), (17, 33, 300, 2048)):
        assert 40 <= plan(M, N, K, 128) < 60, (M, N, K, plan(M, N, K, 128))          # a wave-specialised tile (gemm_common.h)
        assert plan(M, N, K, 128, asym=1) == ROUND1, (M, N, K)


def test_what_the_streaming_kernel_cannot_do_never_reaches_it():
    """int8 weights, row-major activations, a second row tile (M = 17: the kernel is built for one), N % 4 != 0, unaligned tables --
    under the plain plan and with 61 forced (a forced tile outside a mode's set is ignored)."""
    try:
        for f in (-1, STREAM):
            force(f)
            for (N, K), asym in itertools.product(DECODER.values(), (0, 1)):
                for kw in (dict(w_bits=8), dict(a_tiled=0), dict(aligned=0)):
                    assert plan(8, N, K, 128, asym=asym, **kw) != STREAM, (f, N, K, asym, kw)
                assert plan(17, N, K, 128, asym=asym) != STREAM, (f, N, K, asym)
                assert plan(8, N + 2, K, 128, asym=asym) != STREAM, (f, N, K, asym)
                assert plan(8, N + 1, K, 128, asym=asym) != STREAM, (f, N, K, asym)
    finally:
        force(-1)


def test_a_forced_61_selects_it_for_every_shape_of_the_gpu_sweep():
    try:
        force(STREAM)
        bad = [(s, asym, xg) for s, asym, xg in itertools.product(SWEEP, (0, 1), (0, 1)) if plan(*s, asym=asym, x_groups=xg) != STREAM]
        assert not bad, bad
    finally:
        force(-1)


def test_a_forced_tiled_id_keeps_the_tiled_kernels():
    """A wave-specialised id or 26 is how the existing tests and the A/B runs address the kernels from before the streaming one:
    symmetric groups answer the forced id, asymmetric groups 26 (the round-1 kernel is the only tiled kernel of that mode)."""
    try:
        for f in WS_IDS + (ROUND1,):
            force(f)
            for (M, N, K, g) in SWEEP + [(1, 4608, 3584, 128), (8, 3584, 19968, 128)]:
                assert plan(M, N, K, g) == f, (f, M, N, K, g, plan(M, N, K, g))
                assert plan(M, N, K, g, asym=1) == ROUND1, (f, M, N, K, g)
    finally:
        force(-1)
