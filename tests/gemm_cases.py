"""Seeded W4A8 GEMM cases on both sides of every point where the default plan (csrc/gemm_w4a8.hip make_plan) switches kernels,
shared by the CPU check of what the plan reaches (test_gemm_sweep_plan_cpu.py) and the GPU sweep of the entry points
(test_gpu_gemm_sweep.py).

A case is (name, M, N, K_pad, w_bits, a_tiled): K_pad is the whole reduction (no zero tail), a_tiled selects the tiled activation
layout (MQ_LD_TILED) over row-major rows.  Outside the weight-streaming, spill and split-K rules the plan does not depend on K, so
those cases use the smallest K_pad; the few shapes that must be large to reach a branch are LARGE: the GPU sweep holds them to exact
integer identities (row and column checksums) and to the oracle on sampled columns instead of the whole product."""
import ctypes as C
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name M N K_pad w_bits a_tiled")

#: multiply-accumulates above which a case is checked on sampled columns (the C oracle runs ~1e10 MAC/s on 16 cores)
ORACLE_MACS = 1_000_000_000


def macs(c: Case) -> int:
    return c.M * c.N * c.K_pad


def large(c: Case) -> bool:
    return macs(c) > ORACLE_MACS


def _both(name, M, N, K_pad, layouts=((4, True),)):
    return [Case(f"{name}|w{b}{'t' if t else 'r'}", M, N, K_pad, b, t) for b, t in layouts]


TW4, TW8, RW4, RW8 = (4, True), (8, True), (4, False), (8, False)
ALL = (TW4, TW8, RW4, RW8)

CASES = (
    # ---- rows: 16 / 17, 32 / 33, 64 / 65 (tiled W4: the weight-streaming kernels 60 / 61 against the wave-specialised tiles)
    _both("M16 few pairs", 16, 200, 1280, ALL)                   # 60, K slices across workgroups (row-major: tile 10)
    + _both("M17 few pairs", 17, 200, 1280, ALL)                 # 53
    + _both("M32 wide", 32, 2048, 512, (TW4, TW8))               # 61, the eight waves of one workgroup are the slices
    + _both("M33 wide", 33, 2048, 512)                           # 53
    + _both("M64 long", 64, 520, 8192, (TW4, TW8))               # 60, many slices / W8: ws split-K
    + _both("M65 long", 65, 520, 8192, (TW4, RW4))               # ws split-K / row-major: tile 10
    + _both("M1", 1, 1000, 384, (TW4, RW8))                      # 60 one slice (K too short to slice)
    # ---- K_pad 512 / 4096 / 8192
    + _both("K384 wide", 20, 2048, 384)                          # 53 (too short for 61)
    + _both("K512 wide", 20, 2048, 512)                          # 61
    + _both("K4096 wide", 24, 2056, 4096)                        # 61, one launch
    + _both("K4224 wide", 24, 2056, 4224)                        # 53 (past the short-reduction rule, not yet long)
    + _both("K4096 M16", 16, 200, 4096)                          # 60, 16 slices
    + _both("K4224 M16", 16, 200, 4224)                          # 61, two workgroup slices
    + _both("K8064 M40", 40, 520, 8064)                          # 53 (kps = 63)
    + _both("K8192 M40", 40, 520, 8192)                          # 60
    + _both("K8192 M32", 32, 200, 8192)                          # 61, four workgroup slices
    # ---- N >= 2048 for 17..32 rows; ceil(N / 128) < 128 for 33..64 rows on long reductions
    + _both("N2047", 20, 2047, 512)                              # 53, N % 4 == 3
    + _both("N2048", 20, 2048, 512)                              # 61
    + _both("N16256 long", 33, 16256, 8192)                      # 60 (127 channel tiles)
    + _both("N16257 long", 33, 16257, 8192)                      # ws walks the whole reduction (128 channel tiles)
    # ---- the tile cost model (K does not matter: smallest K_pad)
    + _both("tiles 96x128", 1090, 2048, 128, ALL)                # 54 / 31
    + _both("tiles 128x128", 1000, 3832, 128, ALL)               # 51 / 26, N = 8 x odd
    + _both("tiles 192x128", 1000, 5112, 128, (TW4, RW4))        # 52 / 35
    + _both("tiles 256x128", 481, 11008, 128, (RW4, RW8))        # 2
    # ---- t256 >= 192: the wide tile (tiled W4: 20, else 3) and the spill rule (rem < 64, long enough reduction; 33 rows: past
    #      the weight-streaming rule of 17..32 rows)
    + _both("t256 191", 17, 48896, 128, ALL)                     # 53 / 10
    + _both("t256 192", 17, 49152, 128, ALL)                     # 20 / 3
    + _both("spill rem63 kps11", 33, 81664, 1408)                # 52
    + _both("spill rem63 kps10", 33, 81664, 1280)                # 20
    + _both("spill rem64 kps11", 33, 81920, 1408)                # 20
    # ---- ceil(M/96) ceil(N/128) >= 128 and split-K (the plan's workspace rules)
    + _both("96-tiles 126", 97, 8064, 8192)                      # ws split-K over the 64 x 128 tile
    + _both("96-tiles 128", 97, 8192, 8192)                      # no split: enough tiles
    + _both("split M256", 256, 769, 8192, (TW4, TW8))            # ws split-K
    + _both("split M257", 257, 769, 8192, (TW4, TW8, RW8))       # tile 3 split-K (row-major: the only split-K rule)
    + _both("split 1 row", 1, 2048, 8192, (TW8, RW4))            # ws split-K (W8) / tile 3 split-K with one row
)

_LIB = None


def plan(M, N, K_pad, w_bits, a_tiled, have_ws=True):
    """(tile id, split-K factor) of the default plan (``mq_gemm_debug_plan``: host arithmetic, no device; an unbounded workspace)."""
    global _LIB
    if _LIB is None:
        from mquant_amd import _lib
        _LIB = _lib.load()
    tile, splits = C.c_int(-1), C.c_int(-1)
    rc = _LIB.mq_gemm_debug_plan(M, N, K_pad, w_bits, int(a_tiled), int(have_ws), C.byref(tile), C.byref(splits))
    assert rc == 0
    return tile.value, splits.value


def operands(c: Case):
    """Seeded int8 activations [M, K_pad], weight levels [N, K_pad] and the per-channel / per-row epilogue operands (numpy).
    Both operands carry their extreme levels; the parameters are exact fp32."""
    rng = np.random.default_rng([c.M, c.N, c.K_pad, c.w_bits, int(c.a_tiled)])
    lim = 8 if c.w_bits == 4 else 128
    a = rng.integers(-128, 128, size=(c.M, c.K_pad), dtype=np.int8)
    a[0, :4] = [-128, 127, -128, -128]
    w = rng.integers(-lim, lim, size=(c.N, c.K_pad), dtype=np.int8)
    w[0, :4] = [-lim, lim - 1, -lim, -lim]
    f32 = np.float32
    return dict(
        rng=rng, a=a, w=w,
        s_w=rng.uniform(0.001, 0.01, size=c.N).astype(f32), bias=rng.normal(size=c.N).astype(f32),
        w0=rng.normal(size=c.N).astype(f32), w1=rng.normal(size=c.N).astype(f32),
        x0=rng.normal(size=c.M).astype(f32), x1=rng.normal(size=c.M).astype(f32),
        rows=rng.uniform(0.01, 0.05, size=c.M).astype(f32), sel=(rng.random(c.M) < 0.5).astype(np.uint8),
        res=(rng.normal(size=(c.M, c.N)) * 3).astype(f32),
    )


def columns(c: Case, rng):
    """Columns the oracle is held to: all of them, or for a LARGE case both edges and a seeded sample of the rest."""
    if not large(c):
        return np.arange(c.N)
    pick = rng.choice(c.N, size=min(c.N, 192), replace=False)
    return np.unique(np.concatenate([np.arange(64), np.arange(c.N - 64, c.N), pick]))
