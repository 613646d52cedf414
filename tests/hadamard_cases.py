"""Seeded cases of the exact online Hadamard (csrc/hadamard.hip) on both sides of every point where its launch switches paths,
shared by the CPU check of what the plan reaches (test_hadamard_sweep_plan_cpu.py) and the GPU sweep (test_gpu_hadamard_sweep.py).

A case is (name, M, n_in, n, K, dtype, fp32_had, quant, act, prepared, tiled, threads, aligned):
  dtype    "f16" / "bf16" / "f32"
  quant    0 = mq_hadamard; 1 = fused quantizer, one scale; 2 = row_sel + second scale; 3 = 2 with skip_col0 (+ x0_out)
  act      0, or ops.ACT_SILU_MUL / ops.ACT_QUICK_GELU (mq_act_hadamard_quant_i8; quant != 0)
  prepared sign words (0) or a prepared descriptor (1)
  threads  mq_hadamard_debug_threads for the call: 0 (by shape), 256, 512
  aligned  "a"    every operand 16-byte aligned
           "x1"   x is a column slice starting one element in (no vector loads)
           "ldx"  x's row stride is not a multiple of 16 bytes
           "x2ok" silu * up with an unaligned gate and an aligned up
           "q4"   out= a column slice of a wider int8 buffer: pointer 4- but not 16-byte aligned, row stride % 16 == 4
           "q2"   the same with a row stride % 4 == 2 (byte stores in the classic / K = 1 paths, 2-byte stores in the units)
The path a case takes is what ``mq_hadamard_debug_plan`` answers (``plan`` / ``key`` below); the launch is driven by the same
function.  The list is: hand-placed sections (shape classes, the short-batch and row-map ladders, n_in ladders, alignment,
fused activations) and a FILL that walks the accepted domain in a fixed order and adds the first point of every path key the
sections did not reach, so whatever the plan can return is run against the oracle.  Outside the switch it probes a case uses three
rows (one of them all zero): the oracle costs O(n (log m + K)) per row."""
import ctypes as C
import functools
import zlib
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name M n_in n K dtype fp32_had quant act prepared tiled threads aligned")

TABLE_K = (12, 20, 28, 36, 40, 52, 60, 108, 140, 156, 172)
DT_CODE = {"f16": 0, "bf16": 1, "f32": 2}           # include/mquant_hip.h MQ_F16 / MQ_BF16 / MQ_F32
MODE = {"f16": 1, "bf16": 2, "f32": 0}              # oracle rounding modes
HAD_FP32, HAD_PREPARED = 1, 2                       # MQ_HAD_*
ALIGN_BITS = {"a": 7, "x1": 6, "ldx": 6, "x2ok": 6, "q4": 7, "q2": 3}      # MQ_HAD_ALIGN_X | _Q2 | _Q4
PLAN_FIELDS = ("threads", "unit", "half_lds", "act", "parts_log2", "grid", "lds", "butterfly", "kxk", "remap", "fast_first",
               "x_vec", "q_vec")                    # MQ_HAD_PLAN_*
KEY_FIELDS = tuple(f for f in PLAN_FIELDS if f not in ("grid", "lds"))
BUTTERFLY = ("scalar", "lane", "reg", "lds")        # MQ_HAD_BF_*
KXK = ("k1_vec4", "k1_scalar", "classic", "unit5", "unit3", "chain")       # MQ_HAD_KXK_*

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        from mquant_amd import _lib
        _LIB = _lib.load()
    return _LIB


def cu_count():
    """CUs the launch plans with: the current device's (a multiple of 8), 256 without a device -- csrc/runtime.hip device_cu_count."""
    cus = C.c_int(0)
    if lib().mq_device_info(None, 0, C.byref(cus)) != 0 or cus.value < 8:
        return 256
    return cus.value // 8 * 8


def query(M, n_in, n, K, dtype, flags, quant, act, tiled, aligned, threads=0):
    """(return code, {field: value}) of mq_hadamard_debug_plan with the thread hook set for the call."""
    L = lib()
    out = (C.c_int * len(PLAN_FIELDS))()
    L.mq_hadamard_debug_threads(threads)
    try:
        rc = L.mq_hadamard_debug_plan(M, n_in, n, K, DT_CODE[dtype], flags, int(quant), act, int(tiled), aligned, out)
    finally:
        L.mq_hadamard_debug_threads(0)
    return rc, dict(zip(PLAN_FIELDS, out))


def flags(c):
    return (HAD_FP32 if c.fp32_had else 0) | (HAD_PREPARED if c.prepared else 0)


def plan(c):
    rc, p = query(c.M, c.n_in, c.n, c.K, c.dtype, flags(c), c.quant != 0, c.act, c.tiled, ALIGN_BITS[c.aligned], c.threads)
    assert rc == 0, (c, rc)
    return p


def key(c):
    p = plan(c)
    return tuple(p[f] for f in KEY_FIELDS)


def describe(p):
    return (f"{p['threads']} threads, unit {p['unit']}, {'16-bit' if p['half_lds'] else 'fp32'} staging, act {p['act']}, "
            f"parts_log2 {p['parts_log2']}, grid {p['grid']}, {p['lds']} B LDS, butterflies {BUTTERFLY[p['butterfly']]}, "
            f"K x K {KXK[p['kxk']]}, remap {p['remap']}, x_vec {p['x_vec']}, q_vec {p['q_vec']}")


def m_ladder(cus):
    """Rows on both sides of every parts_log2 step (M << (parts + 1) <= CUs) and of the 128-row remap."""
    out = {1, 127, 128, 129, 130, 256, 257}
    for j in range(1, 5):
        if cus >> j >= 1:
            out |= {cus >> j, (cus >> j) + 1}
    return sorted(out)


# (n_in, n, K) of every shape class: butterfly class x {K = 1, K > 1}, every K x K class
SCALAR = [(1, 1, 1), (2, 2, 1), (4, 4, 1), (20, 20, 20), (40, 40, 20), (70, 80, 20)]
CHAIN = [(96, 96, 12), (160, 160, 20), (448, 448, 28), (1280, 1280, 40), (1664, 1664, 52)]       # m = 8, 8, 16, 32, 32
LANE_K1 = [(8, 8, 1), (64, 64, 1), (500, 512, 1)]
CLASSIC = [(768, 768, 12), (1280, 1280, 20), (3584, 3584, 28), (3456, 3456, 108), (4480, 4480, 140), (7680, 7680, 60),
           (27648, 27648, 108)]
UNIT5 = [(18944, 19968, 156), (17920, 17920, 140)]            # contiguous / aliased last row group
UNIT3 = [(5120, 5120, 40), (11008, 11008, 172), (6656, 6656, 52)]   # four waves contiguous; eight waves, both aliased
REG_K1 = [(1024, 1024, 1), (2048, 2048, 1), (4096, 4096, 1), (8192, 8192, 1)]                     # R = 2, 4, 8, 16
REG_K = [(12288, 12288, 12), (20000, 20480, 20), (28672, 28672, 28), (36864, 36864, 36), (24576, 24576, 12)]   # R = 2 .. 2, 4
LDS_K1 = [(16384, 16384, 1), (32768, 32768, 1)]
SHAPES = SCALAR + CHAIN + LANE_K1 + CLASSIC + UNIT5 + UNIT3 + REG_K1 + REG_K + LDS_K1
UNITS = UNIT5 + UNIT3
TIE_SHAPES = [(4096, 4096, 1, 0), (3584, 3584, 28, 0), (18944, 19968, 156, 1), (5120, 5120, 40, 1), (1280, 1280, 40, 0)]

_DT_HOOK = [("f16", 0, 0), ("bf16", 0, 0), ("f32", 0, 0), ("f16", 1, 0), ("f16", 0, 256), ("f16", 0, 512), ("f32", 0, 256),
            ("f32", 0, 512)]
_MODES = [(0, False), (2, False), (3, True)]          # (quant, tiled)


def _name(tag, M, n_in, n, K, dtype, fp32_had, quant, act, prepared, tiled, threads, aligned):
    return (f"{tag}|{n_in}>{n}x{K}|M{M}|{dtype}{'+fp32' if fp32_had else ''}|q{quant}{'t' if tiled else 'r'}|act{act}|"
            f"{'desc' if prepared else 'words'}|t{threads}|{aligned}")


def _case(tag, M, shape, dtype="f16", fp32_had=0, quant=0, act=0, prepared=0, tiled=False, threads=0, aligned="a"):
    n_in, n, K = shape
    prepared = int(bool(prepared) and K > 1)
    args = (M, n_in, n, K, dtype, int(fp32_had), quant, act, prepared, bool(tiled), threads, aligned)
    return Case(_name(tag, *args), *args)


def domain_keys(cus=None):
    """{path key: first grid point} over the accepted domain, smallest shapes first (refused points left out)."""
    cus = cu_count() if cus is None else cus
    Ms = m_ladder(cus)
    L = lib()
    out = {}
    buf = (C.c_int * len(PLAN_FIELDS))()
    keep = [PLAN_FIELDS.index(f) for f in KEY_FIELDS]
    try:
        for threads in (0, 256, 512):
            L.mq_hadamard_debug_threads(threads)
            for K in (1,) + TABLE_K:
                for p in range(16):
                    n = K << p
                    for dtype, fp32_had in (("f16", 0), ("f32", 0), ("bf16", 0), ("f16", 1)):
                        for prepared in ((0, 1) if K > 1 else (0,)):
                            fl = (HAD_FP32 if fp32_had else 0) | (HAD_PREPARED if prepared else 0)
                            for quant, act, tiled in ((0, 0, False), (2, 0, False), (3, 0, True), (2, 1, False), (3, 1, True)):
                                for aligned in ("a", "x1", "q2"):
                                    if aligned == "q2" and (not quant or tiled):
                                        continue
                                    for M in Ms:
                                        if L.mq_hadamard_debug_plan(M, n, n, K, DT_CODE[dtype], fl, int(quant != 0), act, int(tiled),
                                                                    ALIGN_BITS[aligned], buf) == 0:
                                            k = tuple(buf[i] for i in keep)
                                            if k not in out:
                                                out[k] = (M, n, n, K, dtype, fp32_had, quant, act, prepared, tiled, threads, aligned)
    finally:
        L.mq_hadamard_debug_threads(0)
    return out


def sections(cus):
    """The hand-placed part of the list."""
    out = []
    # ---- every shape class: dtypes, forced threads, sign words / descriptor, plain / row-major / tiled
    for sh in SHAPES:
        for dtype, fp32_had, threads in _DT_HOOK:
            for prepared in ((0, 1) if sh[2] > 1 else (0,)):
                for quant, tiled in _MODES:
                    out.append(_case("class", 3, sh, dtype, fp32_had, quant, 0, prepared, tiled, threads))
    # ---- short batches and the row map: M on both sides of every parts_log2 step and of the 128-row remap
    ladder = m_ladder(cus)
    for sh in UNITS:
        for M in ladder:
            if M > 130 and sh not in ((18944, 19968, 156), (5120, 5120, 40)):
                continue
            for tiled in (False, True):
                out.append(_case("rows", M, sh, "f16", 0, 3, 0, 1, tiled))
    for sh, act in (((18944, 19968, 156), 1), ((5120, 5120, 40), 2), ((11008, 11008, 172), 2)):
        for M in (max(1, cus >> 3), (cus >> 3) + 1, (cus >> 2) + 1, 127):
            for dtype in ("bf16", "f32"):
                out.append(_case("rows", M, sh, dtype, 0, 2, 0, 1, M % 2 == 1))
            out.append(_case("rows", M, sh, "f16", 0, 3, act, 1, M % 2 == 0))
    for sh in ((3584, 3584, 28), (4096, 4096, 1), (1280, 1280, 40), (12288, 12288, 12)):     # the row map without units
        for M in (127, 128, 129, 130, 256, 257):
            out.append(_case("rows", M, sh, "f16", 0, 3, 0, 0, True))
    for sh, M in (((5120, 5120, 40), 2500), ((3584, 3584, 28), 2100), ((18944, 19968, 156), 1040)):   # past the resident workgroups
        for tiled in (False, True):
            out.append(_case("rowloop", M, sh, "f16", 0, 3, 0, 1, tiled))
    # ---- zero padding: kept k-steps n (all), one less, even, odd, one, n_in <= m, 1, n_in % 8 != 0
    for n_in0, n, K in UNITS + [(3584, 3584, 28)]:
        m = n // K
        for n_in in (n, n - 4 * m, 8 * m, 12 * m, 4 * m, 4 * m - 3, m, m - 3, 1, 8 * m + 5):
            for prepared in (0, 1):
                for quant, tiled in _MODES:
                    out.append(_case("pad", 3, (n_in, n, K), "f16", 0, quant, 0, prepared, tiled))
            out.append(_case("pad", 3, (n_in, n, K), "f32", 0, 2, 0, 1, False))
    # ---- unaligned operands and destinations
    al_shapes = [(18944, 19968, 156), (5120, 5120, 40), (11008, 11008, 172), (3584, 3584, 28), (4096, 4096, 1), (1280, 1280, 40),
                 (70, 80, 20), (12288, 12288, 12), (4, 4, 1)]
    for sh in al_shapes:
        for dtype in ("f16", "f32"):
            for aligned in ("x1", "ldx"):
                out.append(_case("align", 3, sh, dtype, 0, 0, 0, 1, False, 0, aligned))
                out.append(_case("align", 3, sh, dtype, 0, 2, 0, 1, False, 0, aligned))
            for aligned in ("q4", "q2"):
                out.append(_case("align", 3, sh, dtype, 0, 3, 0, 1, False, 0, aligned))
                out.append(_case("align", 3, sh, dtype, 0, 2, 0, 0, False, 0, aligned))
    # ---- the fused-activation instantiation on every unit class, the classic, chain, K = 1 and register paths
    for sh in UNITS + [(3584, 3584, 28), (27648, 27648, 108), (1280, 1280, 40), (96, 96, 12), (4096, 4096, 1), (500, 512, 1),
                       (12288, 12288, 12), (16384, 16384, 1)]:
        for act in (1, 2):
            for dtype, fp32_had, threads in (("f16", 0, 0), ("bf16", 0, 0), ("f32", 0, 0), ("f16", 0, 256), ("f16", 0, 512)):
                for prepared in ((0, 1) if sh[2] > 1 else (0,)):
                    out.append(_case("act", 3, sh, dtype, fp32_had, 3 if act == 1 else 2, act, prepared, act == 1, threads))
        out.append(_case("act", 3, sh, "f16", 0, 2, 1, 1, False, 0, "x2ok"))
        out.append(_case("act", 3, sh, "f32", 0, 3, 1, 1, True, 0, "x2ok"))
    return out


@functools.lru_cache(maxsize=4)
def build_cases(cus):
    out = sections(cus)
    have = {key(c) for c in out}
    for k, g in domain_keys(cus).items():
        if k not in have:
            have.add(k)
            args = g
            out.append(Case(_name("fill", *args), *args))
    names = [c.name for c in out]
    assert len(names) == len(set(names))
    return tuple(out)


def cases():
    return build_cases(cu_count())


# ------------------------------------------------------------------------------------------------ inputs and the oracle
def seed_of(*parts):
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


def round_dtype(x, dtype):
    import oracle
    return oracle.round_to(x, MODE[dtype])


@functools.lru_cache(maxsize=6)
def _rows(n_in, dtype, gen, which):
    from golden_inputs import make_x
    x = make_x(seed_of(n_in, dtype, which), (gen, n_in), outlier_frac=0.002, outlier_gain=12.0)
    return round_dtype(x, dtype)


def make_rows(c, which=0):
    """[M, n_in] fp32 values representable in the case's dtype; row 1 (when there is one) is all zero."""
    gen = 4 if c.M <= 4 else 257 if c.M <= 257 else c.M
    x = _rows(c.n_in, c.dtype, gen, which)[: c.M].copy()
    if c.M > 1 and which == 0:
        x[1] = 0.0
    return x


@functools.lru_cache(maxsize=4)
def _rotated(n_in, n, K, dtype, fp32_had, gen, zero_row, hk_bytes):
    import oracle
    x = _rows(n_in, dtype, gen, 0).copy()
    if zero_row:
        x[1] = 0.0
    hk = None if K == 1 else np.frombuffer(hk_bytes, dtype=np.int8).reshape(K, K)
    return rotate(x, n, K, hk, dtype, fp32_had)


def rotate(x, n, K, hk, dtype, fp32_had):
    """The oracle's rotated activations of fp32 rows ``x`` (fp32 values of the case's dtype)."""
    import oracle
    mode = MODE[dtype]
    return oracle.hadamard(x, n, K, None if K == 1 else hk, mid_round=0 if fp32_had else mode, out_round=mode)


def rotated(c, mats):
    """oracle.hadamard of make_rows(c) (cached per shape: the rows of a shorter batch are a prefix of a longer one's)."""
    gen = 4 if c.M <= 4 else 257 if c.M <= 257 else c.M
    hk = b"" if c.K == 1 else np.ascontiguousarray(mats[c.K], dtype=np.int8).tobytes()
    return _rotated(c.n_in, c.n, c.K, c.dtype, c.fp32_had, gen, True, hk)[: c.M]


def scales(rot):
    """Static scales: the first spans the row's range, the second saturates both clamps."""
    s0 = np.float32(max(float(np.abs(rot).max()), 1e-3) / 127.0)
    return s0, np.float32(s0 * np.float32(0.6))


def row_sel(M):
    return (np.arange(M) % 2).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ ties of the fused quantizer
TIE_SCALES_F32 = (0.0371, 0.0113, 0.0457)
TIE_SCALES_16 = (2.0 ** -5, 2.0 ** -3)


def _ulps(v, k):
    out = v.copy()
    for _ in range(abs(k)):
        out = np.nextafter(out, np.float32(np.inf if k > 0 else -np.inf)).astype(np.float32)
    return out


def tie_amplitudes_f32(n, s, step=1):
    """One-hot amplitudes a (fp32) whose rotated value y = fl(a * fl(1 / sqrt n)) -- the same in every column up to sign -- makes
    fl(y / s) an exact half-integer in 0.5 .. 128.5 (first list), or makes rint(fl(y * fl(1 / s))) differ from rint(fl(y / s))
    (second list).  Searched a few ulps around t * s and y / scale; targets with no such amplitude are left out."""
    f32 = np.float32
    s = f32(s)
    inv = f32(1.0) / s
    scale = f32(1.0) / np.sqrt(f32(n))
    t = (np.arange(0, 129, step, dtype=np.float32) + f32(0.5))
    ties, flips = [], []
    for d in range(-6, 7):
        y = _ulps((t * s).astype(f32), d)
        quo = (y / s).astype(f32)
        rcp = (y * inv).astype(f32)
        for i in np.nonzero(quo == t)[0]:
            ties.append((float(t[i]), y[i]))
        for i in np.nonzero(np.rint(quo) != np.rint(rcp))[0]:
            flips.append((float(t[i]), y[i]))

    def amplitudes(pairs):
        seen, out = set(), []
        for tt, y in pairs:
            if tt in seen:
                continue
            a0 = np.array([y / scale], dtype=f32)
            for d in range(-4, 5):
                a = _ulps(a0, d)
                if (a * scale).astype(f32)[0] == y:
                    seen.add(tt)
                    out.append(a[0])
                    break
        return out

    return amplitudes(ties), amplitudes(flips)


def tie_amplitudes_16(n, s, dtype):
    """The same for 16-bit inputs and a scale that puts 16-bit values on exact ties: every positive 16-bit amplitude a whose
    rotated value rnd(fl(a * fl(1 / sqrt n))) is (k + 0.5) * s, one per k."""
    f32 = np.float32
    bits = np.arange(1, 0x7C00 if dtype == "f16" else 0x7F80, dtype=np.uint16)
    a = bits.view(np.float16).astype(f32) if dtype == "f16" else (bits.astype(np.uint32) << 16).view(f32)
    scale = f32(1.0) / np.sqrt(f32(n))
    y = round_dtype((a * scale).astype(f32), dtype)
    q = (y / f32(s)).astype(f32)
    ok = (q <= 128.5) & (q == np.floor(q) + f32(0.5))
    _, first = np.unique(q[ok], return_index=True)
    return list(a[ok][first]), []


def tie_rows(n_in, n, K, dtype, s, step=1):
    """(x [rows, n_in], number of tie rows): one one-hot row per amplitude, the hot column moving through the row."""
    ties, flips = tie_amplitudes_f32(n, s, step) if dtype == "f32" else tie_amplitudes_16(n, s, dtype)
    amps = ties + flips
    x = np.zeros((len(amps), n_in), dtype=np.float32)
    for r, a in enumerate(amps):
        x[r, (r * 131 + 7) % n_in] = a if r % 2 == 0 else -a
    return x, len(ties)


def tie_shares(rot, s):
    """(share of exact ties, share of quotient / reciprocal disagreements) among the elements of ``rot``."""
    f32 = np.float32
    s = f32(s)
    quo = (rot / s).astype(f32)
    rcp = (rot * (f32(1.0) / s)).astype(f32)
    tie = np.abs(quo - np.trunc(quo)) == f32(0.5)
    return float(tie.mean()), float((np.rint(quo) != np.rint(rcp)).mean())
