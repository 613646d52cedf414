"""What the activation-quantizer entry points refuse, and in which words (csrc/act_quant.hip, act_quant_dyn.hip, rmsn_quant.hip,
rowsum.hip, minmax.hip).  The host checks run before anything touches a device, so every call here is made with dummy addresses on
any machine: a table of violating calls, each with the status and the mq_last_error() text it must produce.  Only refused calls (and
M == 0 / K == 0 / N == 0, which return before the buffers are looked at) belong here: nothing in the table may reach a launch.  That
is why the "unknown dtype" exits of mq_minmax_channels and mq_minmax_tensor have no row: both launch their initialisation kernel
before they look at the dtype.

The expected values were recorded from the library as it was before the quantizers shared one destination check and one dtype
dispatcher.  One row is not a recording (NEW_IN_SHARED_CHECK below): mq_rmsn_quantize_i8 used to accept a destination that is not
16-byte aligned although its kernel stores 16 bytes at a time like its siblings; it now refuses it in the words of its own
destination check."""

import pytest

from mquant_amd import _lib

OK, EINVAL = 0, -1
F16, BF16, F32 = _lib.MQ_F16, _lib.MQ_BF16, _lib.MQ_F32
TILED = 0                      # MQ_LD_TILED
P = 0x7F0000001000             # a 16-byte aligned address nobody dereferences: every call is refused first

# the parameter names of include/mquant_hip.h, in order
PARAMS = {
    "mq_quantize_act_i8": "x x_dtype M K ldx scale0 scale1 scale_vec0 scale_vec1 row_sel skip_col0 x0_out out K_pad ldo stream",
    "mq_fakequant_act": "x x_dtype M K ldx scale0 scale1 scale_vec0 scale_vec1 row_sel skip_col0 out ldo stream",
    "mq_quantize_act_dyn_i8": "x x_dtype M K ldx bits clip_ratio skip_col0 x0_out scale_out out K_pad ldo stream",
    "mq_quantize_act_dyn_asym_i8": "x x_dtype M K ldx bits clip_ratio scale_out zero_out shift_out out K_pad ldo stream",
    "mq_quantize_act_range_i8": "x x_dtype M K ldx bits clip_ratio asym skip_col0 minmax x0_out scale_out zero_out shift_out out K_pad "
                                "ldo stream",
    "mq_quantize_act_group_i8": "x x_dtype M K ldx groupsize bits clip_ratio scale_out out K_pad ldo stream",
    "mq_quantize_act_group_asym_i8": "x x_dtype M K ldx groupsize bits clip_ratio scale_out zero_out shift_out out K_pad ldo stream",
    "mq_rmsn_quantize_i8": "x x_dtype M K ldx mean_dim eps scale0 scale1 row_sel y_out ldy out K_pad ldo stream",
    "mq_act_rowsum_scaled": "a lda M K_pad s_x0 s_x1 row_sel s_x_rows out stream",
    "mq_rank1_add_cast": "y32 M N ldy x_rows w out out_dtype ldo stream",
    "mq_minmax_channels": "x x_dtype M C ldx col_begin mn mx stream",
    "mq_minmax_tensor": "x x_dtype M C ldx col_begin out2 stream",
}

# a well-formed call of every entry point (32 x 256 fp16 rows into a row-major [32, 256] image); a table row overrides what it violates
BASE = dict(
    x=P, x_dtype=F16, M=32, K=256, ldx=256, scale0=0.5, scale1=0.25, scale_vec0=None, scale_vec1=None, row_sel=None, skip_col0=0,
    x0_out=None, out=P, K_pad=256, ldo=256, stream=None, bits=8, clip_ratio=1.0, scale_out=P, zero_out=P, shift_out=P, asym=0,
    minmax=P, groupsize=128, mean_dim=256.0, eps=1e-6, y_out=None, ldy=0, a=P, lda=256, s_x0=0.5, s_x1=0.5, s_x_rows=None,
    y32=P, N=256, x_rows=P, w=P, out_dtype=F16, C=256, col_begin=0, mn=P, mx=P, out2=P,
)
PER_FN = {"mq_rank1_add_cast": dict(ldy=256)}
NOTHING = dict(x=None, out=None, scale_out=None, zero_out=None, shift_out=None, minmax=None, a=None, y32=None, x_rows=None, w=None)

STATIC, FAKE = "mq_quantize_act_i8", "mq_fakequant_act"
DYN, DYNA, RANGE = "mq_quantize_act_dyn_i8", "mq_quantize_act_dyn_asym_i8", "mq_quantize_act_range_i8"
GRP, GRPA, RMSN = "mq_quantize_act_group_i8", "mq_quantize_act_group_asym_i8", "mq_rmsn_quantize_i8"
ROWSUM, RANK1, MMC, MMT = "mq_act_rowsum_scaled", "mq_rank1_add_cast", "mq_minmax_channels", "mq_minmax_tensor"
ROW_OWNERS = [DYN, DYNA, RANGE]                    # one workgroup per row, rows up to 32768 channels
TO_IMAGE = [DYN, DYNA, RANGE, GRP, GRPA, RMSN]     # the six that share one destination check and one message per entry point

# what a destination can violate: (what, overrides)
BAD_DEST = [("K_pad < K", dict(K_pad=128)), ("K_pad % 16", dict(K_pad=264, ldo=272)), ("misaligned out", dict(out=P + 8)),
            ("ldo < K_pad", dict(ldo=240)), ("ldo % 16", dict(ldo=264)), ("tiled, K_pad % 64", dict(K_pad=272, ldo=TILED))]

# (entry point, what the call violates, overrides of the well-formed call)
CALLS = (
    # ---- the static quantizer and its quantize -> dequantize form
    [(f, "negative M", dict(M=-1)) for f in (STATIC, FAKE)]
    + [(f, "negative K", dict(K=-16)) for f in (STATIC, FAKE)]
    + [(f, "no rows, nothing else", dict(M=0, **NOTHING)) for f in (STATIC, FAKE)]
    + [(f, "no channels, nothing else", dict(K=0, **NOTHING)) for f in (STATIC, FAKE)]
    + [(f, "null x", dict(x=None)) for f in (STATIC, FAKE)]
    + [(f, "null out", dict(out=None)) for f in (STATIC, FAKE)]
    + [(STATIC, "K_pad < K", dict(K_pad=128)),
       (STATIC, "K_pad % 16", dict(K_pad=264, ldo=272)),
       (STATIC, "misaligned out", dict(out=P + 8)),
       (STATIC, "ldo < K_pad", dict(ldo=240)),
       (STATIC, "ldo % 16", dict(ldo=264)),
       (STATIC, "tiled, K_pad % 64", dict(K_pad=272, ldo=TILED)),
       (STATIC, "ldx < K", dict(ldx=255)),
       (STATIC, "token types, per-channel scales, one vector", dict(row_sel=P, scale_vec0=P)),
       (STATIC, "unknown dtype", dict(x_dtype=3)),
       (FAKE, "ldx < K", dict(ldx=255)),
       (FAKE, "ldo < K", dict(ldo=255)),
       (FAKE, "unknown dtype", dict(x_dtype=-1))]
    # ---- the six that write the int8 image through one check
    + [(f, "no rows, nothing else", dict(M=0, **NOTHING)) for f in TO_IMAGE]
    + [(f, "null x", dict(x=None)) for f in TO_IMAGE]
    + [(f, "null out", dict(out=None)) for f in TO_IMAGE]
    + [(f, "null scale_out", dict(scale_out=None)) for f in (DYN, DYNA, RANGE, GRP, GRPA)]
    + [(f, "negative M", dict(M=-1)) for f in TO_IMAGE]
    + [(f, "no channels", dict(K=0)) for f in TO_IMAGE]
    + [(f, "ldx < K", dict(ldx=255)) for f in TO_IMAGE]
    + [(DYNA, "null shift_out", dict(shift_out=None)),
       (GRPA, "null shift_out", dict(shift_out=None)),
       (RANGE, "null minmax", dict(minmax=None)),
       (RANGE, "asymmetric, null shift_out", dict(asym=1, shift_out=None)),
       (RANGE, "asymmetric with the split column", dict(asym=1, skip_col0=1))]
    + [(f, "bits 1", dict(bits=1)) for f in (DYN, DYNA, RANGE, GRP, GRPA)]
    + [(f, "bits 9", dict(bits=9)) for f in (DYN, DYNA, RANGE, GRP, GRPA)]
    + [(f, "K too large", dict(K=32784, ldx=32784, K_pad=32896, ldo=32896)) for f in ROW_OWNERS]
    + [(RMSN, "K too large", dict(K=16400, ldx=16400, K_pad=16512, ldo=16512)),
       (RMSN, "K % 16", dict(K=250))]
    + [(f, "group size 8", dict(groupsize=8)) for f in (GRP, GRPA)]
    + [(f, "group size 2048", dict(groupsize=2048, K=2048, ldx=2048, K_pad=2048, ldo=2048)) for f in (GRP, GRPA)]
    + [(f, "group size 48", dict(groupsize=48, K=96, K_pad=96, ldo=96)) for f in (GRP, GRPA)]
    + [(f, "K % group size", dict(groupsize=128, K=192)) for f in (GRP, GRPA)]
    + [(f, "K_pad does not hold whole groups", dict(K_pad=272, ldo=272)) for f in (GRP, GRPA)]
    + [(f, what, ov) for f in TO_IMAGE for what, ov in BAD_DEST if not (f == RMSN and what == "misaligned out")]
    + [(RMSN, "misaligned out", dict(out=P + 8)),                       # NEW_IN_SHARED_CHECK
       (RMSN, "ldy < K", dict(y_out=P, ldy=255)),
       (RMSN, "scale 0", dict(scale0=0.0)),
       (RMSN, "mean_dim 0", dict(mean_dim=0.0)),
       (RMSN, "misaligned x", dict(x=P + 8)),
       (RMSN, "row stride % 16 bytes", dict(ldx=260)),
       (RMSN, "fp32 row stride % 16 bytes", dict(x_dtype=F32, ldx=258))]
    + [(f, "unknown dtype", dict(x_dtype=3)) for f in TO_IMAGE]
    + [(RANGE, "asymmetric, unknown dtype", dict(asym=1, x_dtype=7)),
       (GRPA, "unknown dtype -1", dict(x_dtype=-1))]
    # ---- the row sums and the third rank-1 term
    + [(ROWSUM, "no rows, nothing else", dict(M=0, **NOTHING)),
       (ROWSUM, "null a", dict(a=None)),
       (ROWSUM, "null out", dict(out=None)),
       (ROWSUM, "negative M", dict(M=-4)),
       (ROWSUM, "K_pad 0", dict(K_pad=0)),
       (ROWSUM, "K_pad % 16", dict(K_pad=264, lda=272)),
       (ROWSUM, "misaligned a", dict(a=P + 4)),
       (ROWSUM, "lda < K_pad", dict(lda=240)),
       (ROWSUM, "lda % 16", dict(lda=264)),
       (ROWSUM, "tiled, K_pad % 64", dict(K_pad=272, lda=TILED)),
       (RANK1, "no rows, nothing else", dict(M=0, **NOTHING)),
       (RANK1, "no channels, nothing else", dict(N=0, **NOTHING)),
       (RANK1, "null y32", dict(y32=None)),
       (RANK1, "null x", dict(x_rows=None)),
       (RANK1, "null w", dict(w=None)),
       (RANK1, "null out", dict(out=None)),
       (RANK1, "negative M", dict(M=-1)),
       (RANK1, "negative N", dict(N=-1)),
       (RANK1, "ldy < N", dict(ldy=255)),
       (RANK1, "ldo < N", dict(ldo=255)),
       (RANK1, "unknown dtype", dict(out_dtype=3))]
    # ---- the observers' reductions
    + [(f, "no rows", dict(M=0)) for f in (MMC, MMT)]
    + [(f, "no channels", dict(C=0)) for f in (MMC, MMT)]
    + [(f, "negative col_begin", dict(col_begin=-1)) for f in (MMC, MMT)]
    + [(f, "col_begin past the row", dict(col_begin=256)) for f in (MMC, MMT)]
    + [(f, "ldx < C", dict(ldx=255)) for f in (MMC, MMT)]
    + [(f, "null x", dict(x=None)) for f in (MMC, MMT)]
    + [(MMC, "null mn", dict(mn=None)),
       (MMC, "null mx", dict(mx=None)),
       (MMT, "null out2", dict(out2=None))]
)

NEW_IN_SHARED_CHECK = (RMSN, "misaligned out")

STATIC_OUT = ("mq_quantize_act_i8: out must be 16-byte aligned with ldo % 16 == 0, or ldo = MQ_LD_TILED with K_pad % 64 == 0 "
              "(ldo={})")
GROUP_SIZE = "mq_quantize_act_group_i8: groupsize={} must be a power of two in 16..1024 that divides K={}"
DEST = {DYN: DYN + ": bad K_pad / ldo / alignment", DYNA: DYNA + ": bad K_pad / ldo / alignment",
        RANGE: RANGE + ": bad K_pad / ldo / alignment",
        GRP: GRP + ": bad K_pad / ldo / alignment (K_pad must hold whole groups)",
        GRPA: GRP + ": bad K_pad / ldo / alignment (K_pad must hold whole groups)",
        RMSN: RMSN + ": bad K_pad / ldo"}


def named(f):
    """The name an entry point's refusals begin with: the asymmetric group-wise quantizer speaks as the symmetric one."""
    return GRP if f == GRPA else f


# (status, mq_last_error()) of every row of CALLS, in order; None: the call succeeds and leaves the message alone
EXPECTED = (
    [(EINVAL, f"{f}: negative shape") for f in (STATIC, FAKE)] * 2
    + [(OK, None)] * 4
    + [(EINVAL, f"{f}: null buffer") for f in (STATIC, FAKE)] * 2
    + [(EINVAL, "mq_quantize_act_i8: K_pad=128 must be >= K=256 and a multiple of 16"),
       (EINVAL, "mq_quantize_act_i8: K_pad=264 must be >= K=256 and a multiple of 16"),
       (EINVAL, STATIC_OUT.format(256)),
       (EINVAL, STATIC_OUT.format(240)),
       (EINVAL, STATIC_OUT.format(264)),
       (EINVAL, STATIC_OUT.format(0)),
       (EINVAL, "mq_quantize_act_i8: ldx < K"),
       (EINVAL, "mq_quantize_act_i8: row_sel with per-channel scales needs scale_vec1"),
       (EINVAL, "mq_quantize_act_i8: unknown dtype 3"),
       (EINVAL, "mq_fakequant_act: leading dimension < K"),
       (EINVAL, "mq_fakequant_act: leading dimension < K"),
       (EINVAL, "mq_fakequant_act: unknown dtype -1")]
    + [(OK, None)] * len(TO_IMAGE)
    + [(EINVAL, f"{named(f)}: bad shape") for f in TO_IMAGE] * 2
    + [(EINVAL, f"{named(f)}: bad shape") for f in (DYN, DYNA, RANGE, GRP, GRPA)]
    + [(EINVAL, f"{named(f)}: bad shape") for f in TO_IMAGE] * 3
    + [(EINVAL, "mq_quantize_act_dyn_asym_i8: bad shape"),
       (EINVAL, "mq_quantize_act_group_i8: bad shape"),
       (EINVAL, "mq_quantize_act_range_i8: bad shape"),
       (EINVAL, "mq_quantize_act_range_i8: the asymmetric mode needs shift_out and no split column"),
       (EINVAL, "mq_quantize_act_range_i8: the asymmetric mode needs shift_out and no split column")]
    + [(EINVAL, f"{named(f)}: bits must be 2..8") for f in (DYN, DYNA, RANGE, GRP, GRPA)] * 2
    + [(EINVAL, f"{f}: K=32784 too large (max 32768)") for f in ROW_OWNERS]
    + [(EINVAL, "mq_rmsn_quantize_i8: K must be a multiple of 16 and <= 16384 (got 16400)"),
       (EINVAL, "mq_rmsn_quantize_i8: K must be a multiple of 16 and <= 16384 (got 250)")]
    + [(EINVAL, GROUP_SIZE.format(8, 256))] * 2
    + [(EINVAL, GROUP_SIZE.format(2048, 2048))] * 2
    + [(EINVAL, GROUP_SIZE.format(48, 96))] * 2
    + [(EINVAL, GROUP_SIZE.format(128, 192))] * 2
    + [(EINVAL, DEST[GRP])] * 2
    + [(EINVAL, DEST[f]) for f in TO_IMAGE for what, _ in BAD_DEST if not (f == RMSN and what == "misaligned out")]
    + [(EINVAL, DEST[RMSN]),                                            # NEW_IN_SHARED_CHECK: not a recording
       (EINVAL, "mq_rmsn_quantize_i8: ldy < K"),
       (EINVAL, "mq_rmsn_quantize_i8: scale and mean_dim must be positive"),
       (EINVAL, "mq_rmsn_quantize_i8: scale and mean_dim must be positive"),
       (EINVAL, "mq_rmsn_quantize_i8: x rows must be 16-byte aligned"),
       (EINVAL, "mq_rmsn_quantize_i8: x rows must be 16-byte aligned"),
       (EINVAL, "mq_rmsn_quantize_i8: x rows must be 16-byte aligned")]
    + [(EINVAL, f"{named(f)}: unknown dtype 3") for f in TO_IMAGE]
    + [(EINVAL, "mq_quantize_act_range_i8: unknown dtype 7"),
       (EINVAL, "mq_quantize_act_group_i8: unknown dtype -1")]
    + [(OK, None)]
    + [(EINVAL, "mq_act_rowsum_scaled: bad shape")] * 5
    + [(EINVAL, "mq_act_rowsum_scaled: bad lda / alignment")] * 4
    + [(OK, None)] * 2
    + [(EINVAL, "mq_rank1_add_cast: bad arguments")] * 8
    + [(EINVAL, "mq_rank1_add_cast: unknown dtype 3")]
    + [(EINVAL, f"{f}: bad shape") for f in (MMC, MMT)] * 5
    + [(EINVAL, f"{f}: null buffer") for f in (MMC, MMT)]
    + [(EINVAL, "mq_minmax_channels: null buffer"),
       (EINVAL, "mq_minmax_channels: null buffer"),
       (EINVAL, "mq_minmax_tensor: null buffer")]
)


def refusal(fn, overrides):
    """(status, message) of one call; the message is None when the call left the thread's last error alone."""
    lib = _lib.load()
    values = {**BASE, **PER_FN.get(fn, {}), **overrides}
    args = [values[name] for name in PARAMS[fn].split()]
    lib.mq_gemm_debug_plan(0, 0, 0, 4, 0, 0, None, None)              # a refused call of its own: sets a known last error
    known = lib.mq_last_error()
    rc = getattr(lib, fn)(*args)
    msg = lib.mq_last_error()
    return rc, (None if msg == known else msg.decode())


IDS = [f"{f[len('mq_'):]}-{what}".replace(" ", "_").replace(",", "") for f, what, _ in CALLS]


def test_the_table_and_its_expectations_line_up():
    assert len(CALLS) == len(EXPECTED) and len(set(IDS)) == len(IDS)
    assert set(PARAMS) == {f for f, *_ in CALLS}, "every entry point has rows"
    for fn, names in PARAMS.items():
        assert len(names.split()) == len(_lib.SIGNATURES[fn][1]), fn
    for (fn, what, _), (rc, msg) in zip(CALLS, EXPECTED):
        # nothing in the table may get as far as a launch: it is refused, or it has no rows / channels
        assert rc != OK or what.startswith(("no rows", "no channels")), (fn, what)
        # a refusal begins with the entry point's name; the two group-wise entry points share the symmetric one's
        assert rc == OK or msg.startswith((fn + ": ", GRP + ": ")), (fn, what)
    assert [(f, what) for f, what, _ in CALLS].count(NEW_IN_SHARED_CHECK) == 1


@pytest.mark.parametrize("i", range(len(CALLS)), ids=IDS)
def test_refusal(i):
    fn, what, overrides = CALLS[i]
    assert refusal(fn, overrides) == EXPECTED[i], (fn, what)
