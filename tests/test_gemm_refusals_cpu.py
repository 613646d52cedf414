"""What the W4A8 GEMM entry points refuse, and in which words (csrc/gemm_w4a8.hip: the entry points' own checks, gemm_common, and the
dispatchers' checks that come before a launch).  The host checks run before anything touches a device, so every call here is made
with dummy addresses on any machine: a table of violating calls, each with the status and the mq_last_error() text it must produce.
Only refused calls (and M == 0 / N == 0, which return before the buffers are looked at) belong here: nothing in the table may reach
a launch.  The expected values were recorded from the library as it was before the dispatcher took a named argument struct."""

import pytest

from mquant_amd import _lib

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
F16, BF16, F32 = _lib.MQ_F16, _lib.MQ_BF16, _lib.MQ_F32
TILED = 0                      # MQ_LD_TILED
SILU_MUL, QUICK_GELU = 1, 2
P = 0x7F0000001000             # a 16-byte aligned address nobody dereferences: every call is refused first

# the parameter names of include/mquant_hip.h, in order
PARAMS = {
    "mq_gemm_w4a8": "a lda w w_bits M N K_pad s_x0 s_x1 row_sel s_w bias x0 w0 out out_dtype ldo stream",
    "mq_gemm_w4a8_ws": "a lda w w_bits M N K_pad s_x0 s_x1 row_sel s_w bias x0 w0 out out_dtype ldo workspace workspace_bytes stream",
    "mq_gemm_w4a8_residual_ws": "a lda w w_bits M N K_pad s_x0 s_x1 row_sel s_w bias x0 w0 residual ldr out out_dtype ldo workspace "
                                "workspace_bytes stream",
    "mq_gemm_w4a8_rope_ws": "a lda w w_bits M N K_pad s_x0 s_x1 row_sel s_w bias rope_cos rope_sin rope_cols head_dim out out_dtype ldo stream",
    "mq_gemm_w4a8_act_ws": "a lda w w_bits M N K_pad s_x0 s_x1 row_sel s_x_rows s_w bias act out out_dtype ldo stream",
    "mq_gemm_w4a8_rowscale_ws": "a lda w w_bits M N K_pad s_x_rows s_w bias x0 w0 out out_dtype ldo workspace workspace_bytes stream",
    "mq_gemm_w4a8_rank2_ws": "a lda w w_bits M N K_pad s_x0 s_x1 row_sel s_x_rows s_w bias x0 w0 x1 w1 out out_dtype ldo workspace "
                             "workspace_bytes stream",
    "mq_gemm_w4a8_groupscale": "a lda w w_bits M N K_pad s_x_groups n_groups group_k s_w bias out out_dtype ldo stream",
    "mq_gemm_w4a8_groupscale_asym": "a lda w w_bits M N K_pad s_x_groups shift_groups wsum_groups n_groups group_k s_w bias out out_dtype "
                                    "ldo stream",
    "mq_gemm_w4a8_wgroupscale": "a lda w w_bits M N K_pad s_w_groups n_groups group_k s_x0 s_x1 row_sel s_x_rows s_x_groups bias out "
                                "out_dtype ldo stream",
    "mq_gemm_w4a8_i32": "a lda w w_bits M N K_pad acc ldacc stream",
    "mq_gemm_w4a8_i32_ws": "a lda w w_bits M N K_pad acc ldacc workspace workspace_bytes stream",
}

# a well-formed call of every entry point (64 x 256 x 512, tiled activations, fp16 output); a table row overrides what it violates
BASE = dict(
    a=P, lda=TILED, w=P, w_bits=4, M=64, N=256, K_pad=512, s_x0=0.5, s_x1=0.5, row_sel=None, s_w=P, bias=P, x0=None, w0=None,
    out=P, out_dtype=F16, ldo=256, workspace=None, workspace_bytes=0, stream=None, acc=P, ldacc=256, act=QUICK_GELU,
    rope_cos=P, rope_sin=P, rope_cols=128, head_dim=128, n_groups=4, group_k=128,
)
PER_FN = {
    "mq_gemm_w4a8_residual_ws": dict(residual=P, ldr=256),
    "mq_gemm_w4a8_act_ws": dict(s_x_rows=None),
    "mq_gemm_w4a8_rowscale_ws": dict(s_x_rows=P),
    "mq_gemm_w4a8_rank2_ws": dict(s_x_rows=None, x0=P, w0=P, x1=P, w1=P),
    "mq_gemm_w4a8_groupscale": dict(s_x_groups=P),
    "mq_gemm_w4a8_groupscale_asym": dict(s_x_groups=P, shift_groups=P, wsum_groups=P),
    "mq_gemm_w4a8_wgroupscale": dict(s_w_groups=P, s_x_rows=None, s_x_groups=None),
}
NO_BUFFERS = dict(a=None, w=None, out=None, s_w=None, bias=None)
FLOAT_OUT = [f for f in PARAMS if "out_dtype" in PARAMS[f] and f != "mq_gemm_w4a8_rope_ws"]      # the nine with the three-dtype test
EARLY_OUT = [f for f in FLOAT_OUT + ["mq_gemm_w4a8_rope_ws"] if f not in ("mq_gemm_w4a8", "mq_gemm_w4a8_ws")]

G, GA, WG = "mq_gemm_w4a8_groupscale", "mq_gemm_w4a8_groupscale_asym", "mq_gemm_w4a8_wgroupscale"
ROPE, ACT, WS, RES = "mq_gemm_w4a8_rope_ws", "mq_gemm_w4a8_act_ws", "mq_gemm_w4a8_ws", "mq_gemm_w4a8_residual_ws"

# (entry point, what the call violates, overrides of the well-formed call, (tile, splits) for mq_gemm_debug_force or None)
CALLS = (
    # ---- the output dtype comes first, before M == 0 || N == 0 and before any pointer is looked at
    [(f, "bad dtype", dict(out_dtype=3), None) for f in FLOAT_OUT]
    + [(f, "bad dtype, no rows", dict(out_dtype=7, M=0, **NO_BUFFERS), None) for f in FLOAT_OUT]
    + [(ROPE, "fp32 output", dict(out_dtype=F32), None),
       (ROPE, "fp32 output, no rows", dict(out_dtype=F32, M=0), None),
       (ROPE, "head_dim 64", dict(head_dim=64), None),
       (ROPE, "head_dim 64, no rows", dict(head_dim=64, M=0), None)]
    # ---- M == 0 || N == 0: MQ_OK before the required pointers and the buffers
    + [(f, "no rows, nothing else", dict(M=0, **NO_BUFFERS, residual=None, rope_cos=None, rope_sin=None, s_x_rows=None, x0=None, w0=None,
                                         x1=None, w1=None, s_x_groups=None, shift_groups=None, wsum_groups=None, s_w_groups=None,
                                         n_groups=0, lda=512), None) for f in EARLY_OUT]
    + [(f, "no channels", dict(N=0, **NO_BUFFERS), None) for f in ("mq_gemm_w4a8", WS, "mq_gemm_w4a8_i32", "mq_gemm_w4a8_i32_ws")]
    # ---- the pointers an entry point requires
    + [(RES, "no residual", dict(residual=None), None),
       (ROPE, "no cos table", dict(rope_cos=None), None),
       (ROPE, "no sin table", dict(rope_sin=None), None),
       (ACT, "row-major activations", dict(lda=512), None),
       ("mq_gemm_w4a8_rowscale_ws", "no row scales", dict(s_x_rows=None), None),
       ("mq_gemm_w4a8_rank2_ws", "no x1", dict(x1=None), None),
       ("mq_gemm_w4a8_rank2_ws", "no w0", dict(w0=None), None),
       (G, "no group scales", dict(s_x_groups=None), None),
       (G, "no groups", dict(n_groups=0), None),
       (GA, "no shifts", dict(shift_groups=None), None),
       (GA, "no weight sums", dict(wsum_groups=None), None),
       (WG, "no weight group scales", dict(s_w_groups=None), None),
       (WG, "activation groups with row scales", dict(s_x_groups=P, s_x_rows=P), None),
       (WG, "activation groups with token types", dict(s_x_groups=P, row_sel=P), None)]
    # ---- groups that do not cover K_pad
    + [(f, "groups past K_pad", dict(n_groups=5), None) for f in (G, GA, WG)]
    + [(f, "groups short of K_pad", dict(n_groups=2), None) for f in (G, GA, WG)]
    + [(f, "group size 96", dict(group_k=96, n_groups=4, K_pad=384), None) for f in (G, GA, WG)]
    # ---- gemm_common: shapes and buffers
    + [("mq_gemm_w4a8", "negative M", dict(M=-1), None),
       ("mq_gemm_w4a8_i32", "negative K_pad", dict(K_pad=-128), None),
       ("mq_gemm_w4a8", "null a", dict(a=None), None),
       (WS, "null w", dict(w=None), None),
       ("mq_gemm_w4a8_i32", "null acc", dict(acc=None), None),
       (RES, "null out", dict(out=None), None),
       ("mq_gemm_w4a8", "K_pad 100", dict(K_pad=100), None),
       ("mq_gemm_w4a8_i32_ws", "K_pad 0", dict(K_pad=0), None),
       ("mq_gemm_w4a8_rowscale_ws", "K_pad 576", dict(K_pad=576), None),
       ("mq_gemm_w4a8", "misaligned a", dict(a=P + 8), None),
       (WS, "lda < K_pad", dict(lda=496), None),
       ("mq_gemm_w4a8_i32", "lda % 16", dict(lda=520), None),
       ("mq_gemm_w4a8", "misaligned w", dict(w=P + 4), None),
       (ACT, "misaligned w", dict(w=P + 8), None),
       ("mq_gemm_w4a8", "w_bits 5", dict(w_bits=5), None),
       (G, "w_bits 2", dict(w_bits=2), None),
       ("mq_gemm_w4a8", "ldo < N", dict(ldo=248), None),
       ("mq_gemm_w4a8_i32", "ldacc < N", dict(ldacc=255), None),
       (ACT, "silu: ldo < N / 2", dict(act=SILU_MUL, ldo=120), None),
       ("mq_gemm_w4a8", "no s_w", dict(s_w=None), None),
       ("mq_gemm_w4a8_rowscale_ws", "no s_w", dict(s_w=None), None),
       (G, "no s_w", dict(s_w=None), None),
       ("mq_gemm_w4a8", "x0 without w0", dict(x0=P), None),
       (WS, "w0 without x0", dict(w0=P), None),
       ("mq_gemm_w4a8_rowscale_ws", "x0 without w0", dict(x0=P), None),
       ("mq_gemm_w4a8", "K too large", dict(K_pad=131072 + 128), None),
       (WS, "misaligned workspace", dict(workspace=P + 8, workspace_bytes=1 << 20), None),
       ("mq_gemm_w4a8_i32_ws", "misaligned workspace", dict(workspace=P + 4, workspace_bytes=1 << 20), None),
       (RES, "ldr < N", dict(ldr=128), None)]
    # ---- gemm_common: the activation epilogue
    + [(ACT, "unknown activation", dict(act=3), None),
       (ACT, "silu: N % 64", dict(act=SILU_MUL, N=96, ldo=96), None),
       (ACT, "N % 8", dict(N=252, ldo=256), None),
       (ACT, "ldo % 8", dict(ldo=260), None),
       (ACT, "misaligned out", dict(out=P + 8), None),
       (ACT, "misaligned s_w", dict(s_w=P + 4), None),
       (ACT, "misaligned bias", dict(bias=P + 4), None)]
    # ---- gemm_common: RoPE in the store
    + [(ROPE, "row-major activations", dict(lda=512), None),
       (ROPE, "rope_cols 64", dict(rope_cols=64), None),
       (ROPE, "rope_cols > N", dict(rope_cols=384), None),
       (ROPE, "N % 8", dict(N=252, ldo=256), None),
       (ROPE, "misaligned cos table", dict(rope_cos=P + 8), None),
       (ROPE, "misaligned out", dict(out=P + 8), None)]
    # ---- forced plans (mq_gemm_debug_force): what the dispatchers refuse before a launch
    + [(WS, "forced split-K, small workspace", dict(workspace=P, workspace_bytes=1024), (-1, 4)),
       ("mq_gemm_w4a8", "wave-specialised tile, row-major", dict(lda=512), (45, 0)),
       ("mq_gemm_w4a8_i32", "ping-pong tile, row-major", dict(lda=512), (14, 0)),
       ("mq_gemm_w4a8", "unknown wave-specialised id", {}, (49, 0)),
       ("mq_gemm_w4a8", "weight-streaming kernel, 100 rows", dict(M=100), (60, 0)),
       ("mq_gemm_w4a8", "eight-wave weight-streaming kernel, 40 rows", dict(M=40), (61, 0))]
)

UNSUPPORTED_DTYPE = "mq_gemm_w4a8_rope_ws: the rotation is defined on a 16-bit output (dtype 2)"
HEAD_DIM = "mq_gemm_w4a8_rope_ws: head_dim 64 (the fused form needs 128 = one output tile; use mq_rope_inplace)"
LDA = "mq_gemm_w4a8: activations must be 16-byte aligned with lda % 16 == 0 and lda >= K_pad (or lda = MQ_LD_TILED)"
ROPE_NEEDS = ("mq_gemm_w4a8_rope_ws: needs tiled activations, a 16-bit 16-byte aligned output with N and ldo multiples of 8, heads of 128 "
              "(rope_cols a multiple of 128, at most N) and 16-byte aligned tables")
ACT_OUT = "mq_gemm_w4a8_act_ws: output columns and ldo must be multiples of 8, out 16-byte aligned"
ACT_PAR = "mq_gemm_w4a8_act_ws: s_w and bias must be 16-byte aligned"
TILED_ONLY = "mq_gemm_w4a8: tile %d needs activations in the tiled layout (lda = MQ_LD_TILED)"

# (status, mq_last_error()) of every row of CALLS, in order; None: the call succeeds and leaves the message alone
EXPECTED = (
    [(EINVAL, f"{f}: unknown output dtype 3") for f in FLOAT_OUT]
    + [(EINVAL, f"{f}: unknown output dtype 7") for f in FLOAT_OUT]
    + [(EINVAL, UNSUPPORTED_DTYPE), (EINVAL, UNSUPPORTED_DTYPE), (EUNSUPPORTED, HEAD_DIM), (EUNSUPPORTED, HEAD_DIM)]
    + [(OK, None)] * len(EARLY_OUT)
    + [(OK, None)] * 4
    + [(EINVAL, "mq_gemm_w4a8_residual_ws: residual is required"),
       (EINVAL, "mq_gemm_w4a8_rope_ws: the cos / sin tables are required"),
       (EINVAL, "mq_gemm_w4a8_rope_ws: the cos / sin tables are required"),
       (EUNSUPPORTED, "mq_gemm_w4a8_act_ws: needs activations in the tiled layout (lda = MQ_LD_TILED)"),
       (EINVAL, "mq_gemm_w4a8_rowscale_ws: s_x_rows is required"),
       (EINVAL, "mq_gemm_w4a8_rank2_ws: both rank-1 terms are required (one term: mq_gemm_w4a8_ws)"),
       (EINVAL, "mq_gemm_w4a8_rank2_ws: both rank-1 terms are required (one term: mq_gemm_w4a8_ws)"),
       (EINVAL, "mq_gemm_w4a8_groupscale: s_x_groups is required"),
       (EINVAL, "mq_gemm_w4a8_groupscale: s_x_groups is required"),
       (EINVAL, "mq_gemm_w4a8_groupscale_asym: s_x_groups, shift_groups and wsum_groups are required"),
       (EINVAL, "mq_gemm_w4a8_groupscale_asym: s_x_groups, shift_groups and wsum_groups are required"),
       (EINVAL, "mq_gemm_w4a8_wgroupscale: s_w_groups is required"),
       (EINVAL, "mq_gemm_w4a8_wgroupscale: group-wise activation scales exclude per-row / per-token-type scales"),
       (EINVAL, "mq_gemm_w4a8_wgroupscale: group-wise activation scales exclude per-row / per-token-type scales")]
    + [(EINVAL, f"{f}: 5 groups of 128 do not cover K_pad=512") for f in (G, GA, WG)]
    + [(EINVAL, f"{f}: 2 groups of 128 do not cover K_pad=512") for f in (G, GA, WG)]
    + [(EINVAL, "mq_gemm_w4a8_groupscale: group size 96 (64 or a multiple of 128)")] * 3
    + [(EINVAL, "mq_gemm_w4a8: negative shape"),
       (EINVAL, "mq_gemm_w4a8: negative shape"),
       (EINVAL, "mq_gemm_w4a8: null buffer"),
       (EINVAL, "mq_gemm_w4a8: null buffer"),
       (EINVAL, "mq_gemm_w4a8: null buffer"),
       (EINVAL, "mq_gemm_w4a8: null buffer"),
       (EINVAL, "mq_gemm_w4a8: K_pad=100 must be a positive multiple of 128"),
       (EINVAL, "mq_gemm_w4a8: K_pad=0 must be a positive multiple of 128"),
       (EINVAL, "mq_gemm_w4a8: K_pad=576 must be a positive multiple of 128"),
       (EINVAL, LDA),
       (EINVAL, LDA),
       (EINVAL, LDA),
       (EINVAL, "mq_gemm_w4a8: weight image must be 16-byte aligned"),
       (EINVAL, "mq_gemm_w4a8: weight image must be 16-byte aligned"),
       (EINVAL, "mq_gemm_w4a8: w_bits must be 4 or 8"),
       (EINVAL, "mq_gemm_w4a8: w_bits must be 4 or 8"),
       (EINVAL, "mq_gemm_w4a8: ldo < N"),
       (EINVAL, "mq_gemm_w4a8: ldo < N"),
       (EINVAL, "mq_gemm_w4a8: ldo < N"),
       (EINVAL, "mq_gemm_w4a8: s_w is required"),
       (EINVAL, "mq_gemm_w4a8: s_w is required"),
       (EINVAL, "mq_gemm_w4a8: s_w is required"),
       (EINVAL, "mq_gemm_w4a8: x0 and w0 go together"),
       (EINVAL, "mq_gemm_w4a8: x0 and w0 go together"),
       (EINVAL, "mq_gemm_w4a8: x0 and w0 go together"),
       (EINVAL, "mq_gemm_w4a8: K too large for int32 accumulation"),
       (EINVAL, "mq_gemm_w4a8: workspace must be 16-byte aligned"),
       (EINVAL, "mq_gemm_w4a8: workspace must be 16-byte aligned"),
       (EINVAL, "mq_gemm_w4a8: bad residual geometry")]
    + [(EINVAL, "mq_gemm_w4a8_act_ws: unknown activation 3"),
       (EINVAL, "mq_gemm_w4a8_act_ws: silu(gate)*up needs N = 2 x (a multiple of 32) channels, gate then up (N = 96)"),
       (EINVAL, ACT_OUT),
       (EINVAL, ACT_OUT),
       (EINVAL, ACT_OUT),
       (EINVAL, ACT_PAR),
       (EINVAL, ACT_PAR)]
    + [(EINVAL, ROPE_NEEDS)] * 6
    + [(EINVAL, "mq_gemm_w4a8: workspace too small for split-K"),
       (EINVAL, TILED_ONLY % 45),
       (EINVAL, TILED_ONLY % 14),
       (EINVAL, "gemm_ws: unknown tile 49"),
       (EINVAL, "gemm_skinny: needs tiled activations, 1 <= M <= 64 and at most 65535 channel blocks"),
       (EINVAL, "gemm_skinny_wg: needs tiled activations, 1 <= M <= 32, K_pad >= 512")]
)

UNTOUCHED = "left by the test"


def refusal(fn, overrides, force):
    """(status, message) of one call; the message is None when the call left the thread's last error alone."""
    lib = _lib.load()
    values = {**BASE, **PER_FN.get(fn, {}), **overrides}
    args = [values[name] for name in PARAMS[fn].split()]
    lib.mq_gemm_debug_plan(0, 0, 0, 4, 0, 0, None, None)              # a refused call of its own: sets a known last error
    known = lib.mq_last_error()
    if force is not None:
        lib.mq_gemm_debug_force(*force)
    try:
        rc = getattr(lib, fn)(*args)
    finally:
        lib.mq_gemm_debug_force(-1, 0)
    msg = lib.mq_last_error()
    return rc, (None if msg == known else msg.decode())


def test_the_table_and_its_expectations_line_up():
    assert len(CALLS) == len(EXPECTED)
    assert set(PARAMS) == {f for f, *_ in CALLS}, "every entry point has rows"
    for fn, names in PARAMS.items():
        assert len(names.split()) == len(_lib.SIGNATURES[fn][1]), fn
    for (fn, what, _, force), (rc, msg) in zip(CALLS, EXPECTED):
        # nothing in the table may get as far as a launch: it is refused, or it has no rows / channels
        assert rc != OK or what.startswith(("no rows", "no channels")), (fn, what)
        assert rc == OK or force is not None or msg.startswith(("mq_gemm_w4a8: ", "mq_gemm_w4a8_groupscale: ", fn + ": ")), (fn, what)


@pytest.mark.parametrize("i", range(len(CALLS)), ids=[f"{f[len('mq_gemm_'):]}-{what}".replace(" ", "_") for f, what, _, _ in CALLS])
def test_refusal(i):
    fn, what, overrides, force = CALLS[i]
    assert refusal(fn, overrides, force) == EXPECTED[i], (fn, what)
