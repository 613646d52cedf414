"""The activation quantizers on the shapes their other tests leave out: rows that are not 16-byte aligned (through the pointer or
through the stride), K that ends inside a 16-channel chunk, a zero tail of more than one store per row, whole and ragged 16-row
tiles, both destination layouts.  These are the paths of the load, pack, zero-tail and range code that the quantizers share
(csrc/act_quant_common.h), so every entry point is swept over all of them against its own function of the C oracle, bit for bit,
with the comparison its existing test uses.  Every int8 destination is filled with a sentinel first: the pad columns K .. K_pad
must come back zero, and for the row-major form every byte outside the [M, K_pad] image must come back untouched."""
import itertools

import numpy as np
import pytest
import torch

import oracle
from golden_inputs import make_x

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
MODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
MS = (1, 16, 17, 33)                       # one row, a whole 16-row tile, ragged tiles
KS = (64, 272, 65, 136, 271)               # K % 16 in {0, 0, 1, 8, 15}
ROWS = ("aligned", "offset", "stride")     # 16-byte aligned rows; a view one element in; a row stride that is not 16 bytes' multiple
SENTINEL = 0x5A
BITS, CLIP = 8, 0.9
S0, S1 = np.float32(0.043), np.float32(0.017)


def ceil_to(v, m):
    return (v + m - 1) // m * m


def vec_ok(x):
    """The host's rule for the 16-byte loads (rows_vec_ok in csrc/act_quant_common.h) on what the wrappers hand to the library:
    base and row stride multiples of 16 bytes."""
    x2 = x.reshape(-1, x.shape[-1])
    return x2.data_ptr() % 16 == 0 and (x2.stride(0) * x2.element_size()) % 16 == 0


def static_kernel(tiled, per_channel, aligned, K, M):
    """Which kernel mq_quantize_act_i8 launches: the condition in launch_act_quant (csrc/act_quant.hip) restated."""
    own = tiled and not per_channel and aligned and K % 16 == 0 and (M + 15) // 16 <= 65535
    return "act_quant_tiled_kernel" if own else "act_quant_kernel"


def layouts():
    """(rows, K_pad - ceil128(K), tiled) of one input: 3 x 2 x 2."""
    return itertools.product(ROWS, (0, 128), (False, True))


def place(x_np, dtype, rows):
    """x on the device as an [M, K] view with the requested row placement (the values are those of x_np rounded to dtype)."""
    M, K = x_np.shape
    ld = ceil_to(K, 16) + (1 if rows == "stride" else 0)
    off = 1 if rows == "offset" else 0
    buf = torch.full((off + M * ld,), 1000.0, dtype=dtype, device=DEV)      # what lies between and behind the rows must not be read as data
    view = buf[off:].view(M, ld)[:, :K]
    view.copy_(torch.from_numpy(x_np))
    assert view.stride(1) == 1
    if M > 1:                                                        # (one row has no stride: whatever torch reports for it goes)
        assert vec_ok(view) == (rows == "aligned"), (rows, M, K)
    else:
        assert not (rows == "offset" and vec_ok(view))
    return view


class Dest:
    """A sentinel-filled destination of M rows and K_pad columns, row-major inside a larger buffer or tiled."""

    def __init__(self, M, K, K_pad, tiled):
        from mquant_amd import ops
        self.M, self.K, self.K_pad, self.tiled = M, K, K_pad, tiled
        if tiled:
            self.out = ops.TiledAct.empty(M, K_pad, DEV)
            self.out.data.fill_(SENTINEL)
        else:
            self.buf = torch.full((M + 2, K_pad + 16), SENTINEL, dtype=torch.int8, device=DEV)      # a row above, a row below, 16 bytes beside
            self.out = self.buf[1:M + 1, :K_pad]

    def levels(self, got):
        """The [M, K] levels after checking the pad columns and, for the row-major form, everything around the image."""
        assert got is self.out
        rows = (self.out.to_rows() if self.tiled else self.out).cpu().numpy()
        assert rows.shape == (self.M, self.K_pad)
        assert not rows[:, self.K:].any(), "pad columns K .. K_pad must be zero"
        if not self.tiled:
            around = self.buf.cpu().numpy().copy()
            around[1:self.M + 1, :self.K_pad] = SENTINEL
            assert (around == SENTINEL).all(), "bytes outside the [M, K_pad] image were written"
        return rows[:, :self.K]


def data(seed, M, K, dtype):
    """fp32 values as the kernel sees them after the cast to dtype, with an all-zero row 1 and a non-negative row 2."""
    x = make_x(seed, (M, K))
    if M > 1:
        x[1] = 0
    if M > 2:
        x[2] = np.abs(x[2])
    return torch.from_numpy(x).to(dtype).float().numpy()


def sel_of(M):
    return (np.arange(M) % 3 == 0).astype(np.uint8)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def eq(got, want, what, case):
    np.testing.assert_array_equal(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want, err_msg=f"{what} {case}")


# (token types, per-channel scales, split column) of the static quantizer: the plain call, the prefill's call, and both with vectors
STATIC_MODES = [(False, False, False), (True, False, True), (False, True, False), (True, True, True)]


def static_reference(x, M, K, with_sel, per_channel):
    sel = sel_of(M) if with_sel else None
    if per_channel:
        s0 = (0.01 + 0.003 * np.arange(K)).astype(np.float32)
        s1 = (0.05 - 0.0001 * np.arange(K)).astype(np.float32)
    else:
        s0, s1 = S0, S1
    q = oracle.quant_static(x, s0, scale1=s1 if with_sel else None, row_sel=sel)
    return sel, s0, s1, q


def test_the_static_cases_reach_both_kernels():
    """With more than one row the placement decides the alignment, so the case list can be judged without a device."""
    picks = {static_kernel(tiled, pc, rows == "aligned", K, M) for M in MS[1:] for K in KS for _, pc, _ in STATIC_MODES
             for rows, _, tiled in layouts()}
    assert picks == {"act_quant_tiled_kernel", "act_quant_kernel"}
    assert static_kernel(True, False, True, 64, 17) == "act_quant_tiled_kernel"
    for other in (static_kernel(False, False, True, 64, 17), static_kernel(True, True, True, 64, 17),
                  static_kernel(True, False, False, 64, 17), static_kernel(True, False, True, 65, 17)):
        assert other == "act_quant_kernel"


@pytest.mark.parametrize("dtype", DTYPES)
def test_static_quantizer(dtype):
    from mquant_amd import ops
    reached = set()
    for M, K, (with_sel, per_channel, skip) in itertools.product(MS, KS, STATIC_MODES):
        x = data(M + K, M, K, dtype)
        sel, s0, s1, want = static_reference(x, M, K, with_sel, per_channel)
        if skip:
            want[:, 0] = 0
        for rows, extra, tiled in layouts():
            case = (M, K, with_sel, per_channel, skip, rows, extra, tiled)
            xd = place(x, dtype, rows)
            reached.add(static_kernel(tiled, per_channel, vec_ok(xd), K, M))
            d = Dest(M, K, ceil_to(K, 128) + extra, tiled)
            kw = dict(scale_vec0=dev(s0), scale_vec1=dev(s1) if with_sel else None) if per_channel else {}
            sc = () if per_channel else (float(s0), float(s1))
            q, x0 = ops.quantize_act_i8(xd, *sc, row_sel=dev(sel), skip_col0=skip, out=d.out, **kw)
            eq(d.levels(q), want, "levels", case)
            if skip:
                eq(x0, x[:, 0], "x0", case)
    assert reached == {"act_quant_tiled_kernel", "act_quant_kernel"}


@pytest.mark.parametrize("dtype", DTYPES)
def test_fakequant(dtype):
    from mquant_amd import ops
    for M, K, (with_sel, per_channel, skip) in itertools.product(MS, KS, STATIC_MODES):
        x = data(M + K + 1, M, K, dtype)
        sel, s0, s1, q = static_reference(x, M, K, with_sel, per_channel)
        want = oracle.round_to(oracle.dequant_static(q, s0, scale1=s1 if with_sel else None, row_sel=sel), MODE[dtype])
        if skip:
            want[:, 0] = x[:, 0]                                         # the split column passes through
        for rows in ROWS:
            kw = dict(scale_vec0=dev(s0), scale_vec1=dev(s1) if with_sel else None) if per_channel else {}
            sc = () if per_channel else (float(s0), float(s1))
            y = ops.fakequant_act(place(x, dtype, rows), *sc, row_sel=dev(sel), skip_col0=skip, **kw)
            assert y.shape == (M, K) and y.dtype == dtype
            eq(y.float(), want, "values", (M, K, with_sel, per_channel, skip, rows))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dynamic_per_token(dtype):
    from mquant_amd import ops
    for M, K, skip in itertools.product(MS, KS, (False, True)):
        x = data(M * 3 + K, M, K, dtype)
        want_q, want_s = oracle.quant_dyn(x, bits=BITS, clip=CLIP, skip_col0=skip)
        for rows, extra, tiled in layouts():
            case = (M, K, skip, rows, extra, tiled)
            d = Dest(M, K, ceil_to(K, 128) + extra, tiled)
            q, s, x0 = ops.quantize_act_dyn_i8(place(x, dtype, rows), BITS, CLIP, skip_col0=skip, out=d.out)
            eq(s, want_s, "scales", case)
            eq(d.levels(q), want_q, "levels", case)
            if skip:
                eq(x0, x[:, 0], "x0", case)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dynamic_per_token_asymmetric(dtype):
    from mquant_amd import ops
    for M, K in itertools.product(MS, KS):
        x = data(M * 5 + K, M, K, dtype)
        want_q, want_s, want_z, want_sh = oracle.quant_dyn_asym(x, bits=BITS, clip=CLIP)
        for rows, extra, tiled in layouts():
            case = (M, K, rows, extra, tiled)
            d = Dest(M, K, ceil_to(K, 128) + extra, tiled)
            q, s, z, sh = ops.quantize_act_dyn_asym_i8(place(x, dtype, rows), BITS, CLIP, out=d.out)
            eq(s, want_s, "scales", case)
            eq(z, want_z, "zero points", case)
            eq(sh, want_sh, "shifts", case)
            eq(d.levels(q), want_q, "levels", case)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dynamic_per_tensor(dtype):
    from mquant_amd import ops
    for M, K, (asym, skip) in itertools.product(MS, KS, ((False, False), (False, True), (True, False))):
        x = data(M * 7 + K, M, K, dtype)
        if M == 16:
            x = np.abs(x)                                                # xmin == 0 alone: the per-tensor rule makes it -1
        want_q, want_s, want_z, want_sh = oracle.quant_tensor(x, bits=BITS, clip=CLIP, asym=asym, skip_col0=skip, mode=MODE[dtype])
        for rows, extra, tiled in layouts():
            case = (M, K, asym, skip, rows, extra, tiled)
            d = Dest(M, K, ceil_to(K, 128) + extra, tiled)
            q, s, z, sh, x0 = ops.quantize_act_tensor_i8(place(x, dtype, rows), BITS, CLIP, asym=asym, skip_col0=skip, out=d.out)
            eq(s, np.full(M, want_s, np.float32), "scales", case)
            eq(d.levels(q), want_q, "levels", case)
            if asym:
                eq(z, np.full(M, want_z, np.float32), "zero points", case)
                eq(sh, np.full(M, want_sh, np.float32), "shifts", case)
            if skip:
                eq(x0, x[:, 0], "x0", case)


def group_sizes(K):
    return [g for g in (16, 64) if K % g == 0]


@pytest.mark.parametrize("asym", [False, True], ids=["sym", "asym"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_wise(dtype, asym):
    from mquant_amd import ops
    from mquant_amd._lib import MQuantHipError
    fn = ops.quantize_act_group_asym_i8 if asym else ops.quantize_act_group_i8
    for M, K in itertools.product(MS, KS):
        x = data(M + K + 16, M, K, dtype)
        if K % 16:
            # K has to hold whole groups of at least 16 channels
            for rows, extra, tiled in layouts():
                with pytest.raises(MQuantHipError, match="groupsize=16 must be a power of two in 16..1024 that divides K"):
                    fn(place(x, dtype, rows), 16, BITS, CLIP, out=Dest(M, K, ceil_to(K, 128) + extra, tiled).out)
            continue
        for g in group_sizes(K):
            x[0, :g] = 0                                                 # an all-zero group
            want = (oracle.quant_group_asym if asym else oracle.quant_group)(x, g, BITS, CLIP, MODE[dtype])
            for rows, extra, tiled in layouts():
                case = (M, K, g, rows, extra, tiled)
                d = Dest(M, K, ceil_to(K, 128) + extra, tiled)
                got = fn(place(x, dtype, rows), g, BITS, CLIP, out=d.out)
                for name, a, b in zip(("scales", "zero points", "shifts"), got[1:], want[1:]):
                    eq(a, b, name, case)
                eq(d.levels(got[0]), want[0], "levels", case)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsn(dtype):
    from mquant_amd import ops
    from mquant_amd._lib import MQuantHipError
    for M, K in itertools.product(MS, KS):
        x = data(M + K, M, K, dtype)
        sel = sel_of(M)
        if K % 16 == 0:
            want_y = oracle.rmsn(x, K, 1e-6, MODE[dtype])
            want_q = oracle.quant_static(want_y, S0, scale1=S1, row_sel=sel)
        for rows, extra, tiled in layouts():
            case = (M, K, rows, extra, tiled)
            d = Dest(M, K, ceil_to(K, 128) + extra, tiled)
            xd = place(x, dtype, rows)
            call = lambda: ops.rmsn_quantize_i8(xd, K, 1e-6, float(S0), float(S1), row_sel=dev(sel), out=d.out, want_y=True)  # noqa: E731
            if K % 16:
                with pytest.raises(MQuantHipError, match="K must be a multiple of 16"):
                    call()
            elif not vec_ok(xd):
                with pytest.raises(MQuantHipError, match="x rows must be 16-byte aligned"):
                    call()
            else:
                q, y = call()
                eq(y.float(), want_y, "normalised rows", case)
                eq(d.levels(q), want_q, "levels", case)
