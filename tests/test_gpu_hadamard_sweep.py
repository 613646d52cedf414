"""GPU sweep of the exact online Hadamard (csrc/hadamard.hip) through the C ABI: every case of hadamard_cases.py -- each path the
launch plan (mq_hadamard_debug_plan) can return, at forced 256 / 512 threads and unforced, sign words and prepared descriptor --
against the CPU oracle, bit for bit.  No tolerance anywhere:

  * plain transform: the output's BIT PATTERNS equal oracle.hadamard's (integer views: the sign of a zero counts).  Every case
    has an all-zero row.  The reference's own outputs (tests/golden/hadamard_fwd.npz, held by test_gpu_kernels.py) contain no
    exact zero, so they cannot arbitrate a zero's sign; the oracle's +0 (a sum of +0 terms) is what the kernel must give.
  * fused quantizer: levels == oracle.quant_static(oracle.hadamard(...)), x0_out == the rotated column 0 (bits), column 0 of the
    image zero with skip_col0, the n .. K_pad tail zero, the tiled image read back row-major, bytes around an out= slice untouched.
  * fused activations: equal to the unfused kernel on the torch composition (the bar of test_gpu_act_hadamard.py; the oracle's exp
    is not the device's), and that unfused result equal to the oracle on the activated tensor.
  * ties and near-ties of the fused quantizer: one-hot rows a * e_i rotate to +-fl(a * fl(1 / sqrt n)) in every column; the
    amplitudes are searched on the host so that whole rows sit on exact half-integer quotients, or where the reciprocal product
    and the IEEE quotient round differently (hadamard_cases.tie_rows; the shares are asserted in the CPU test).

Every assertion message carries the plan's answer for the live device, and the last test asserts that the sweep as run here met
every path key of the accepted domain (the M ladder is computed from the device's CU count).

Wall time on an MI355X: 23.8 s for the 2795 tests of this file (most of it the CPU oracle and pytest's per-test overhead), next to
9.3 s for the 62 tests of tests/test_gpu_gemm_sweep.py on the same machine."""
import numpy as np
import pytest
import torch

import hadamard_cases as hc
import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
INT_VIEW = {"f16": torch.int16, "bf16": torch.int16, "f32": torch.int32}
FILL = 0x55

CASES = hc.cases()
RAN, SEEN = set(), set()
_SIGNS = {}


def signs(had_table, K, prepared):
    """Sign words, or the prepared descriptor, of hadK on the device (None for K = 1)."""
    from mquant_amd import ops
    if K == 1:
        return None
    if (K, 0) not in _SIGNS:
        _SIGNS[(K, 0)] = torch.from_numpy(np.ascontiguousarray(had_table["words"][K])).to(DEV)
        _SIGNS[(K, 1)] = ops.hadamard_prepare(_SIGNS[(K, 0)], K)
    return _SIGNS[(K, int(prepared))]


def ceil8(v):
    return (v + 7) // 8 * 8


def place(xs, dtype, aligned):
    """The fp32 row blocks ``xs`` (one, or gate and up) as column slices of ONE device tensor of ``dtype`` (same row stride), laid
    out as ``aligned`` asks."""
    M, n_in = xs[0].shape
    first = 0 if aligned in ("a", "q4", "q2", "ldx") else 1
    offs = [first]
    for _ in xs[1:]:
        nxt = ceil8(offs[-1] + n_in)
        offs.append(nxt if aligned in ("a", "q4", "q2", "ldx", "x2ok") else nxt + 1)
    W = ceil8(offs[-1] + n_in)
    if aligned == "ldx":
        W += 1              # (W * element size) % 16 != 0 for 2- and 4-byte elements
    wide = torch.zeros((M, W), dtype=TORCH_DT[dtype])
    for o, x in zip(offs, xs):
        wide[:, o:o + n_in] = torch.from_numpy(x).to(TORCH_DT[dtype])
    wide = wide.to(DEV)
    views = [wide[:, o:o + n_in] for o in offs]
    esz = wide.element_size()
    vec = [v.data_ptr() % 16 == 0 and (W * esz) % 16 == 0 for v in views]
    assert vec[0] == (aligned in ("a", "q4", "q2")) and (aligned != "x2ok" or vec[1])
    return views


def destination(c, K_pad):
    """(out argument, the whole buffer, column offset) of a quantizing case, prefilled so that an unwritten byte shows."""
    from mquant_amd import ops
    if c.tiled:
        out = ops.TiledAct.empty(c.M, K_pad, DEV)
        out.data.fill_(FILL)
        return out, None, 0
    if c.aligned in ("q4", "q2"):
        buf = torch.full((c.M, K_pad + (20 if c.aligned == "q4" else 18)), FILL, dtype=torch.int8, device=DEV)
        out = buf[:, 4:4 + K_pad]
        assert out.data_ptr() % 16 == 4 and out.stride(0) % 16 == (4 if c.aligned == "q4" else 2)
        return out, buf, 4
    return torch.full((c.M, K_pad), FILL, dtype=torch.int8, device=DEV), None, 0


def bits_of(t):
    return t.contiguous().view(INT_VIEW[{torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}[t.dtype]]).cpu().numpy()


def ref_bits(ref, dtype):
    return bits_of(torch.from_numpy(np.ascontiguousarray(ref)).to(TORCH_DT[dtype]))


def check_quant(c, msg, out, buf, x0, rot, s0, s1, sel):
    n = c.n
    want = oracle.quant_static(rot, s0, scale1=s1, row_sel=sel) if c.quant >= 2 else oracle.quant_static(rot, s0)
    if c.quant == 3:
        want[:, 0] = 0
        np.testing.assert_array_equal(x0.cpu().numpy().view(np.int32), np.ascontiguousarray(rot[:, 0]).view(np.int32), err_msg=msg)
    got = (out.to_rows() if c.tiled else out).cpu().numpy()
    np.testing.assert_array_equal(got[:, :n], want, err_msg=msg)
    assert not got[:, n:].any(), msg
    if buf is not None:
        whole = buf.cpu().numpy()
        assert (whole[:, :4] == FILL).all() and (whole[:, 4 + got.shape[1]:] == FILL).all(), msg


def run_case(c, had_table):
    from mquant_amd import ops
    p = hc.plan(c)
    msg = f"{c.name}: {hc.describe(p)}"
    hk = had_table["mats"].get(c.K)
    sg = signs(had_table, c.K, c.prepared)
    K_pad = ops.ceil_to(c.n, 128)
    fp32_had = bool(c.fp32_had)
    sel = hc.row_sel(c.M)
    sel_dev = torch.from_numpy(sel).to(DEV) if c.quant >= 2 else None
    hc.lib().mq_hadamard_debug_threads(c.threads)
    try:
        if c.act:
            g = hc.make_rows(c) * np.float32(2.0)
            xs = [hc.round_dtype(g, c.dtype)] + ([hc.make_rows(c, 1)] if c.act == ops.ACT_SILU_MUL else [])
            views = place(xs, c.dtype, c.aligned)
            gate, up = views[0], (views[1] if len(views) > 1 else None)
            act_x = (torch.nn.functional.silu(gate) * up if up is not None else gate * torch.sigmoid(1.702 * gate)).contiguous()
            rot = hc.rotate(act_x.float().cpu().numpy(), c.n, c.K, hk, c.dtype, fp32_had)
            s0, s1 = hc.scales(rot)
            kw = dict(fp32_had=fp32_had, row_sel=sel_dev, skip_col0=c.quant == 3)
            s1_arg = float(s1) if c.quant >= 2 else None
            out, buf, _ = destination(c, K_pad)
            out, x0 = ops.act_hadamard_quant_i8(gate, up, c.act, c.n, c.K, sg, float(s0), s1_arg, out=out, **kw)
            out_u, buf_u, _ = destination(c, K_pad)
            out_u, x0_u = ops.hadamard_quant_i8(act_x, c.n, c.K, sg, float(s0), s1_arg, out=out_u, **kw)
            torch.cuda.synchronize()
            a, b = (out.to_rows(), out_u.to_rows()) if c.tiled else (out, out_u)
            assert torch.equal(a, b), msg
            if c.quant == 3:
                assert torch.equal(x0.view(torch.int32), x0_u.view(torch.int32)), msg
            check_quant(c, msg + " (unfused kernel on the torch composition)", out_u, buf_u, x0_u, rot, s0, s1, sel)
            return p
        x_np = hc.make_rows(c)
        rot = hc.rotated(c, had_table["mats"])
        x = place([x_np], c.dtype, c.aligned)[0]
        if not c.quant:
            y = ops.hadamard(x, c.n, c.K, sg, fp32_had=fp32_had)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(bits_of(y), ref_bits(rot, c.dtype), err_msg=msg)
            assert not bits_of(y)[1].any() if c.M > 1 else True, msg          # the all-zero row: +0 everywhere
            return p
        s0, s1 = hc.scales(rot)
        out, buf, _ = destination(c, K_pad)
        out, x0 = ops.hadamard_quant_i8(x, c.n, c.K, sg, float(s0), float(s1) if c.quant >= 2 else None, fp32_had=fp32_had,
                                        row_sel=sel_dev, skip_col0=c.quant == 3, out=out)
        torch.cuda.synchronize()
        check_quant(c, msg, out, buf, x0, rot, s0, s1, sel)
        return p
    finally:
        hc.lib().mq_hadamard_debug_threads(0)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_equals_the_oracle(had_table, c):
    p = run_case(c, had_table)
    RAN.add(c.name)
    SEEN.add(tuple(p[f] for f in hc.KEY_FIELDS))


TIES = [(sh, dtype, s, tiled)
        for sh in hc.TIE_SHAPES
        for dtype, ss in (("f32", hc.TIE_SCALES_F32), ("f16", hc.TIE_SCALES_16), ("bf16", hc.TIE_SCALES_16))
        for i, s in enumerate(ss) for tiled in ((False, True) if i == 0 else (i % 2 == 1,))]


@pytest.mark.parametrize("shape,dtype,s,tiled", TIES, ids=[f"{sh[1]}x{sh[2]}|{dt}|s{s:g}|{'t' if t else 'r'}" for sh, dt, s, t in TIES])
def test_ties_and_near_ties_of_the_fused_quantizer(had_table, shape, dtype, s, tiled):
    """Whole rows on exact half-integer quotients (both clamps included) and on quotient / reciprocal disagreements: the levels
    equal the oracle's on every element.  1280 = 40 x 32 takes the scalar chain, whose quantizer is the plain IEEE quotient
    (quant_level): the control."""
    from mquant_amd import ops
    n_in, n, K, prepared = shape
    x_np, n_ties = hc.tie_rows(n_in, n, K, dtype, s, step=2 if n > 8192 else 1)
    assert n_ties >= 8
    M = x_np.shape[0]
    c = hc.Case("ties", M, n_in, n, K, dtype, 0, 1, 0, prepared, tiled, 0, "a")
    msg = f"{n}x{K} {dtype} s={s}: {hc.describe(hc.plan(c))}"
    rot = hc.rotate(x_np, n, K, had_table["mats"].get(K), dtype, 0)
    x = torch.from_numpy(x_np).to(TORCH_DT[dtype]).to(DEV)
    out, buf, _ = destination(c, ops.ceil_to(n, 128))
    out, _ = ops.hadamard_quant_i8(x, n, K, signs(had_table, K, prepared), float(np.float32(s)), out=out)
    torch.cuda.synchronize()
    check_quant(c, msg, out, buf, None, rot, np.float32(s), None, None)


def test_refused_destination_of_the_unit_paths(had_table):
    """An odd row stride of a row-major int8 destination is refused where a prepared descriptor selects the mask-driven units
    (they store two levels at a time); the classic path takes it with byte stores."""
    from mquant_amd import ops
    from mquant_amd._lib import MQuantHipError
    n, K = 5120, 40
    x = torch.zeros((2, n), dtype=torch.float16, device=DEV)
    buf = torch.full((2, n + 1), FILL, dtype=torch.int8, device=DEV)
    with pytest.raises(MQuantHipError, match="even row stride"):
        ops.hadamard_quant_i8(x, n, K, signs(had_table, K, 1), 0.05, out=buf[:, :n])
    torch.cuda.synchronize()
    assert (buf == FILL).all()
    out, _ = ops.hadamard_quant_i8(x, n, K, signs(had_table, K, 0), 0.05, out=buf[:, :n])
    torch.cuda.synchronize()
    assert not buf[:, :n].any() and (buf[:, n] == FILL).all()


def test_the_sweep_met_every_path_key_of_this_device():
    """The case list was built for THIS device's CU count: its plans cover every path key of the accepted domain, and (when the
    whole file ran) every one of them was launched above."""
    want = set(hc.domain_keys(hc.cu_count()))
    planned = {hc.key(c) for c in CASES}
    assert planned == want, (sorted(want - planned)[:5], sorted(planned - want)[:5])
    if len(RAN) == len(CASES):
        assert SEEN == want, sorted(want - SEEN)[:5]
