"""ASYMMETRIC group-wise weights on the integer path (mq_act_group_rowsum_i32 + mq_gemm_w4a8_wgroupscale_asym): the kernels against
the restatement acc' = acc + d r bit for bit -- int4 through the unchanged oracle over the levels q - z, int8 (q - z does not fit
int8) through numpy --, and the wrapper over the reference's own asymmetric GPTQ weights, scales and zero points against the
reference's forward (tests/golden/wrapper_wgasym_*.npz, tools/gen_golden_wgroup_asym.py).  One sweeping test per property, each
naming every failing configuration."""
import itertools
import types

import numpy as np
import pytest
import torch

import oracle
from golden_inputs import make_w, make_x
from test_wgroup_asym_cpu import act_scales, cases, parts_of, wrapper_from_golden
from test_wgroup_cpu import DT, TOL, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
MODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
SHAPES = [(37, 200, 1280, 128), (33, 72, 192, 64), (300, 264, 1920, 64), (130, 260, 1024, 256), (16, 48, 2048, 512)]


def sweep(check, *axes):
    """``check`` over the product of ``axes`` in ONE test that names every failing configuration."""
    bad = []
    for case in itertools.product(*axes):
        try:
            check(*case)
        except AssertionError as e:
            bad.append((case, str(e).strip().splitlines()[:4]))
    assert not bad, bad


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def restate(a, stored, d, s_wg, g, bias=None, sx0=1.0, sx1=None, row_sel=None, sx_rows=None, s_xg=None):
    """mq_gemm_w4a8_wgroupscale_asym in numpy, one fp32 rounding per written operation: a int8 [M, K], stored levels int8 [N, K],
    d int16 [G, N].  Returns (y fp32, acc' int64 [M, G, N])."""
    M, K = a.shape
    N, G = stored.shape[0], K // g
    a64 = a.astype(np.int64).reshape(M, G, g)
    acc = np.einsum("mgk,ngk->mgn", a64, stored.astype(np.int64).reshape(N, G, g)) + a64.sum(axis=2)[:, :, None] * d.astype(np.int64)[None]
    assert np.abs(acc).max() < 2 ** 24                                   # float(acc') is exact
    f = np.zeros((M, N), np.float32)
    for gi in range(G):
        t = acc[:, gi, :].astype(np.float32)
        if s_xg is not None:
            t = (t * s_xg[:, gi:gi + 1]).astype(np.float32)
        f = (f + (t * s_wg[gi][None, :]).astype(np.float32)).astype(np.float32)
    sx = np.full(M, sx0, np.float32)
    if row_sel is not None:
        sx = np.where(row_sel != 0, np.float32(sx0 if sx1 is None else sx1), np.float32(sx0)).astype(np.float32)
    if sx_rows is not None:
        sx = sx_rows.astype(np.float32)
    if s_xg is None:
        f = (f * sx[:, None]).astype(np.float32)
    return (f if bias is None else (f + bias[None, :]).astype(np.float32)), acc


def expected(w_bits, a, stored, d, s_wg, g, **kw):
    """int4: the oracle over the levels q - z = stored + d (values in -15 .. 15); int8: the numpy restatement."""
    if w_bits == 4:
        qmz = (stored.astype(np.int32) + np.repeat(d.T.astype(np.int32), g, axis=1)).astype(np.int8)
        return oracle.gemm_wgroup(a, qmz, s_wg, g, **kw)
    return restate(a, stored, d, s_wg, g, **kw)[0]


def problem(rng, w_bits, M, N, K, g):
    K_pad = (K + 127) // 128 * 128
    G, half = K // g, 1 << (w_bits - 1)
    a = np.zeros((M, K_pad), np.int8)
    a[:, :K] = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    stored = rng.integers(-half, half, size=(N, K), dtype=np.int8)
    wp = np.zeros((N, K_pad), np.int8)
    wp[:, :K] = stored
    d = (half - rng.integers(0, 2 * half, size=(G, N))).astype(np.int16)
    s_wg = (rng.random((G, N), dtype=np.float32) * 0.01 + 0.001).astype(np.float32)
    bias = rng.normal(size=N).astype(np.float32)
    return K_pad, G, a, stored, wp, d, s_wg, bias


def scale_case(rng, act, M, G):
    if act == "static":
        return dict(s_x0=0.031), dict(sx0=0.031)
    if act == "msq":
        sel = (rng.random(M) < 0.4).astype(np.uint8)
        return dict(s_x0=0.031, s_x1=0.0077, row_sel=to_dev(sel)), dict(sx0=0.031, sx1=0.0077, row_sel=sel)
    if act == "rows":
        rows = (rng.random(M, dtype=np.float32) * 0.05 + 0.01).astype(np.float32)
        return dict(s_x_rows=to_dev(rows)), dict(sx_rows=rows)
    s_xg = (rng.random((M, G), dtype=np.float32) * 0.2 + 0.01).astype(np.float32)
    return dict(s_x_groups=to_dev(s_xg)), dict(s_xg=s_xg)


def run_asym(ops, at, img, w_bits, N, s_wg, d, g, G, **kw):
    sums = ops.act_group_rowsum(at, g, G)
    return ops.gemm_w4a8_wgroupscale_asym(at, img, w_bits, N, to_dev(s_wg), to_dev(d), sums, g, **kw)


def test_kernel_equals_the_restatement():
    """Ragged M and N, K_pad > K with the clamped tail group (K = 192, g = 64), groups of 64 .. 512, every s_x case, both layouts,
    fp16 / bf16 / fp32 outputs, int4 and int8."""
    sweep(_kernel_case, [(4, torch.float16), (4, torch.bfloat16), (4, torch.float32), (8, torch.float16), (8, torch.float32)], SHAPES,
          ["static", "msq", "rows", "groups"])


def _kernel_case(bits_dtype, shape, act):
    from mquant_amd import ops
    (w_bits, out_dtype), (M, N, K, g) = bits_dtype, shape
    rng = np.random.default_rng(M + N + K + g + w_bits)
    K_pad, G, a, stored, wp, d, s_wg, bias = problem(rng, w_bits, M, N, K, g)
    kw, okw = scale_case(rng, act, M, G)
    want = oracle.round_to(expected(w_bits, a[:, :K], stored, d, s_wg, g, bias=bias, **okw), MODE[out_dtype])
    img = ops.prepack(to_dev(wp), w_bits)
    for at in (ops.TiledAct.from_rows(to_dev(a)), to_dev(a)):
        y = run_asym(ops, at, img, w_bits, N, s_wg, d, g, G, bias=to_dev(bias), out_dtype=out_dtype, **kw)
        np.testing.assert_array_equal(y.float().cpu().numpy(), want)


def test_numpy_restatement_equals_the_oracle_on_int4():
    """The int8 cases rest on ``restate``: on int4, where both exist, it gives the oracle's bits."""
    rng = np.random.default_rng(11)
    M, N, K, g = 19, 40, 512, 128
    _, G, a, stored, _, d, s_wg, bias = problem(rng, 4, M, N, K, g)
    for act in ("static", "msq", "rows", "groups"):
        _, okw = scale_case(rng, act, M, G)
        okw = {k: v for k, v in okw.items()}
        np.testing.assert_array_equal(restate(a, stored, d, s_wg, g, bias=bias, **okw)[0], expected(4, a, stored, d, s_wg, g, bias=bias, **okw))


def test_a_forced_tile_does_not_change_the_bits():
    """The round-1 kernel (tile 26) serves this mode; the fold tiles of the symmetric call (45 .. 48) do not and a forced one is
    ignored, as the symmetric call ignores a forced tile outside its set: the same bits either way."""
    sweep(_forced_tile_case, [45, 46, 47, 48, 26], [(4, torch.float16), (8, torch.bfloat16)],
          [(300, 264, 1920, 64), (33, 72, 192, 64), (130, 260, 1024, 256)])


def _forced_tile_case(tile, bits_dtype, shape):
    from mquant_amd import ops
    (w_bits, out_dtype), (M, N, K, g) = bits_dtype, shape
    rng = np.random.default_rng(M + N + K + g + w_bits + 1)
    K_pad, G, a, stored, wp, d, s_wg, bias = problem(rng, w_bits, M, N, K, g)
    s_xg = (rng.random((M, G), dtype=np.float32) * 0.2 + 0.01).astype(np.float32)
    img = ops.prepack(to_dev(wp), w_bits)
    at = ops.TiledAct.from_rows(to_dev(a))
    try:
        ops.gemm_debug_force(tile, 0)
        y0 = run_asym(ops, at, img, w_bits, N, s_wg, d, g, G, bias=to_dev(bias), out_dtype=out_dtype, s_x0=0.031)
        y1 = run_asym(ops, at, img, w_bits, N, s_wg, d, g, G, bias=to_dev(bias), out_dtype=out_dtype, s_x_groups=to_dev(s_xg))
    finally:
        ops.gemm_debug_force(-1, 0)
    np.testing.assert_array_equal(y0.float().cpu().numpy(), oracle.round_to(expected(w_bits, a[:, :K], stored, d, s_wg, g, bias=bias, sx0=0.031), MODE[out_dtype]))
    np.testing.assert_array_equal(y1.float().cpu().numpy(), oracle.round_to(expected(w_bits, a[:, :K], stored, d, s_wg, g, bias=bias, s_xg=s_xg), MODE[out_dtype]))


def test_extreme_levels_keep_every_bit():
    sweep(_extreme_case, [4, 8], [128, 256])


def _extreme_case(w_bits, g):
    """Rows of constant -128 and +127 against stored levels -2^(b-1) with z = 2^b - 1 and 2^(b-1) - 1 with z = 0: every product of a
    group has the same sign and |acc'_g| reaches g * 128 * (2^b - 1) -- past the 2^18 / 2^22 up to which an accumulator can be read
    out of a magic-number bias without a conversion at g = 256."""
    from mquant_amd import ops
    half, M, N, G = 1 << (w_bits - 1), 35, 72, 3
    K = G * g
    K_pad = (K + 127) // 128 * 128
    a = np.zeros((M, K_pad), np.int8)
    a[0::2, :K], a[1::2, :K] = -128, 127
    stored = np.zeros((N, K_pad), np.int8)
    stored[0::2, :K], stored[1::2, :K] = -half, half - 1
    d = np.zeros((G, N), np.int16)
    d[:, 0::2], d[:, 1::2] = half - (2 * half - 1), half
    rng = np.random.default_rng(g + w_bits)
    s_wg = (rng.random((G, N), dtype=np.float32) * 0.01 + 0.001).astype(np.float32)
    acc = restate(a[:, :K], stored[:, :K], d, s_wg, g)[1]
    assert int(np.abs(acc).max()) == g * 128 * (2 * half - 1)
    want = expected(w_bits, a[:, :K], stored[:, :K], d, s_wg, g, sx0=0.0123)
    img = ops.prepack(to_dev(stored), w_bits)
    for at in (ops.TiledAct.from_rows(to_dev(a)), to_dev(a)):
        y = run_asym(ops, at, img, w_bits, N, s_wg, d, g, G, out_dtype=torch.float32, s_x0=0.0123)
        np.testing.assert_array_equal(y.cpu().numpy(), want)


def test_act_group_rowsum_equals_numpy_and_stays_inside_its_buffer():
    sweep(_rowsum_case, [(37, 192, 64, 1), (37, 1280, 128, 0), (130, 2048, 64, 0), (5, 3072, 1024, 0), (21, 1536, 384, 0), (18, 4096, 2048, 0)])


def _rowsum_case(shape):
    """Ragged M, K_pad > K (``extra``: one more group, inside the zero padding -- sums to 0), power-of-two groups and the general
    walk (384, 2048), both layouts; the int32 words around the [M, n_groups] result keep their sentinel."""
    from mquant_amd import ops
    M, K, g, extra = shape
    rng = np.random.default_rng(M + K + g)
    K_pad = (K + 127) // 128 * 128
    G = K // g + extra
    a = np.zeros((M, K_pad), np.int8)
    a[:, :K] = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    want = np.zeros((M, G), np.int32)
    want[:, :K // g] = a[:, :K].astype(np.int32).reshape(M, K // g, g).sum(axis=2)
    for at in (ops.TiledAct.from_rows(to_dev(a)), to_dev(a)):
        buf = torch.full((M * G + 64,), -77, dtype=torch.int32, device=DEV)
        out = buf[32:32 + M * G].view(M, G)
        ops.act_group_rowsum(at, g, G, out=out)
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        assert bool((buf[:32] == -77).all()) and bool((buf[32 + M * G:] == -77).all())


def test_gemm_writes_its_output_columns_only():
    sweep(_sentinel_case, [torch.float16, torch.float32])


def _sentinel_case(out_dtype):
    """Ragged M and N inside a wider buffer: the clamped rows and channels a tile reads leak into no stored element."""
    from mquant_amd import ops
    rng = np.random.default_rng(5)
    M, N, K, g, ldo = 37, 200, 1280, 128, 216
    K_pad, G, a, stored, wp, d, s_wg, bias = problem(rng, 4, M, N, K, g)
    want = oracle.round_to(expected(4, a[:, :K], stored, d, s_wg, g, bias=bias, sx0=0.031), MODE[out_dtype])
    buf = torch.full((M + 2, ldo), 777.0, dtype=out_dtype, device=DEV)
    out = buf[1:M + 1, 8:8 + N]
    img = ops.prepack(to_dev(wp), 4)
    run_asym(ops, ops.TiledAct.from_rows(to_dev(a)), img, 4, N, s_wg, d, g, G, bias=to_dev(bias), s_x0=0.031, out=out)
    np.testing.assert_array_equal(out.float().cpu().numpy(), want)
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[1:M + 1, 8:8 + N] = False
    assert bool((buf[keep] == 777.0).all())


def test_entry_points_refuse_what_they_cannot_do():
    from mquant_amd import ops
    from mquant_amd._lib import MQuantHipError, call
    a = torch.zeros((16, 256), dtype=torch.int8, device=DEV)
    img = ops.prepack(torch.zeros((32, 256), dtype=torch.int8, device=DEV), 4)
    s_wg, d, r = torch.ones((2, 32), device=DEV), torch.zeros((2, 32), dtype=torch.int16, device=DEV), torch.zeros((16, 2), dtype=torch.int32, device=DEV)
    out = torch.empty((16, 32), dtype=torch.float16, device=DEV)

    def raw(zp, sums, **kw):
        call("mq_gemm_w4a8_wgroupscale_asym", a.data_ptr(), 256, img.data_ptr(), kw.get("bits", 4), 16, 32, 256, s_wg.data_ptr(), zp, sums,
             kw.get("G", 2), kw.get("g", 128), 1.0, 1.0, None, kw.get("rows"), kw.get("groups"), None, out.data_ptr(), 0, 32, None)
    with pytest.raises(MQuantHipError, match="w_zero_offsets and a_group_sums are required"):
        raw(None, r.data_ptr())
    with pytest.raises(MQuantHipError, match="w_zero_offsets and a_group_sums are required"):
        raw(d.data_ptr(), None)
    with pytest.raises(MQuantHipError, match="do not cover"):                  # groups that do not cover K
        raw(d.data_ptr(), r.data_ptr(), G=1, g=64)
    with pytest.raises(MQuantHipError, match="group size"):
        raw(d.data_ptr(), r.data_ptr(), G=8, g=32)
    with pytest.raises(MQuantHipError, match="exclude per-row"):
        raw(d.data_ptr(), r.data_ptr(), rows=torch.ones(16, device=DEV).data_ptr(), groups=torch.ones((16, 2), device=DEV).data_ptr())
    a8 = torch.zeros((16, 1024), dtype=torch.int8, device=DEV)
    img8 = ops.prepack(torch.zeros((32, 1024), dtype=torch.int8, device=DEV), 8)
    with pytest.raises(MQuantHipError, match="int8 weight groups of 1024"):
        ops.gemm_w4a8_wgroupscale_asym(a8, img8, 8, 32, torch.ones((1, 32), device=DEV), d[:1].contiguous(), r[:, :1].contiguous(), 1024)
    with pytest.raises(MQuantHipError, match="exceed K_pad"):
        ops.act_group_rowsum(a, 128, 3)
    with pytest.raises(MQuantHipError, match="group size"):
        ops.act_group_rowsum(a, 32, 8)
    assert ops.gemm_w4a8_wgroupscale_asym(a, img, 4, 32, s_wg, d, ops.act_group_rowsum(a, 128, 2), 128).shape == (16, 32)


class Args:
    skip_names = []


def _configure_acts(wrap, g, c, dt):
    from fake_quant import quant_utils as qu
    if c["mode"] == "static":
        wrap.quantizer.configure(bits=8, sym=True, static=True, observer_type="minmax")
        qu.calib_layer(wrap, [torch.from_numpy(make_x(c["seed"] + 10 + i, (c["M"], c["K_in"]))).to(dt).to(DEV) for i in range(3)], Args())
    elif c["mode"] == "dyn":
        wrap.quantizer.configure(bits=8, sym=True)
    else:
        wrap.quantizer.configure(bits=8, groupsize=c["g"], sym=True, clip_ratio=1.0)


def test_wrapper_over_the_references_asymmetric_gptq_weights_matches_the_references_forward(golden_dir):
    from mquant_amd import ops
    paths = cases(golden_dir)
    assert len(paths) == 6
    for path in paths:
        g, c = load(path)
        dt = DT[c["dtc"]]
        qmz, stored, d = parts_of(g, c)
        wrap = wrapper_from_golden(g, c, DEV)
        _configure_acts(wrap, g, c, dt)
        if c["mode"] == "static":
            np.testing.assert_array_equal(np.asarray(wrap.quantizer.quantizer.scale.cpu().numpy(), np.float32), g["s_x"], err_msg=path)
        shape = (1, c["M"], c["K_in"]) if c["mode"] == "agrp" else (c["M"], c["K_in"])
        x = torch.from_numpy(make_x(c["seed"] + 20, shape)).to(dt).to(DEV)
        assert wrap._real_ready(x), (path, wrap.backend())
        assert wrap.backend().startswith("W4A8 integer") and wrap.backend().endswith("weight groups of %d, asymmetric)" % c["g"]), wrap.backend()
        y = wrap(x)
        real = wrap._real
        assert real is not None and real.w_groups is not None and real.w_groups[1] == c["g"] and real.w_group_offsets is not None
        tol = TOL[c["dtc"]] * float(np.abs(g["y"]).max())
        np.testing.assert_allclose(y.float().cpu().numpy().reshape(c["M"], c["N"]), g["y"], rtol=0, atol=tol, err_msg=path)
        # the stored levels, scales and zero offsets the engine froze are the reference's, group by group
        assert torch.equal(real.w_img, ops.prepack(to_dev(stored), c["w_bits"])), path
        np.testing.assert_array_equal(real.w_groups[0].cpu().numpy(), g["group_scales"].T, err_msg=path)
        np.testing.assert_array_equal(real.w_group_offsets.cpu().numpy(), d, err_msg=path)
        # ... and the activation levels / scales equal the reference's own quantizer's
        rows = x.reshape(c["M"], c["K_in"])
        xr = ops.hadamard(rows, real.had.n, real.had.K, real.had.bits) if c["had"] else rows
        if "perm" in g:
            assert real.col_perm is not None and torch.equal(real.col_perm.cpu(), torch.from_numpy(g["perm"]))
            xr = xr.index_select(1, real.col_perm)
        if c["mode"] == "static":
            a, _ = real.quantize(rows)
            qx = a.to_rows() if isinstance(a, ops.TiledAct) else a
        elif c["mode"] == "dyn":
            qx, s_rows, _ = ops.quantize_act_dyn_i8(xr, 8, 1.0)
            np.testing.assert_array_equal(s_rows.cpu().numpy(), g["s_x_rows"], err_msg=path)
        else:
            qx, s_g = ops.quantize_act_group_i8(xr, c["g"], 8, 1.0)
            np.testing.assert_array_equal(s_g.cpu().numpy(), g["s_x_groups"], err_msg=path)
        np.testing.assert_array_equal(qx[:, :c["K_pad"]].cpu().numpy(), g["qx"], err_msg=path)
        bias = None if not c["bias"] else wrap.module.bias.data.float().cpu().numpy()
        want = oracle.gemm_wgroup(g["qx"], qmz, g["group_scales"].T.copy(), c["g"], bias=bias, **act_scales(g, c))
        # the wrapper's output IS the oracle's evaluation of the reference's integers q - z, bit for bit
        np.testing.assert_array_equal(y.float().cpu().numpy().reshape(c["M"], c["N"]), oracle.round_to(want, c["dtc"]), err_msg=path)


def test_asymmetric_groups_run_end_to_end_through_the_solvers():
    sweep(_solver_case, ["gptq", "gptq_actorder", "rtn"])


def _solver_case(solver_kind):
    """This repository's GPTQ (with and without --act_order) and its group-wise RTN with sym = False -> attach -> static calibration ->
    the wrapper runs the integer kernels and stays on the simulated evaluation of the same wrapper."""
    from fake_quant import quant_utils as qu
    from fake_quant.gptq.gptq_utils import GPTQ
    from fake_quant.gptq.rtn import rtn_module
    K, N, M = 1024, 96, 64
    root = torch.nn.Module()
    root.lin = torch.nn.Linear(K, N, bias=True)
    root.lin.weight.data = torch.from_numpy(make_w(5, (N, K))) * 4.0 + torch.from_numpy(make_w(7, (N, 1))) * 2.0
    root = root.to(DEV)
    qu.add_actquant(root)
    wrap = root.lin
    if solver_kind == "rtn":
        rtn_module(root, "m", 4, False, False, [], {}, groupsize=128)
    else:
        solver = GPTQ(wrap.module)
        solver.quantizer = qu.WeightQuantizer()
        solver.quantizer.configure(4, perchannel=True, sym=False, mse=False)
        for i in range(3):
            solver.add_batch(torch.from_numpy(make_x(50 + i, (1, 80, K))).to(DEV))
        solver.fasterquant(percdamp=0.01, groupsize=128, actorder=solver_kind == "gptq_actorder", static_groups=False)
        qu.attach_weight_quantizer(wrap, "module", solver.quantizer)
    wq = wrap.weight_quantizers["module"]
    assert not wq.sym and tuple(wq.group_zeros.shape) == (N, K // 128) and len(torch.unique(wq.group_zeros)) > 3
    wrap.quantizer.configure(bits=8, sym=True, static=True, observer_type="minmax")
    qu.calib_layer(wrap, [torch.from_numpy(make_x(60 + i, (M, K))).to(DEV) for i in range(2)], Args())
    x = torch.from_numpy(make_x(70, (M, K))).to(DEV)
    assert wrap._real_ready(x) and wrap.backend() == "W4A8 integer (static, weight groups of 128, asymmetric)", wrap.backend()
    y = wrap(x)
    assert wrap._real.w_group_offsets is not None and (wrap._real.col_perm is not None) == (solver_kind == "gptq_actorder")
    wrap.real_quant = False
    y_sim = wrap(x.clone())
    np.testing.assert_allclose(y.cpu().numpy(), y_sim.cpu().numpy(), rtol=0, atol=1e-3 * float(y_sim.abs().max()))


def test_sibling_fusion_with_asymmetric_groups_equals_the_per_linear_evaluation():
    """q / k / v wrappers with asymmetric weight groups of one size fuse into ONE quantize + ONE group-sum launch + ONE grouped GEMM
    (scale and zero-offset tables side by side): bit-identical to evaluating every Linear on its own."""
    from fake_quant import quant_utils as qu
    from fake_quant.gptq.rtn import rtn_module

    class Attn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj = torch.nn.Linear(512, 256, bias=True)
            self.k_proj = torch.nn.Linear(512, 64, bias=True)
            self.v_proj = torch.nn.Linear(512, 64, bias=True)

        def forward(self, x):
            return self.q_proj(x), self.k_proj(x), self.v_proj(x)

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.attn = Attn()

        def forward(self, x):
            return self.attn(x)

    torch.manual_seed(3)
    model = Holder().to(DEV)
    for lin in (model.attn.q_proj, model.attn.k_proj, model.attn.v_proj):
        lin.weight.data += 0.02
    qu.add_actquant(model)
    rtn_module(model, "m", 4, False, False, [], {}, groupsize=128)
    for name in ("q_proj", "k_proj", "v_proj"):
        getattr(model.attn, name).quantizer.configure(bits=8, sym=True, static=True, observer_type="minmax")
    qu.calib_layer(model, [torch.from_numpy(make_x(40 + i, (24, 512))).to(DEV) for i in range(2)], Args())
    x = torch.from_numpy(make_x(50, (24, 512))).to(DEV)
    fused = [t.clone() for t in model(x)]
    grp = model.attn.q_proj.__dict__.get("_group")
    assert grp is not None and grp.enabled and grp.engine is not None and grp.launches == 1
    assert tuple(grp.engine.w_groups[0].shape) == (4, 384) and tuple(grp.engine.w_group_offsets.shape) == (4, 384)
    offs = grp.engine.w_group_offsets.clone()
    qu.model_quant(model, types.SimpleNamespace(skip_names=[], no_sibling_fusion=True))
    plain = model(x)
    assert all(torch.equal(a, b) for a, b in zip(fused, plain))
    assert model.attn.k_proj._real is not None and torch.equal(offs[:, 256:320], model.attn.k_proj._real.w_group_offsets)


def test_asymmetric_groups_round_trip_through_the_flat_checkpoint(golden_dir, tmp_path):
    """The record gains ``w_group_zero_offsets`` (int16 [K / g, N]); the rebuilt engine gives the wrapper's bits, through a file too."""
    import os
    from safetensors.torch import load_file, save_file
    from mquant_amd import checkpoint
    for tag in ("g128_static_had_1280_f16", "ao_g128_static_1024_f32", "g128_agrp_1024_f32"):
        g, c = load(os.path.join(golden_dir, "wrapper_wgasym_%s.npz" % tag))
        dt = DT[c["dtc"]]
        wrap = wrapper_from_golden(g, c, DEV)
        _configure_acts(wrap, g, c, dt)
        x = torch.from_numpy(make_x(c["seed"] + 20, (c["M"], c["K_in"]))).to(dt).to(DEV)
        y = wrap(x.reshape(1, c["M"], c["K_in"]) if c["mode"] == "agrp" else x).reshape(c["M"], c["N"])
        rec = checkpoint.export_wrapper(wrap)
        offs = rec["w_group_zero_offsets"]
        assert offs.dtype == torch.int16 and tuple(offs.shape) == (c["K_pad"] // c["g"], c["N"]) and "w_shift" not in rec
        np.testing.assert_array_equal(offs.numpy(), parts_of(g, c)[2])
        path = str(tmp_path / (tag + ".safetensors"))
        save_file(rec, path)
        back = load_file(path)
        assert all(torch.equal(back[k], rec[k]) for k in rec) and set(back) == set(rec)
        eng = checkpoint.build_linear(back, torch.device(DEV))
        assert torch.equal(eng.forward(x), y), tag
        # a record without the offsets loads as before: symmetric groups
        del back["w_group_zero_offsets"]
        assert checkpoint.build_linear(back, torch.device(DEV)).w_group_offsets is None
