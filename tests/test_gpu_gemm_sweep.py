"""Every W4A8 GEMM entry point at the DEFAULT plan over the seeded cases of gemm_cases.py, which sit on both sides of each point where
the plan switches kernels (test_gemm_sweep_plan_cpu.py pins which kernels they reach).  Per case:

 * ``gemm_w4a8_i32`` equal to ``oracle.gemm_i32``; ``gemm_w4a8`` (two static scales, row_sel, bias), ``gemm_w4a8_rowscale`` (+ x0 / w0)
   and ``gemm_w4a8_rank2`` (static and per-row scales) equal bit for bit to ``oracle.epilogue`` + ``oracle.round_to``, three output
   dtypes; ``gemm_w4a8_residual`` out of place and in place equal to torch's add on the rounded GEMM output; ``gemm_w4a8_act`` equal to
   the GEMM + the torch ops (test_gpu_act_gemm.py's bar); ``gemm_w4a8_rope`` equal to the GEMM + ``rope_inplace``; the group-scale
   entry points equal to their restated arithmetic (test_gpu_wgroup.py / test_gpu_groupwise.py);
 * placement: parameters as views at a 4-byte offset into larger tensors, outputs and residuals as column slices of sentinel-filled
   buffers (ldo, ldr > N; at an odd column, or aligned with a wider row): the same bits as the call on fresh tensors, the sentinel
   untouched -- or MQuantHipError where a host check refuses the placement;
 * workspace: no workspace, and one smaller than the planned split: the same bits.
LARGE cases are held to the oracle on sampled columns plus exact row and column checksums of the int32 product."""
import numpy as np
import pytest
import torch

import gemm_cases as gc
import oracle
from test_gpu_act_gemm import _torch_act

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DTYPES = (torch.float16, torch.bfloat16, torch.float32)
MODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
SX0, SX1 = 0.0213, 0.0077
SENTINEL = -1234.0


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def offset_view(t):
    """The same values as a view 4 bytes into a larger tensor (a slice of a fused parameter tensor)."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def placed(M, N, dtype, how):
    """A [M, N] column slice of a sentinel-filled buffer: ``odd`` -- at column 1 of rows N + 9 wide (no 16-byte alignment anywhere),
    ``wide`` -- at column 0 of rows padded to a multiple of 8 plus 8 (aligned, ld > N)."""
    ld, c0 = (N + 9, 1) if how == "odd" else ((N + 7) // 8 * 8 + 8, 0)
    buf = torch.full((M, ld), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:, c0:c0 + N], c0


def sentinel_kept(buf, c0, N):
    chk = buf.clone()
    chk[:, c0:c0 + N] = SENTINEL
    return torch.equal(chk, torch.full_like(buf, SENTINEL))


class Sweep:
    def __init__(self, c, o):
        self.c, self.o = c, o
        d = gc.operands(c)
        self.d = d
        self.cols = gc.columns(c, d["rng"])
        self.a_rows = dev(d["a"])
        self.a = o.TiledAct.from_rows(self.a_rows) if c.a_tiled else self.a_rows
        self.w_dev = dev(d["w"])
        self.img = o.prepack(self.w_dev, c.w_bits)
        self.t = {k: dev(d[k]) for k in ("s_w", "bias", "w0", "w1", "x0", "x1", "rows", "sel")}
        self.acc_ref = oracle.gemm_i32(d["a"], d["w"][self.cols])

    def col(self, k):
        return self.d[k][self.cols]

    def assert_oracle(self, y, want, what):
        np.testing.assert_array_equal(y[:, torch.from_numpy(self.cols).to(DEV)].float().cpu().numpy(), want, err_msg=f"{self.c.name}: {what}")

    def assert_acc(self, acc):
        c = self.c
        np.testing.assert_array_equal(acc[:, torch.from_numpy(self.cols).to(DEV)].cpu().numpy(), self.acc_ref, err_msg=f"{c.name}: int32")
        if gc.large(c):        # every column: row and column sums of the product from the factors' sums (exact integers)
            a64 = self.a_rows.to(torch.int64)
            acc64 = acc.to(torch.int64)
            assert torch.equal(acc64.sum(1), (a64 * self.w_dev.sum(0, dtype=torch.int64)[None, :]).sum(1)), c.name
            asum = a64.sum(0)
            colsum = torch.cat([(self.w_dev[n0:n0 + 2048].to(torch.int64) * asum[None, :]).sum(1) for n0 in range(0, c.N, 2048)])
            assert torch.equal(acc64.sum(0), colsum), c.name

    # the entry points, with the operands of this case (parameter tensors overridable for the placement variant)
    def plain(self, dt, p=None, out=None):
        p = p or self.t
        return self.o.gemm_w4a8(self.a, self.img, self.c.w_bits, self.c.N, SX0, p["s_w"], s_x1=SX1, row_sel=self.t["sel"], bias=p["bias"],
                                out_dtype=dt, out=out)

    def rowscale(self, dt, p=None, out=None):
        p = p or self.t
        return self.o.gemm_w4a8_rowscale(self.a, self.img, self.c.w_bits, self.c.N, self.t["rows"], p["s_w"], bias=p["bias"],
                                         x0=self.t["x0"], w0=p["w0"], out_dtype=dt, out=out)

    def rank2(self, dt, rows, p=None, out=None):
        p = p or self.t
        kw = dict(s_x_rows=self.t["rows"]) if rows else dict(s_x0=SX0, s_x1=SX1, row_sel=self.t["sel"])
        return self.o.gemm_w4a8_rank2(self.a, self.img, self.c.w_bits, self.c.N, p["s_w"], self.t["x0"], p["w0"], self.t["x1"], p["w1"],
                                      bias=p["bias"], out_dtype=dt, out=out, **kw)

    def residual(self, res, p=None, out=None):
        p = p or self.t
        return self.o.gemm_w4a8_residual(self.a, self.img, self.c.w_bits, self.c.N, SX0, p["s_w"], res, s_x1=SX1, row_sel=self.t["sel"],
                                         bias=p["bias"], out=out)

    def act(self, dt, act, p=None, out=None):
        p = p or self.t
        return self.o.gemm_w4a8_act(self.a, self.img, self.c.w_bits, self.c.N, SX0, p["s_w"], act, s_x1=SX1, row_sel=self.t["sel"],
                                    bias=p["bias"], out_dtype=dt, out=out)

    def rope(self, dt, cos, sin, cols, p=None, out=None):
        p = p or self.t
        return self.o.gemm_w4a8_rope(self.a, self.img, self.c.w_bits, self.c.N, SX0, p["s_w"], cos, sin, cols, s_x1=SX1,
                                     row_sel=self.t["sel"], bias=p["bias"], out_dtype=dt, out=out)

    def i32_into(self, out, ws=None):
        o = self.o
        aptr, lda, M, K_pad = o._a_args(self.a)
        o.call("mq_gemm_w4a8_i32_ws", aptr, lda, self.img.data_ptr(), self.c.w_bits, M, self.c.N, K_pad, out.data_ptr(), out.stride(0),
               None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), o._stream())
        return out


def rope_tables(T, dtype):
    inv = 1.0 / (1e6 ** (torch.arange(0, 128, 2, device=DEV, dtype=torch.float32) / 128))
    ang = torch.arange(T, device=DEV, dtype=torch.float32)[:, None] * inv[None, :]
    ang = torch.cat([ang, ang], dim=-1)
    return ang.cos().to(dtype).contiguous(), ang.sin().to(dtype).contiguous()


def acts(c, o):
    """The activations the host check accepts for the case: tiled activations, silu(gate) * up on 2 x (a multiple of 32) channels,
    QuickGELU on a multiple of 8."""
    if not c.a_tiled:
        return ()
    return tuple(a for a, ok in ((o.ACT_SILU_MUL, c.N % 64 == 0), (o.ACT_QUICK_GELU, c.N % 8 == 0)) if ok)


def rope_cols(c):
    return min(c.N // 128, 4) * 128 if c.a_tiled and c.N % 8 == 0 else 0


@pytest.mark.parametrize("idx", range(len(gc.CASES)), ids=[c.name for c in gc.CASES])
def test_entry_points_at_the_default_plan(idx, monkeypatch):
    from mquant_amd import ops as o
    from mquant_amd._lib import MQuantHipError
    c = gc.CASES[idx]
    o.gemm_debug_force(-1, 0)                                        # the default plan (a test before may have forced a tile)
    try:
        o.splitk_workspace(torch.device(DEV), 64 << 20)
        s = Sweep(c, o)
        M, N = c.M, c.N
        s.assert_acc(o.gemm_w4a8_i32(s.a, s.img, c.w_bits, N))

        # ---- oracle: every floating-point entry point, three output dtypes --------------------------------------------------
        e_plain = oracle.epilogue(s.acc_ref, np.float32(SX0), s.col("s_w"), bias=s.col("bias"), sx1=np.float32(SX1), row_sel=s.d["sel"])
        e_rows = oracle.epilogue(s.acc_ref, s.d["rows"], s.col("s_w"), bias=s.col("bias"), x0=s.d["x0"], w0=s.col("w0"))
        e_r2 = oracle.epilogue(s.acc_ref, np.float32(SX0), s.col("s_w"), bias=s.col("bias"), sx1=np.float32(SX1), row_sel=s.d["sel"],
                               x0=s.d["x0"], w0=s.col("w0"), x1=s.d["x1"], w1=s.col("w1"))
        e_r2rows = oracle.epilogue(s.acc_ref, s.d["rows"], s.col("s_w"), bias=s.col("bias"), x0=s.d["x0"], w0=s.col("w0"),
                                   x1=s.d["x1"], w1=s.col("w1"))
        res = dev(s.d["res"])
        got = {}
        for dt in DTYPES:
            md = MODE[dt]
            y = s.plain(dt)
            s.assert_oracle(y, oracle.round_to(e_plain, md), f"gemm_w4a8 {dt}")
            got[("plain", dt)] = y
            got[("rows", dt)] = s.rowscale(dt)
            s.assert_oracle(got[("rows", dt)], oracle.round_to(e_rows, md), f"gemm_w4a8_rowscale {dt}")
            got[("r2", dt)] = s.rank2(dt, rows=False)
            s.assert_oracle(got[("r2", dt)], oracle.round_to(e_r2, md), f"gemm_w4a8_rank2 {dt}")
            got[("r2rows", dt)] = s.rank2(dt, rows=True)
            s.assert_oracle(got[("r2rows", dt)], oracle.round_to(e_r2rows, md), f"gemm_w4a8_rank2 per-row {dt}")
            r = res.to(dt)
            want = r + y                                             # torch: hidden + linear(x), the Linear's output rounded first
            got[("res", dt)] = want
            assert torch.equal(s.residual(r), want), f"{c.name}: residual {dt}"
            inplace = r.clone()
            s.residual(inplace, out=inplace)
            assert torch.equal(inplace, want), f"{c.name}: residual in place {dt}"
            for act in acts(c, o):
                a_out = s.act(dt, act)
                assert torch.equal(a_out, _torch_act(y, act, o)), f"{c.name}: act {act} {dt}"
                got[("act", act, dt)] = a_out
            rc = rope_cols(c)
            if rc and dt != torch.float32:
                cos, sin = rope_tables(M, dt)
                want = y.clone()
                o.rope_inplace(want[:, :rc], rc // 128, 128, cos, sin)
                assert torch.equal(s.rope(dt, cos, sin, rc), want), f"{c.name}: rope {dt}"
                got[("rope", dt)] = (want, cos, sin, rc)

        # ---- the group-scale entry points (their own kernels; the restated arithmetic) ------------------------------------
        g = 64 if (c.K_pad // 128) % 2 else 128
        G = c.K_pad // g
        rng = np.random.default_rng(idx)
        s_wg = (rng.random((G, N), dtype=np.float32) * 0.01 + 0.001).astype(np.float32)
        s_xg = (rng.random((M, G), dtype=np.float32) * 0.2 + 0.01).astype(np.float32)
        if not gc.large(c):
            e_wg = oracle.gemm_wgroup(s.d["a"], s.d["w"], s_wg, g, sx0=SX0, sx1=SX1, row_sel=s.d["sel"], bias=s.d["bias"])
            f = np.zeros((M, N), np.float32)
            for gi in range(G):                                      # ascending groups, one fp32 rounding per operation
                acc_g = oracle.gemm_i32(s.d["a"][:, gi * g:(gi + 1) * g], s.d["w"][:, gi * g:(gi + 1) * g])
                f = (f + (acc_g.astype(np.float32) * s_xg[:, gi:gi + 1]).astype(np.float32)).astype(np.float32)
            e_g = ((f * s.d["s_w"][None, :]).astype(np.float32) + s.d["bias"][None, :]).astype(np.float32)
            s_wg_t, s_xg_t = dev(s_wg), dev(s_xg)
            for dt in DTYPES:
                y = o.gemm_w4a8_wgroupscale(s.a, s.img, c.w_bits, N, s_wg_t, g, s_x0=SX0, s_x1=SX1, row_sel=s.t["sel"], bias=s.t["bias"],
                                            out_dtype=dt)
                np.testing.assert_array_equal(y.float().cpu().numpy(), oracle.round_to(e_wg, MODE[dt]), err_msg=f"{c.name}: wgroupscale {dt}")
                got[("wg", dt)] = y
                y = o.gemm_w4a8_groupscale(s.a, s.img, c.w_bits, N, s_xg_t, g, s.t["s_w"], bias=s.t["bias"], out_dtype=dt)
                np.testing.assert_array_equal(y.float().cpu().numpy(), oracle.round_to(e_g, MODE[dt]), err_msg=f"{c.name}: groupscale {dt}")
                got[("g", dt)] = y

        # ---- placement: offset parameter views, strided / unaligned outputs and residuals ---------------------------------
        dv = DTYPES[idx % 3]
        views = {k: offset_view(s.t[k]) for k in ("s_w", "bias", "w0", "w1")}
        for how in ("odd", "wide"):
            p = views if how == "odd" else None
            tag = f"{c.name}: placement {how} {dv}"
            for name, fn in (("plain", lambda out: s.plain(dv, p, out)), ("rows", lambda out: s.rowscale(dv, p, out)),
                             ("r2", lambda out: s.rank2(dv, False, p, out)), ("r2rows", lambda out: s.rank2(dv, True, p, out))):
                buf, out, c0 = placed(M, N, dv, how)
                fn(out)
                assert torch.equal(out, got[(name, dv)]) and sentinel_kept(buf, c0, N), f"{tag}: {name}"
            rbuf, rv, rc0 = placed(M, N, dv, how)
            rv.copy_(res.to(dv))
            buf, out, c0 = placed(M, N, dv, how)
            s.residual(rv, p, out)
            assert torch.equal(out, got[("res", dv)]) and sentinel_kept(buf, c0, N) and sentinel_kept(rbuf, rc0, N), f"{tag}: residual"
            s.residual(rv, p, rv)
            assert torch.equal(rv, got[("res", dv)]) and sentinel_kept(rbuf, rc0, N), f"{tag}: residual in place"
            ibuf = torch.full((M, N + 9 if how == "odd" else (N + 7) // 8 * 8 + 8), -7, dtype=torch.int32, device=DEV)
            i0 = 1 if how == "odd" else 0
            s.i32_into(ibuf[:, i0:i0 + N])
            assert torch.equal(ibuf[:, i0:i0 + N], o.gemm_w4a8_i32(s.a, s.img, c.w_bits, N)), f"{tag}: int32"
            chk = ibuf.clone()
            chk[:, i0:i0 + N] = -7
            assert bool((chk == -7).all()), f"{tag}: int32 sentinel"
            for act in acts(c, o):
                n_out = N // 2 if act == o.ACT_SILU_MUL else N
                buf, out, c0 = placed(M, n_out, dv, how)
                if how == "odd":
                    with pytest.raises(MQuantHipError):             # an unaligned output: the activation store needs 16-byte rows
                        s.act(dv, act, None, out)
                    with pytest.raises(MQuantHipError):             # parameters the activation epilogue cannot load 16 bytes at a time
                        s.act(dv, act, views)
                else:
                    s.act(dv, act, None, out)
                    assert torch.equal(out, got[("act", act, dv)]) and sentinel_kept(buf, c0, n_out), f"{tag}: act {act}"
            if ("rope", dv) in got:
                want, cos, sin, rc = got[("rope", dv)]
                buf, out, c0 = placed(M, N, dv, how)
                if how == "odd":
                    with pytest.raises(MQuantHipError):             # the rotation's store needs a 16-byte aligned output
                        s.rope(dv, cos, sin, rc, None, out)
                    assert torch.equal(s.rope(dv, cos, sin, rc, views), want), f"{tag}: rope with offset parameters"
                else:
                    s.rope(dv, cos, sin, rc, None, out)
                    assert torch.equal(out, want) and sentinel_kept(buf, c0, N), f"{tag}: rope"
            if ("wg", dv) in got:
                buf, out, c0 = placed(M, N, dv, how)
                wg = offset_view(dev(s_wg)) if how == "odd" else dev(s_wg)
                o.gemm_w4a8_wgroupscale(s.a, s.img, c.w_bits, N, wg, g, s_x0=SX0, s_x1=SX1, row_sel=s.t["sel"],
                                        bias=(p or s.t)["bias"], out=out)
                assert torch.equal(out, got[("wg", dv)]) and sentinel_kept(buf, c0, N), f"{tag}: wgroupscale"
                buf, out, c0 = placed(M, N, dv, how)
                o.gemm_w4a8_groupscale(s.a, s.img, c.w_bits, N, dev(s_xg), g, (p or s.t)["s_w"], bias=(p or s.t)["bias"], out=out)
                assert torch.equal(out, got[("g", dv)]) and sentinel_kept(buf, c0, N), f"{tag}: groupscale"

        # ---- workspace: none, and one too small for the planned split --------------------------------------------------------
        dw = DTYPES[(idx + 1) % 3]
        planned = gc.plan(M, N, c.K_pad, c.w_bits, c.a_tiled)[1]
        small = torch.empty(((max(planned // 2, 1) * M * N * 4 + 15) // 16 * 16,), dtype=torch.uint8, device=DEV)
        acc_full = o.gemm_w4a8_i32(s.a, s.img, c.w_bits, N)
        for ws in (None, small):
            tag = f"{c.name}: workspace {'none' if ws is None else ws.numel()} {dw}"
            monkeypatch.setattr(o, "splitk_workspace", lambda device, nbytes=0, _ws=ws: _ws)
            assert torch.equal(o.gemm_w4a8_i32(s.a, s.img, c.w_bits, N), acc_full), f"{tag}: int32"
            assert torch.equal(s.plain(dw), got[("plain", dw)]), f"{tag}: gemm_w4a8"
            assert torch.equal(s.rowscale(dw), got[("rows", dw)]), f"{tag}: rowscale"
            assert torch.equal(s.rank2(dw, False), got[("r2", dw)]), f"{tag}: rank2"
            assert torch.equal(s.residual(res.to(dw)), got[("res", dw)]), f"{tag}: residual"
            monkeypatch.undo()
        assert torch.equal(o.gemm_w4a8(s.a, s.img, c.w_bits, N, SX0, s.t["s_w"], s_x1=SX1, row_sel=s.t["sel"], bias=s.t["bias"],
                                       out_dtype=dw, use_workspace=False), got[("plain", dw)]), f"{c.name}: use_workspace=False"
    finally:
        o.gemm_debug_force(-1, 0)
