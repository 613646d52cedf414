"""(Named to be collected behind every older test file: the positions of the existing GPU tests in the run stay what they were.)
Group-wise W4 weights at generation steps: the streaming kernel with the group fold (gemm_skinny.hip, tile id 61 of the weight-group
entry points) promises the BITS of the tiled kernels -- exact int32 inside a group, the fp32 fold in ascending group order -- so every
check here is an equality: against the CPU oracle, against the poison around the output, against the same rows inside a prefill batch,
and of a greedy loop's ids and cache bytes on either path.  One sweeping test per property, each naming every failing configuration."""
import functools
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
MODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
STREAM = 61
# (M, N, K, g); K_pad = K rounded up to 128, zero padded
SHAPES = [(1, 200, 1280, 128),      # G = 10: a ragged second round, a ragged last pair
          (3, 72, 192, 64),         # G = 3 < 8, a zero-padding k-tile, N not a multiple of 16
          (16, 48, 3584, 256),      # G = 14, four k-tiles per group, a full row tile
          (5, 264, 1920, 64),       # G = 30, one k-tile per group
          (9, 520, 19968, 128),     # G = 156: the long reduction, many rounds
          (2, 96, 2048, 512),       # G = 4
          (1, 136, 1024, 1024)]     # G = 1


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


@functools.lru_cache(maxsize=None)
def problem(M, N, K, g):
    """Levels, tables and the device operands of a shape: built once, shared by the tests, never written to."""
    from mquant_amd import ops
    rng = np.random.default_rng(M + N + K + g)
    K_pad, G = (K + 127) // 128 * 128, K // g
    a = np.zeros((M, K_pad), np.int8)
    a[:, :K] = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    stored = rng.integers(-8, 8, size=(N, K), dtype=np.int8)
    wp = np.zeros((N, K_pad), np.int8)
    wp[:, :K] = stored
    d = (8 - rng.integers(0, 16, size=(G, N))).astype(np.int16)
    s_wg = (rng.random((G, N), dtype=np.float32) * 0.01 + 0.001).astype(np.float32)
    bias = rng.normal(size=N).astype(np.float32)
    qmz = (stored.astype(np.int32) + np.repeat(d.T.astype(np.int32), g, axis=1)).astype(np.int8)      # the levels q - z = stored + d
    at = ops.TiledAct.from_rows(to_dev(a))
    dev = dict(at=at, img=ops.prepack(to_dev(wp), 4), s_wg=to_dev(s_wg), d=to_dev(d), bias=to_dev(bias), sums=ops.act_group_rowsum(at, g, G))
    return dict(K_pad=K_pad, G=G, a=a[:, :K], stored=stored, qmz=qmz, s_wg=s_wg, bias=bias, dev=dev)


@functools.lru_cache(maxsize=None)
def scale_case(act, M, G):
    """(keyword arguments of the GEMM wrapper, those of the oracle) for an activation-scale mode"""
    rng = np.random.default_rng(7 * M + G)
    if act == "static":
        return dict(s_x0=0.031), dict(sx0=0.031)
    if act == "msq":
        sel = (rng.random(M) < 0.4).astype(np.uint8)
        sel[0] = 1
        return dict(s_x0=0.031, s_x1=0.0077, row_sel=to_dev(sel)), dict(sx0=0.031, sx1=0.0077, row_sel=sel)
    if act == "rows":
        rows = (rng.random(M, dtype=np.float32) * 0.05 + 0.01).astype(np.float32)
        return dict(s_x_rows=to_dev(rows)), dict(sx_rows=rows)
    s_xg = (rng.random((M, G), dtype=np.float32) * 0.2 + 0.01).astype(np.float32)
    return dict(s_x_groups=to_dev(s_xg)), dict(s_xg=s_xg)


@functools.lru_cache(maxsize=None)
def expected(shape, asym, act):
    """The oracle's fp32 result of a configuration (asymmetric groups: over the levels q - z); rounded per output dtype by the caller."""
    M, N, K, g = shape
    p = problem(*shape)
    return oracle.gemm_wgroup(p["a"], p["qmz"] if asym else p["stored"], p["s_wg"], g, bias=p["bias"], **scale_case(act, M, p["G"])[1])


def run(shape, asym, act, **kw):
    from mquant_amd import ops
    M, N, K, g = shape
    v = problem(*shape)["dev"]
    kw = dict(scale_case(act, M, problem(*shape)["G"])[0], bias=v["bias"], **kw)
    if asym:
        return ops.gemm_w4a8_wgroupscale_asym(v["at"], v["img"], 4, N, v["s_wg"], v["d"], v["sums"], g, **kw)
    return ops.gemm_w4a8_wgroupscale(v["at"], v["img"], 4, N, v["s_wg"], g, **kw)


def planned(shape, asym, act):
    from mquant_amd import ops
    M, N, K, g = shape
    return ops.gemm_group_plan(M, N, problem(*shape)["K_pad"], g, problem(*shape)["G"], x_groups=act == "groups", asym=asym)


def test_bits_equal_the_oracle():
    """Every shape x {symmetric, asymmetric} x {static, MSQ row_sel, per-row, per-group activation scales} x {fp16, bf16, fp32}, with tile 61
    forced and under the plain plan, each launch twice back to back."""
    sweep(_oracle_case, SHAPES, [False, True], ["static", "msq", "rows", "groups"], [torch.float16, torch.bfloat16, torch.float32])


def _oracle_case(shape, asym, act, out_dtype):
    from mquant_amd import ops
    want = oracle.round_to(expected(shape, asym, act), MODE[out_dtype])
    for force in (STREAM, -1):
        try:
            ops.gemm_debug_force(force, 0)
            if force == STREAM:
                assert planned(shape, asym, act) == STREAM, "a forced 61 was not taken"
            y0 = run(shape, asym, act, out_dtype=out_dtype)
            y1 = run(shape, asym, act, out_dtype=out_dtype)
        finally:
            ops.gemm_debug_force(-1, 0)
        np.testing.assert_array_equal(y0.float().cpu().numpy(), want, err_msg=f"force {force}")
        np.testing.assert_array_equal(y1.float().cpu().numpy(), want, err_msg=f"force {force}, second launch")


def test_nothing_is_stored_outside_the_output_block():
    sweep(_poison_case, [(1, 200, 1280, 128), (3, 72, 192, 64)], [False, True], [torch.float16, torch.float32])


def _poison_case(shape, asym, out_dtype):
    """The output is a view with ldo > N inside a poisoned buffer with spare rows: the ragged last pair and the rows past M that a
    workgroup computes leak into no stored element."""
    from mquant_amd import ops
    M, N, K, g = shape
    want = oracle.round_to(expected(shape, asym, "static"), MODE[out_dtype])
    for c0 in (8, 3):                                                        # an aligned view (vector stores) and an odd one (element stores)
        buf = torch.full((M + 2, N + 24), 777.0, dtype=out_dtype, device=DEV)
        out = buf[1:M + 1, c0:c0 + N]
        try:
            ops.gemm_debug_force(STREAM, 0)
            assert planned(shape, asym, "static") == STREAM
            run(shape, asym, "static", out=out)
        finally:
            ops.gemm_debug_force(-1, 0)
        np.testing.assert_array_equal(out.float().cpu().numpy(), want, err_msg=f"column offset {c0}")
        keep = torch.ones_like(buf, dtype=torch.bool)
        keep[1:M + 1, c0:c0 + N] = False
        assert bool((buf[keep] == 777.0).all()), f"column offset {c0}: a store outside the {M} x {N} block"


def rtn_groups(w, g, asym):
    """Seeded group-wise round-to-nearest of fp32 weights [N, K]: (stored int8 levels [N, K], scales fp32 [K / g, N], zero offsets int16
    [K / g, N] or None).  Symmetric: levels -8 .. 7; asymmetric: q in 0 .. 15 stored as q - 8, offsets 8 - z."""
    N, K = w.shape
    wg = w.reshape(N, K // g, g)
    if not asym:
        s = (wg.abs().amax(dim=2) / 7.0).clamp_min(1e-8)
        lv = torch.clamp(torch.round(wg / s[:, :, None]), -8, 7)
        return lv.reshape(N, K).to(torch.int8), s.t().contiguous().float(), None
    lo, hi = wg.amin(dim=2).clamp_max(0.0), wg.amax(dim=2).clamp_min(0.0)
    s = ((hi - lo) / 15.0).clamp_min(1e-8)
    z = torch.round(-lo / s)
    q = torch.clamp(torch.round(wg / s[:, :, None]) + z[:, :, None], 0, 15)
    return (q - 8).reshape(N, K).to(torch.int8), s.t().contiguous().float(), (8 - z).t().contiguous().to(torch.int16)


def test_a_rows_bits_do_not_depend_on_the_batch_it_came_in():
    """A W4A8Linear with weight groups of 128 at the q|k|v shape over 300 rows: rows that arrive alone, five together or as one full row
    tile take the streaming kernel, the 300 rows the tiled ones -- the same bits (mirrors tests/test_gpu_skinny.py for per-channel scales)."""
    sweep(_row_batch_case, [False, True])


def _row_batch_case(asym):
    from mquant_amd import ops
    from mquant_amd.engine import W4A8Linear
    N, K, g = 4608, 3584, 128
    gen = torch.Generator(device=DEV).manual_seed(11 + int(asym))
    w = torch.randn((N, K), generator=gen, device=DEV) * 0.02 + (0.004 if asym else 0.0)
    levels, tbl, offs = rtn_groups(w, g, asym)
    lin = W4A8Linear(levels, torch.ones(N, device=DEV), 4, torch.randn((N,), generator=gen, device=DEV), 0.05, 0.02,
                     w_groups=(tbl, g) if offs is None else (tbl, g, offs))
    x = torch.randn((300, K), generator=gen, device=DEV, dtype=torch.float16)
    sel = (torch.arange(300, device=DEV) % 3 == 0).to(torch.uint8)
    ops.gemm_debug_force(-1, 0)
    assert ops.gemm_group_plan(300, N, K, g, asym=asym) != STREAM
    full = lin.forward(x, sel)
    for rows in ([7], [0, 1, 2, 3, 4], list(range(16, 32))):
        assert ops.gemm_group_plan(len(rows), N, K, g, asym=asym) == STREAM, (len(rows), "rows do not take the streaming kernel")
        idx = torch.tensor(rows, device=DEV)
        part = lin.forward(x.index_select(0, idx).contiguous(), sel.index_select(0, idx).contiguous())
        assert torch.equal(part, full.index_select(0, idx)), (rows[:2], len(rows))


# ---- a greedy loop over group-wise layers ----------------------------------------------------------------------------------------------
DIM, H, HKV, D, INTER, VOCAB, CAP, LAYERS, G128 = 512, 4, 2, 128, 1024, 1000, 32, 2, 128
FIRST, STEPS, EPS = 123, 12, 1e-6


@functools.lru_cache(maxsize=None)
def _toy():
    """(embedding table, lm_head, per layer four W4A8Linear with symmetric weight groups of 128 and static activation scales, cos, sin)"""
    from mquant_amd.engine import W4A8Linear
    from mquant_amd.full_prefill import _rope_tables
    gen = torch.Generator(device=DEV).manual_seed(2025)
    rnd = lambda *shape, s=1.0: torch.randn(shape, generator=gen, device=DEV) * s

    def lin(n, k, s_x):
        levels, tbl, _ = rtn_groups(rnd(n, k, s=k ** -0.5), G128, False)
        return W4A8Linear(levels, torch.ones(n, device=DEV), 4, None, s_x, w_groups=(tbl, G128))
    layers = [dict(qkv=lin((H + 2 * HKV) * D, DIM, 0.03), o=lin(DIM, H * D, 0.03), gate_up=lin(2 * INTER, DIM, 0.03), down=lin(DIM, INTER, 0.02))
              for _ in range(LAYERS)]
    cos, sin = _rope_tables(CAP, D, DEV, torch.float16)
    return rnd(VOCAB, DIM).half(), rnd(VOCAB, DIM, s=0.05).half(), layers, cos[:, 0].contiguous(), sin[:, 0].contiguous()


def _greedy(force, capture):
    """start(0, token), [capture()], generate(STEPS) under a forced tile -> (ids, the token picked last, the cache bytes per layer)"""
    from mquant_amd import GreedyLoop, KVCache16, ops
    table, lm_head, layers, cos, sin = _toy()
    cache = KVCache16(LAYERS, CAP, HKV, D, cos, sin, DEV, torch.float16)
    for c in cache.caches:
        c.view(torch.int16)[:] = 0x7E00                               # an fp16 NaN: every row that matters is written by the loop itself

    def body(h):
        for i, L in enumerate(layers):
            x = F.rms_norm(h, (DIM,), eps=EPS)
            h = h + L["o"].forward(cache.step(i, L["qkv"].forward(x), H))
            x = F.rms_norm(h, (DIM,), eps=EPS)
            gu = L["gate_up"].forward(x)
            h = h + L["down"].forward(F.silu(gu[:, :INTER]) * gu[:, INTER:])
        return h
    try:
        ops.gemm_debug_force(force, 0)
        loop = GreedyLoop(cache, table, lm_head, body, eps=EPS)
        loop.start(0, FIRST)
        if capture:
            loop.capture()
        ids = loop.generate(STEPS).tolist()
        token = int(loop.token.item())
    finally:
        ops.gemm_debug_force(-1, 0)
    assert int(cache.n_keys.item()) == STEPS
    return ids, token, [c.view(torch.int16).clone() for c in cache.caches]


def test_a_greedy_loop_gives_the_same_ids_on_either_path():
    """GreedyLoop over KVCache16, two layers whose every Linear has symmetric weight groups of 128: captured replays on the streaming
    kernel, the same with the tiled kernel forced, and the streaming run eagerly -- ids, the last token and every cache byte are equal
    (no tolerance: both paths promise the same bits)."""
    from mquant_amd import ops
    ops.gemm_debug_force(-1, 0)
    calls = [((H + 2 * HKV) * D, DIM), (DIM, H * D), (2 * INTER, DIM), (DIM, INTER)]
    assert all(ops.gemm_group_plan(1, n, k, G128) == STREAM for n, k in calls), [ops.gemm_group_plan(1, n, k, G128) for n, k in calls]
    # the id these calls take without the streaming kernel: the tile plan is the same for every M up to one 64-row tile, and 17 rows
    # are past the streaming kernel's single row tile
    tiled = {ops.gemm_group_plan(17, n, k, G128) for n, k in calls}
    assert len(tiled) == 1 and STREAM not in tiled, tiled
    tiled = tiled.pop()
    try:
        ops.gemm_debug_force(tiled, 0)
        assert all(ops.gemm_group_plan(1, n, k, G128) == tiled for n, k in calls)
    finally:
        ops.gemm_debug_force(-1, 0)
    ids, token, rows = _greedy(-1, True)
    assert ids[0] == FIRST and all(0 <= t < VOCAB for t in ids + [token]) and len(set(ids + [token])) > 2, ids
    for name, (ids2, token2, rows2) in (("tiled kernel forced", _greedy(tiled, True)), ("eager", _greedy(-1, False))):
        assert ids2 == ids and token2 == token, (name, ids, ids2, token, token2)
        assert all(torch.equal(a, b) for a, b in zip(rows, rows2)), (name, "cache bytes differ")
