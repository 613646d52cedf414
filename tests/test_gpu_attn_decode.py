"""Decode attention over the e4m3 KV cache (mq_attn_decode_fp8kv, mq_attn_decode_fp8kv_quant_i8; csrc/attn_decode.hip) on the GPU:
every output element within the bound of tests/attn_decode_reference.py (float64 softmax attention over the dequantised cache)
for the cases of tests/attn_decode_cases.py, and the exact properties of the launch -- no tolerance: what lies at or beyond key
n, in another kv head, in the workspace before the call or around the output cannot change a bit of the result."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import attn_decode_cases as cases
from attn_decode_reference import decode_reference, dequant_cache
from attn_reference import assert_within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DTYPES = [torch.float16, torch.bfloat16]
CAP = 1000                  # rows of the shared cases: the largest n of the short lists
_RATIOS = {}                # dtype -> largest error / bound seen (printed at the end with MQ_ATTN_BOUND_REPORT=1)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if os.environ.get("MQ_ATTN_BOUND_REPORT"):
        for k, (r, what) in sorted(_RATIOS.items()):
            print(f"\nlargest error / bound, {k}: {r:.3f} ({what})")


def _within(got, o, bound, what):
    r = assert_within(got, o, bound, what)
    key = str(got.dtype).replace("torch.", "")
    if r > _RATIOS.get(key, (-1.0, None))[0]:
        _RATIOS[key] = (r, what)
    return r


@contextlib.contextmanager
def forced(plan):
    from mquant_amd import ops
    ops.attn_decode_debug_force(*plan)
    try:
        yield
    finally:
        ops.attn_decode_debug_force(0, 0)


@functools.lru_cache(maxsize=None)
def _inputs(dtype, H, HKV, rows=CAP, q_gain=1.0):
    """(q [rows, H, 128], cache [rows, 2 HKV, 128], scale) made once per geometry and never written to"""
    _, q, cache, scale = cases.make_case(rows + H, rows, H, HKV, dtype, DEV, q_gain)
    return q, cache, scale


@functools.lru_cache(maxsize=None)
def _want(dtype, H, HKV, R, n, causal, rows=CAP, q_gain=1.0):
    """the checker's (o, bound) for the last R of the first n rows: one computation for all plans of a shape"""
    q, cache, scale = _inputs(dtype, H, HKV, rows, q_gain)
    k, v = dequant_cache(cache[:n], scale)
    return decode_reference(q[n - R:n], k, v, causal)


def _run(c, dtype, rows=CAP, q_gain=1.0, **kw):
    from mquant_amd import ops
    q, cache, scale = _inputs(dtype, c["heads"], c["kv_heads"], rows, q_gain)
    n, R = c["n"], c["R"]
    with forced(c["plan"]):
        return ops.attn_decode_fp8kv(q[n - R:n], cache, scale, n_keys=n, causal=c["causal"], **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("c", cases.PARITY, ids=cases.case_id)
def test_one_row_is_within_the_bound(c, dtype):
    got = _run(c, dtype)
    _within(got, *_want(dtype, c["heads"], c["kv_heads"], 1, c["n"], True), cases.case_id(c))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("c", cases.ROWS, ids=cases.case_id)
def test_several_rows_are_within_the_bound(c, dtype):
    got = _run(c, dtype)
    _within(got, *_want(dtype, c["heads"], c["kv_heads"], c["R"], c["n"], c["causal"]), cases.case_id(c))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_several_passes_under_the_heuristic_plan(dtype):
    c = dict(R=3, n=300, heads=64, kv_heads=8, causal=True, plan=(0, 0))
    _within(_run(c, dtype), *_want(dtype, 64, 8, 3, 300, True), cases.case_id(c))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_the_long_case(dtype):
    c = cases.LONG
    got = _run(c, dtype, rows=c["n"])
    _within(got, *_want(dtype, c["heads"], c["kv_heads"], 1, c["n"], True, rows=c["n"]), cases.case_id(c))


@pytest.mark.parametrize("plan", [(0, 0), (1, 0), (3, 0)])
def test_peaked_scores(plan):
    c = dict(R=1, n=300, heads=4, kv_heads=2, causal=True, plan=plan)
    got = _run(c, torch.float16, rows=300, q_gain=6.0)
    assert torch.isfinite(got).all()
    _within(got, *_want(torch.float16, 4, 2, 1, 300, True, rows=300, q_gain=6.0), "peaked scores")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_one_key_returns_its_value_row(dtype):
    """n = 1: the softmax is 1, O = V[0] * s_v rounded once"""
    H, HKV = 8, 2
    q, cache, scale = _inputs(dtype, H, HKV)
    got = _run(dict(R=1, n=1, heads=H, kv_heads=HKV, causal=True, plan=(0, 0)), dtype).double()
    v0 = cache.float().double()[0, HKV:] * scale.double()[HKV:, None]
    np.testing.assert_allclose(got[0].view(H, 128).cpu().numpy(), v0.repeat_interleave(H // HKV, dim=0).cpu().numpy(),
                               rtol=2 ** -10 if dtype == torch.float16 else 2 ** -8, atol=1e-6)


@pytest.mark.parametrize("plan", [(1, 0), (3, 0)])
def test_other_kv_heads_cannot_change_a_head_and_two_calls_agree(plan):
    from mquant_amd import ops
    H, HKV, n, R = 8, 2, 300, 2
    q, cache, scale = _inputs(torch.float16, H, HKV)
    with forced(plan):
        a = ops.attn_decode_fp8kv(q[n - R:n], cache, scale, n_keys=n)
        b = ops.attn_decode_fp8kv(q[n - R:n], cache, scale, n_keys=n)
        assert torch.equal(a, b)
        other, scale2 = cache.clone(), scale.clone()
        codes = torch.randint(0, 0x7E, (CAP, 128), device=DEV, dtype=torch.uint8)
        other.view(torch.uint8)[:, 1] = codes                         # K of kv head 1
        other.view(torch.uint8)[:, HKV + 1] = codes.flip(0)           # V of kv head 1
        scale2[1] *= 3.0
        scale2[HKV + 1] *= 0.25
        c = ops.attn_decode_fp8kv(q[n - R:n], other, scale2, n_keys=n)
    half = H // HKV * 128
    assert torch.equal(a[:, :half], c[:, :half])
    assert not torch.equal(a[:, half:], c[:, half:])


@pytest.mark.parametrize("plan", [(1, 0), (3, 0)])
def test_strided_q_and_out_and_nothing_outside_the_output_is_written(plan):
    from mquant_amd import ops
    H, HKV, n, R = 8, 2, 130, 3
    q, cache, scale = _inputs(torch.float16, H, HKV)
    assert q.stride(0) > H * 128                                      # a column slice of the fused q|k|v tensor
    flat = torch.full(((R + 2) * (H * 128 + 64),), 7.0, device=DEV, dtype=torch.float16)
    wide = flat.view(R + 2, H * 128 + 64)
    with forced(plan):
        ops.attn_decode_fp8kv(q[n - R:n], cache, scale, n_keys=n, out=wide[1:R + 1, :H * 128])
        want = ops.attn_decode_fp8kv(q[n - R:n].contiguous(), cache, scale, n_keys=n)
    assert torch.equal(wide[1:R + 1, :H * 128], want)
    assert bool((wide[0] == 7.0).all()) and bool((wide[R + 1] == 7.0).all()) and bool((wide[:, H * 128:] == 7.0).all())


@pytest.mark.parametrize("n_dev", [None, 70])
def test_the_workspace_is_used_inside_its_bytes_and_its_contents_do_not_matter(n_dev):
    """A test-owned workspace of exactly the queried size: the bytes behind it stay, and NaN bit patterns in it before the call give
    the bits that zeros give -- with the key count on the device too, where six of the eight ranges are empty."""
    from mquant_amd import ops
    H, HKV, R = 8, 2, 2
    q, cache, scale = _inputs(torch.float16, H, HKV)
    cap, plan = (512, (8, 64)) if n_dev else (300, (3, 0))
    n = n_dev or cap
    outs = []
    with forced(plan):
        need = ops.attn_decode_workspace_bytes(R, cap, H, HKV)
        assert need > 0
        nk = torch.tensor([n], dtype=torch.int32, device=DEV) if n_dev else n
        for fill in (0xFF, 0x00):
            buf = torch.full((need + 256,), fill, dtype=torch.uint8, device=DEV)
            buf[need:] = 0xA5
            outs.append(ops.attn_decode_fp8kv(q[n - R:n], cache[:cap], scale, n_keys=nk, workspace=buf[:need]))
            assert bool((buf[need:] == 0xA5).all())
            if n_dev:                                                 # the slots of the empty ranges were not written either
                acc = buf[:8 * R * H * 512].view(8, R * H * 512)
                assert bool((acc[2:] == fill).all()) and not bool((acc[:2] == fill).all())
        with pytest.raises(Exception, match=f"workspace of {need} bytes"):
            ops.attn_decode_fp8kv(q[n - R:n], cache[:cap], scale, n_keys=nk, workspace=buf[:need - 16])
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    _within(outs[0], *_want(torch.float16, H, HKV, R, n, True), "test-owned workspace")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("n", [1, 64, 70, 512])
def test_a_key_count_on_the_device(n, dtype):
    """Capacity 512 cut into 8 ranges of 64; cache rows at or beyond n hold 0x7F (e4m3fn NaN): finite, within the bound, and the
    bits of the same call with those rows zeroed."""
    from mquant_amd import ops
    H, HKV, cap = 28, 4, 512
    q, cache, scale = _inputs(dtype, H, HKV)
    nk = torch.tensor([n], dtype=torch.int32, device=DEV)
    outs = []
    with forced((8, 64)):
        for fill in (0x7F, 0x00):
            c = cache[:cap].clone()
            c.view(torch.uint8)[n:] = fill
            outs.append(ops.attn_decode_fp8kv(q[n - 1:n], c, scale, n_keys=nk))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    _within(outs[0], *_want(dtype, H, HKV, 1, n, True), f"device key count {n}")
    with forced((8, 64)):                                             # beyond the capacity: clamped to it
        big = ops.attn_decode_fp8kv(q[cap - 1:cap], cache[:cap], scale, n_keys=torch.tensor([9999], dtype=torch.int32, device=DEV))
        assert torch.equal(big, ops.attn_decode_fp8kv(q[cap - 1:cap], cache[:cap], scale, n_keys=cap))


def test_one_captured_graph_serves_a_growing_cache():
    """A generation loop: the graph holds one decode attention (one stream, no branches) and is replayed for three key counts, the
    cache append and the new query row written between the replays."""
    from mquant_amd import ops
    H, HKV, cap, dtype = 28, 4, 512, torch.float16
    qkv, q_all, _, scale = cases.make_case(77, cap, H, HKV, dtype, DEV)
    kv_all = qkv[:, H * 128:].view(cap, 2 * HKV, 128)
    cache = torch.zeros((cap, 2 * HKV, 128), dtype=torch.float8_e4m3fn, device=DEV)
    cache.view(torch.uint8)[:] = 0x7F                                 # nothing beyond n may matter
    n0 = 190
    ops.kv_quant_fp8(kv_all[:n0], scale, out=cache[:n0])
    q_buf = torch.zeros((1, H, 128), dtype=dtype, device=DEV)
    out = torch.zeros((1, H * 128), dtype=dtype, device=DEV)
    nk = torch.tensor([n0], dtype=torch.int32, device=DEV)
    q_buf.copy_(q_all[n0 - 1:n0])
    ops.attn_decode_fp8kv(q_buf, cache, scale, n_keys=nk, out=out)    # warm-up: the wrapper's workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.attn_decode_fp8kv(q_buf, cache, scale, n_keys=nk, out=out)
    for n in (n0, n0 + 1, n0 + 2):
        if n > n0:
            ops.kv_quant_fp8(kv_all[n - 1:n], scale, out=cache[n - 1:n])       # the append
        q_buf.copy_(q_all[n - 1:n])
        nk.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        k, v = dequant_cache(cache[:n], scale)
        _within(out.clone(), *decode_reference(q_all[n - 1:n], k, v, True), f"replay at n = {n}")


@pytest.mark.parametrize("T,H,HKV", [(129, 4, 2), (768, 28, 4)])
def test_it_agrees_with_the_last_row_of_the_prefill_kernel(T, H, HKV):
    from attn_reference import reference
    from mquant_amd import ops
    q, cache, scale = _inputs(torch.float16, H, HKV)
    pre = ops.attn_prefill_fp8kv(q[:T], cache[:T], scale, causal=True)[T - 1].double()
    dec = ops.attn_decode_fp8kv(q[T - 1:T], cache, scale, n_keys=T)[0].double()
    k, v = dequant_cache(cache[:T], scale)
    _, bound_pre = reference(q[:T], k, v, True)
    _, bound_dec = _want(torch.float16, H, HKV, 1, T, True)
    assert bool(((pre - dec).abs() <= bound_pre[T - 1] + bound_dec[0]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("tiled", [True, False], ids=["tiled", "rows"])
@pytest.mark.parametrize("plan", [(1, 0), (3, 0)])
def test_the_fused_quantizer_equals_decode_then_quantize(plan, tiled, dtype):
    """mq_attn_decode_fp8kv_quant_i8: bit for bit what mq_quantize_act_i8 makes of the 16-bit decode output of the same plan, a
    different scale for each of the two rows."""
    from mquant_amd import ops
    H, HKV, n, R = 28, 4, 300, 2
    q, cache, scale = _inputs(dtype, H, HKV)
    sel = torch.tensor([0, 1], dtype=torch.uint8, device=DEV)
    with forced(plan):
        o = ops.attn_decode_fp8kv(q[n - R:n], cache, scale, n_keys=n)
        s0 = float(o.float().abs().max()) / 127.0 * 0.8               # some values saturate
        s1 = 0.37 * s0
        got = ops.attn_decode_quant_i8(q[n - R:n], cache, scale, s0, s1, n_keys=n, row_sel=sel, tiled=tiled)
    want, _ = ops.quantize_act_i8(o, s0, s1, row_sel=sel, tiled=tiled)
    a = got.to_rows() if tiled else got
    b = want.to_rows() if tiled else want
    assert a.shape == b.shape == (R, H * 128)
    assert torch.equal(a, b)
    assert int(a.abs().max()) >= 127 and not torch.equal(a[0], a[1])
