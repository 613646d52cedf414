"""Decode attention over a 16-bit KV cache (mq_attn_decode, mq_attn_decode_quant_i8; csrc/attn_decode.hip with KVB = 2) on the GPU.

The inputs are those of tests/attn_decode_cases.make_case: q is the Q columns of one fused tensor and the cache is its K|V columns
THEMSELVES, in q's dtype and unquantised (gains 0.05 / 1 / 6 / 20 per head) -- a strided view, as a generation step has it.  The
checker is tests/attn_decode_reference.decode_reference over the cache halves with its bound and constant unchanged.

Two kinds of test: within the bound (B2, B7), and exact properties with no tolerance -- above all B1: the 16-bit kernel is the
e4m3 kernel with both scales 1.0f, so on a cache holding exactly the e4m3 VALUES (every one is exact in fp16 and bf16) it must
give the e4m3 kernel's bits under the same forced plan, which pins every index of the new load path.

The cases of a property are walked INSIDE one test (a few hundred launches of microseconds each), so that the file adds two dozen
items to the suite, not five hundred; every assertion names its case."""
import contextlib
import functools

import pytest
import torch

import attn_decode_cases as cases
from attn_decode_reference import decode_reference
from attn_reference import assert_within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
CAP = 1000                  # rows of the shared cases: the largest n of the short lists
D = 128
# two NaN / Inf bit patterns per dtype, as int16
POISON = {torch.float16: (0x7E00, 0x7C00), torch.bfloat16: (0x7FC0, 0x7F80)}


@contextlib.contextmanager
def forced(plan):
    from mquant_amd import ops
    ops.attn_decode_debug_force(*plan)
    try:
        yield
    finally:
        ops.attn_decode_debug_force(0, 0)


@functools.lru_cache(maxsize=None)
def _inputs(dtype, H, HKV, rows=CAP):
    """(q [rows, H, 128], cache16 [rows, 2 HKV, 128]: both column slices of one qkv; cache8, scale: its e4m3 form) made once per
    geometry and never written to"""
    qkv, q, cache8, scale = cases.make_case(rows + H, rows, H, HKV, dtype, DEV)
    cache16 = qkv[:, H * D:].view(rows, 2 * HKV, D)
    assert cache16.stride(0) == (H + 2 * HKV) * D and cache16.data_ptr() == qkv.data_ptr() + H * D * 2
    return q, cache16, cache8, scale


@functools.lru_cache(maxsize=None)
def _want(dtype, H, HKV, R, n, causal, rows=CAP):
    """the checker's (o, bound) for the last R of the first n rows: one computation for all plans of a shape"""
    q, cache, _, _ = _inputs(dtype, H, HKV, rows)
    return decode_reference(q[n - R:n], cache[:n, :HKV], cache[:n, HKV:], causal)


def _run(c, dtype, rows=CAP, **kw):
    from mquant_amd import ops
    q, cache, _, _ = _inputs(dtype, c["heads"], c["kv_heads"], rows)
    n, R = c["n"], c["R"]
    with forced(c["plan"]):
        return ops.attn_decode(q[n - R:n], cache, n_keys=n, causal=c["causal"], **kw)


def _poisoned(cache, n, dtype, poison):
    """a compact copy of `cache` whose rows [n, capacity) hold NaN and Inf bit patterns, or zeros"""
    c = cache.contiguous().clone()
    tail = c.view(torch.int16)[n:]
    tail.zero_()
    if poison:
        tail[..., 0::2] = POISON[dtype][0]
        tail[..., 1::2] = POISON[dtype][1]
    return c


def _count(n, on_device):
    return torch.tensor([n], dtype=torch.int32, device=DEV) if on_device else n


# ---- B1: the bits of the e4m3 kernel on equal values
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_equal_values_give_the_bits_of_the_e4m3_kernel(dtype):
    for H, HKV in [(28, 4), (4, 1)]:
        for plan in [(1, 0), (3, 0), (0, 32)]:
            _equal_bits(H, HKV, plan, dtype)


def _equal_bits(H, HKV, plan, dtype):
    from mquant_amd import ops
    q, _, cache8, _ = _inputs(dtype, H, HKV)
    ones = torch.ones((2 * HKV,), dtype=torch.float32, device=DEV)
    cache16 = ops.kv_dequant_fp8(cache8, ones, dtype)
    assert torch.equal(cache16.float(), cache8.float())               # every e4m3 value is exact in the 16-bit dtype
    sel = torch.tensor([0, 1, 1], dtype=torch.uint8, device=DEV)
    ran = 0
    for n in (1, 63, 64, 65, 130, 1000):
        for R in (1, 3):
            if n < R or cases.plan_is_refused(n, plan):               # no call exists for these: the plan function refuses them
                continue
            for causal in (True, False):
                with forced(plan):
                    a = ops.attn_decode(q[n - R:n], cache16, n_keys=n, causal=causal)
                    b = ops.attn_decode_fp8kv(q[n - R:n], cache8, ones, n_keys=n, causal=causal)
                    s0 = max(float(b.float().abs().max()), 1e-3) / 127.0 * 0.8
                    a8 = ops.attn_decode_quant_i8(q[n - R:n], cache16, None, s0, 0.37 * s0, n_keys=n, causal=causal, row_sel=sel[:R])
                    b8 = ops.attn_decode_quant_i8(q[n - R:n], cache8, ones, s0, 0.37 * s0, n_keys=n, causal=causal, row_sel=sel[:R])
                what = f"heads {H}/{HKV} plan {plan} n {n} R {R} causal {causal}"
                assert torch.isfinite(b).all() and bool((b != 0).any()), what
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), what
                assert a8.dtype == torch.int8 and torch.equal(a8, b8), what
                ran += 1
    assert ran >= 8


# ---- B2: within the bound
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_one_row_is_within_the_bound(dtype):
    """every case of attn_decode_cases.PARITY"""
    assert len(cases.PARITY) > 100
    for c in cases.PARITY:
        assert_within(_run(c, dtype), *_want(dtype, c["heads"], c["kv_heads"], 1, c["n"], True), cases.case_id(c))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_several_rows_several_passes_and_the_long_case_are_within_the_bound(dtype):
    """every case of attn_decode_cases.ROWS, then R = 3 at 64 / 8 heads over 300 keys under the heuristic plan (two passes), then LONG"""
    for c in cases.ROWS + [dict(R=3, n=300, heads=64, kv_heads=8, causal=True, plan=(0, 0))]:
        assert_within(_run(c, dtype), *_want(dtype, c["heads"], c["kv_heads"], c["R"], c["n"], c["causal"]), cases.case_id(c))
    c = cases.LONG
    got = _run(c, dtype, rows=c["n"])
    assert_within(got, *_want(dtype, c["heads"], c["kv_heads"], 1, c["n"], True, rows=c["n"]), cases.case_id(c))


# ---- B3: nothing at or beyond key n
B3_CAP = 96                 # three ranges of 32 keys under the plan (3, 0) when the count is on the device
B3 = [(n, plan, on_device) for n in (1, 64, 70) for plan in [(1, 0), (3, 0)] for on_device in (False, True)
      if on_device or not cases.plan_is_refused(n, plan)]      # a host n IS the plan's T: (3, 0) cannot cut 1 or 64 keys in three


def test_nothing_beyond_n_reaches_the_output():
    assert len(B3) == 10          # twelve combinations less (3, 0) with a host n of 1 and of 64
    for dtype in DTYPES:
        for n, plan, on_device in B3:
            _nothing_beyond_n(n, plan, on_device, dtype)


def _nothing_beyond_n(n, plan, on_device, dtype):
    from mquant_amd import ops
    H, HKV = 28, 4
    q, cache, _, _ = _inputs(dtype, H, HKV)
    outs = []
    with forced(plan):
        for poison in (True, False):
            c = _poisoned(cache[:B3_CAP], n, dtype, poison)
            assert bool(torch.isnan(c[n:].float()).any()) == poison == bool(torch.isinf(c[n:].float()).any())
            outs.append(ops.attn_decode(q[n - 1:n], c, n_keys=_count(n, on_device)))
    what = f"poison beyond n = {n}, plan {plan}, device count {on_device}, {dtype}"
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), what
    assert_within(outs[0], *_want(dtype, H, HKV, 1, n, True), what)


# ---- B4: the key count on the device
def test_a_key_count_on_the_device():
    for dtype in DTYPES:
        for plan in [(1, 0), (0, 32)]:
            for n_dev, acts_as in [("R", "R"), (40, 40), (96, 96), (9999, 96), (0, "R")]:
                _device_key_count(n_dev, acts_as, plan, dtype)


def _device_key_count(n_dev, acts_as, plan, dtype):
    """n_keys as a tensor: the bits of the host-n call under the same forced plan (whole ranges of 32 keys, or one range: the
    ranges that hold keys are the same either way, the others are empty and not merged); beyond the capacity it acts as the
    capacity, below R as R.  The rows at and beyond n hold NaN / Inf patterns."""
    from mquant_amd import ops
    H, HKV, R, cap = 28, 4, 3, 96
    n_dev, n = (R if n_dev == "R" else n_dev), (R if acts_as == "R" else acts_as)
    q, cache, _, _ = _inputs(dtype, H, HKV)
    c = _poisoned(cache[:cap], n, dtype, True)
    nk = torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    with forced(plan):
        got = ops.attn_decode(q[n - R:n], c, n_keys=nk)
        want = ops.attn_decode(q[n - R:n], c, n_keys=n)
    what = f"device key count {n_dev}, plan {plan}, {dtype}"
    assert int(nk.item()) == n_dev, what                              # read, never written
    assert torch.isfinite(want).all() and torch.equal(got.view(torch.int16), want.view(torch.int16)), what
    assert_within(got, *_want(dtype, H, HKV, R, n, True), what)


def test_one_captured_graph_serves_a_growing_cache():
    """One graph holds one decode attention; it is replayed at three growing lengths, the new cache row and the new query row
    copied in between.  Each replay gives the bits of an eager call."""
    from mquant_amd import ops
    H, HKV, cap, dtype, n0 = 28, 4, 512, torch.float16, 190
    q_all, kv_all, _, _ = _inputs(dtype, H, HKV)
    cache = _poisoned(kv_all[:cap], n0, dtype, True)
    q_buf = q_all[n0 - 1:n0].contiguous()
    out = torch.zeros((1, H * D), dtype=dtype, device=DEV)
    nk = torch.tensor([n0], dtype=torch.int32, device=DEV)
    ops.attn_decode(q_buf, cache, n_keys=nk, out=out)                 # warm-up: the wrapper's workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.attn_decode(q_buf, cache, n_keys=nk, out=out)
    seen = []
    for n in (n0, n0 + 1, n0 + 70):
        cache[n0:n].copy_(kv_all[n0:n])                               # the appends
        q_buf.copy_(q_all[n - 1:n])
        nk.fill_(n)
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.attn_decode(q_all[n - 1:n], cache, n_keys=nk)
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16)), n
        assert_within(out.clone(), *_want(dtype, H, HKV, 1, n, True), f"replay at n = {n}")
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- B5: strided and padded
def test_strided_operands_a_padded_cache_and_a_poisoned_workspace():
    for plan in [(1, 0), (3, 0)]:
        _strided_and_padded(plan)


def _strided_and_padded(plan):
    from mquant_amd import ops
    H, HKV, n, R, dtype = 8, 2, 130, 3, torch.float16
    q, cache, _, _ = _inputs(dtype, H, HKV)
    assert q.stride(0) > H * D                                        # a column slice of the fused q|k|v tensor
    row = 2 * HKV * D
    padded = torch.full((n, row + 64), float("nan"), dtype=dtype, device=DEV)
    padded[:, :row] = cache[:n].reshape(n, row)
    pcache = padded[:, :row].unflatten(1, (2 * HKV, D))
    assert pcache.stride() == (row + 64, D, 1) and pcache.data_ptr() == padded.data_ptr()
    wide = torch.full((R + 2, H * D + 64), 7.0, dtype=dtype, device=DEV)
    with forced(plan):
        need = ops.attn_decode_workspace_bytes(R, n, H, HKV)
        assert (need > 0) == (plan[0] > 1)
        ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=DEV)      # fp32 NaN patterns in the workspace
        ws[need:] = 0xA5
        ops.attn_decode(q[n - R:n], pcache, n_keys=n, out=wide[1:R + 1, :H * D], workspace=ws[:need] if need else None)
        want = ops.attn_decode(q[n - R:n].contiguous(), cache[:n].contiguous(), n_keys=n)
    assert torch.isfinite(want).all() and torch.equal(wide[1:R + 1, :H * D].view(torch.int16), want.view(torch.int16))
    assert bool((wide[0] == 7.0).all()) and bool((wide[R + 1] == 7.0).all()) and bool((wide[:, H * D:] == 7.0).all())
    assert bool((ws[need:] == 0xA5).all()) and bool(torch.isnan(padded[:, row:]).all())
    assert_within(want, *_want(dtype, H, HKV, R, n, True), "strided and padded")


# ---- B6: other kv heads, repeatability
def test_other_kv_heads_cannot_change_a_head_and_two_calls_agree():
    for plan in [(1, 0), (3, 0)]:
        _other_kv_heads(plan)


def _other_kv_heads(plan):
    from mquant_amd import ops
    H, HKV, n, R, dtype = 8, 2, 300, 2, torch.float16
    q, cache, _, _ = _inputs(dtype, H, HKV)
    with forced(plan):
        a = ops.attn_decode(q[n - R:n], cache, n_keys=n)
        b = ops.attn_decode(q[n - R:n], cache, n_keys=n)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        other = cache.contiguous().clone()
        g = torch.Generator(device=DEV).manual_seed(5)
        other[:, 1] = torch.randn((CAP, D), generator=g, device=DEV).to(dtype)           # K of kv head 1
        other[:, HKV + 1] = torch.randn((CAP, D), generator=g, device=DEV).to(dtype)     # V of kv head 1
        c = ops.attn_decode(q[n - R:n], other, n_keys=n)
    half = H // HKV * D
    assert torch.equal(a[:, :half].view(torch.int16), c[:, :half].view(torch.int16))
    assert not torch.equal(a[:, half:], c[:, half:])


# ---- B7: the prefill kernel's last row
def test_it_agrees_with_the_last_row_of_the_prefill_kernel():
    for T, H, HKV in [(129, 4, 2), (768, 28, 4)]:
        _prefill_last_row(T, H, HKV)


def _prefill_last_row(T, H, HKV):
    from attn_reference import reference
    from mquant_amd import ops
    dtype = torch.float16
    q, cache, _, _ = _inputs(dtype, H, HKV)
    k, v = cache[:T, :HKV], cache[:T, HKV:]                           # the same buffer: v = cache + kv_heads * 128
    pre = ops.attn_prefill(q[:T], k, v, causal=True)[T - 1].double()
    dec = ops.attn_decode(q[T - 1:T], cache, n_keys=T)[0].double()
    o_pre, bound_pre = reference(q[:T], k, v, True)
    o_dec, bound_dec = _want(dtype, H, HKV, 1, T, True)
    assert bool(((pre - o_pre[T - 1]).abs() <= bound_pre[T - 1]).all()) and bool(((dec - o_dec[0]).abs() <= bound_dec[0]).all())
    assert bool(((pre - dec).abs() <= bound_pre[T - 1] + bound_dec[0]).all())


# ---- B8: the fused quantizer
def test_the_fused_quantizer_equals_decode_then_quantize():
    for dtype in DTYPES:
        for tiled in (True, False):
            for plan in [(1, 0), (3, 0)]:
                _fused_quantizer(plan, tiled, dtype)
    _quantizer_wrapper_names_both_accepted_forms()


def _fused_quantizer(plan, tiled, dtype):
    from mquant_amd import ops
    H, HKV, n, R = 28, 4, 300, 2
    q, cache, _, _ = _inputs(dtype, H, HKV)
    sel = torch.tensor([0, 1], dtype=torch.uint8, device=DEV)
    with forced(plan):
        o = ops.attn_decode(q[n - R:n], cache, n_keys=n)
        s0 = float(o.float().abs().max()) / 127.0 * 0.8               # some values saturate
        s1 = 0.37 * s0
        got = ops.attn_decode_quant_i8(q[n - R:n], cache, None, s0, s1, n_keys=n, row_sel=sel, tiled=tiled)
    want, _ = ops.quantize_act_i8(o, s0, s1, row_sel=sel, tiled=tiled)
    a = got.to_rows() if tiled else got
    b = want.to_rows() if tiled else want
    assert a.shape == b.shape == (R, H * D)
    assert torch.equal(a, b)
    assert int(a.abs().max()) >= 127 and not torch.equal(a[0], a[1])


def _quantizer_wrapper_names_both_accepted_forms():
    from mquant_amd import ops
    q, cache, cache8, scale = _inputs(torch.float16, 4, 1)
    for bad in [(cache, scale), (cache8, None), (cache.to(torch.bfloat16), None)]:
        with pytest.raises(AssertionError, match="float8_e4m3fn cache with its kv_scale, or a cache of q's dtype"):
            ops.attn_decode_quant_i8(q[:1], bad[0], bad[1], 0.1)
    with pytest.raises(AssertionError):
        ops.attn_decode(q[:1], cache8)


# ---- B9: offsets past 2^31 bytes
LD_WIDE = 1 << 24           # elements: a 32 MiB row stride
WIDE_ROWS = 90              # (90 + 32) x 32 MiB < 4 GiB; row 64 starts 2^31 bytes in


@pytest.fixture(scope="module")
def big():
    buf = torch.empty(((WIDE_ROWS + 7) * LD_WIDE * 2,), dtype=torch.uint8, device=DEV)      # 97 rows: about 3 GiB
    assert buf.data_ptr() % 16 == 0
    yield buf
    del buf
    torch.cuda.empty_cache()


def _wide_cache(big, rows, dtype, HKV):
    view = big.view(dtype)[:rows * LD_WIDE].view(rows, LD_WIDE)
    cache = view[:, :2 * HKV * D].unflatten(1, (2 * HKV, D))
    assert cache.data_ptr() == big.data_ptr() and cache.stride() == (LD_WIDE, D, 1)
    return cache


def test_cache_rows_beyond_2_gib(big):
    for dtype in DTYPES:
        _rows_beyond_2_gib(big, dtype)
    _one_more_block_reaches_4_gib_and_is_refused(big)


def _rows_beyond_2_gib(big, dtype):
    from mquant_amd import ops
    H, HKV, n = 4, 2, WIDE_ROWS
    q, cache, _, _ = _inputs(dtype, H, HKV)
    compact = cache[:n].contiguous()
    wide = _wide_cache(big, n, dtype, HKV)
    wide.copy_(compact)
    assert wide[64].data_ptr() - big.data_ptr() == 1 << 31 and torch.equal(wide.view(torch.int16), compact.view(torch.int16))
    short = ops.attn_decode(q[n - 1:n], compact, n_keys=64, causal=False)      # the rows below 2 GiB alone
    for plan in [(1, 0), (3, 0)]:
        with forced(plan):
            got = ops.attn_decode(q[n - 1:n], wide, n_keys=n)
            want = ops.attn_decode(q[n - 1:n], compact, n_keys=n)
        assert torch.isfinite(want).all() and torch.equal(got.view(torch.int16), want.view(torch.int16)), plan
        assert not torch.equal(want, short)                           # the rows beyond 2 GiB matter to the result
        assert_within(got, *_want(dtype, H, HKV, 1, n, True), f"32 MiB row stride, plan {plan}")


def _one_more_block_reaches_4_gib_and_is_refused(big):
    from mquant_amd import ops
    from mquant_amd._lib import MQuantHipError
    H, HKV, rows = 4, 2, WIDE_ROWS + 7
    assert (rows + 32) * LD_WIDE * 2 >= 1 << 32 > (WIDE_ROWS + 32) * LD_WIDE * 2
    wide = _wide_cache(big, rows, torch.float16, HKV)
    q = torch.zeros((1, H, D), dtype=torch.float16, device=DEV)
    out = torch.full((1, H * D), 7.0, dtype=torch.float16, device=DEV)
    for on_device in (False, True):
        with pytest.raises(MQuantHipError, match=r"mq_attn_decode failed \(status -1\): .*must stay below 4 GiB \(T 97, stride 33554432 bytes\)"):
            ops.attn_decode(q, wide, n_keys=_count(rows, on_device), out=out)
    with pytest.raises(MQuantHipError, match=r"mq_attn_decode_quant_i8 failed \(status -1\): .*must stay below 4 GiB"):
        ops.attn_decode_quant_i8(q, wide, None, 0.05, n_keys=rows)
    assert bool((out == 7.0).all())                                   # nothing was launched
