"""The generation step's cache append (mq_kv_append_rope_fp8, csrc/kv_append.hip; ops.kv_append_rope_fp8, kv_cache.Fp8KVCache) on
the GPU.  The contract is bit-identity with two existing entry points -- ``rope_inplace`` on the R new rows, then ``kv_quant_fp8``
of the rotated K | V columns into cache rows [n - R, n) -- so every comparison is exact, and each looks at WHOLE buffers: the
sentinel columns behind qkv, its V columns, the padding of the cache rows and every cache row outside [n - R, n) included.

Inputs as in tests/attn_decode_cases.make_case (gains 0.05 / 1 / 6 / 20 on the K / V heads, scales from the absmax), for any
head_dim, with the scale of K head 0 made 4x too small: its values leave +-448 and meet the clamp.  qkv sits in a wider buffer
(row stride = columns + 8), the cache is a slice of a wider byte buffer (row stride = 2 HKV D + 16) pre-filled with 0x7F (an
e4m3fn NaN).  The cache holds 96 rows throughout."""
import functools

import numpy as np
import pytest
import torch

import oracle
from attn_decode_reference import decode_reference, dequant_cache
from attn_reference import assert_within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
CAP = 96                    # cache rows
TABLE_ROWS = 104            # rows of cos / sin: a few more than the cache has, so that a small offset stays inside
SENTINEL = 7.0
GEOMETRIES = [(28, 4, 128), (8, 8, 128), (4, 1, 128), (4, 2, 64), (2, 1, 16)]      # (28, 4, 128) at R = 8: nine workgroups


@functools.lru_cache(maxsize=None)
def _inputs(dtype, H, HKV, D):
    """(raw qkv [CAP, (H + 2 HKV) D], scale [2 HKV], cos, sin [TABLE_ROWS, D]) made once per geometry and never written to"""
    from mquant_amd import ops
    from mquant_amd.full_prefill import _rope_tables
    g = torch.Generator(device=DEV).manual_seed(1000 * H + 10 * HKV + D)
    raw = (torch.randn(CAP, (H + 2 * HKV) * D, generator=g, device=DEV) * 0.8).to(dtype)
    gain = torch.tensor([0.05, 1.0, 6.0, 20.0] * HKV, device=DEV)[:2 * HKV].repeat_interleave(D)
    raw[:, H * D:] = (raw[:, H * D:].float() * gain).to(dtype)
    scale = ops.kv_scale_from_absmax(raw[:, H * D:].view(CAP, 2 * HKV, D))
    scale[0] *= 0.25                                                  # K head 0 saturates
    cos, sin = _rope_tables(TABLE_ROWS, D, torch.device(DEV), dtype)
    return raw, scale, cos[:, 0].contiguous(), sin[:, 0].contiguous()


def _buffers(rows, HKV, D):
    """(wide qkv buffer [R, cols + 8] holding `rows` and sentinels, its [R, cols] view, cache byte buffer [CAP, 2 HKV D + 16] of 0x7F,
    its e4m3 view [CAP, 2 HKV, D])"""
    R, cols = rows.shape
    wide = torch.full((R, cols + 8), SENTINEL, dtype=rows.dtype, device=DEV)
    wide[:, :cols] = rows
    buf = torch.full((CAP, 2 * HKV * D + 16), 0x7F, dtype=torch.uint8, device=DEV)
    cache = buf[:, :2 * HKV * D].view(torch.float8_e4m3fn).unflatten(1, (2 * HKV, D))
    assert cache.data_ptr() == buf.data_ptr() and cache.stride() == (2 * HKV * D + 16, D, 1)
    return wide, wide[:, :cols], buf, cache


def _reference(rows, H, HKV, D, scale, cos_rows=None, sin_rows=None):
    """rope_inplace with one table row per qkv row, then kv_quant_fp8: (rotated rows [R, cols], cache bytes [R, 2 HKV D])"""
    from mquant_amd import ops
    ref = rows.clone()
    if cos_rows is not None:
        ops.rope_inplace(ref[:, :(H + HKV) * D], H + HKV, D, cos_rows.contiguous(), sin_rows.contiguous())
    q8 = ops.kv_quant_fp8(ref[:, H * D:].view(-1, 2 * HKV, D), scale)
    return ref, q8.view(torch.uint8).reshape(rows.shape[0], 2 * HKV * D)


def _expected(rows, n, ref, ref_bytes):
    """the two whole buffers after an append of `rows` at key count n"""
    R, cols = rows.shape
    wide = torch.full((R, cols + 8), SENTINEL, dtype=rows.dtype, device=DEV)
    wide[:, :cols] = ref
    buf = torch.full((CAP, ref_bytes.shape[1] + 16), 0x7F, dtype=torch.uint8, device=DEV)
    buf[n - R:n, :ref_bytes.shape[1]] = ref_bytes
    return wide, buf


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _append(dtype, H, HKV, D, R, n_rows, rotate=True, **kw):
    """One fused call on fresh buffers with the raw rows [n_rows - R, n_rows): (wide, buf) afterwards."""
    from mquant_amd import ops
    raw, scale, cos, sin = _inputs(dtype, H, HKV, D)
    wide, qkv, buf, cache = _buffers(raw[n_rows - R:n_rows], HKV, D)
    cos, sin = kw.pop("tables", (cos, sin) if rotate else (None, None))
    out = ops.kv_append_rope_fp8(qkv, H, cache, scale, cos, sin, **kw)
    assert out is qkv
    return wide, buf


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("H,HKV,D", GEOMETRIES)
@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("n", ["R", 65, 96])
def test_it_equals_rope_inplace_then_kv_quant_fp8(n, R, H, HKV, D, dtype):
    n = R if n == "R" else n
    raw, scale, cos, sin = _inputs(dtype, H, HKV, D)
    rows = raw[n - R:n]
    ref, ref_bytes = _reference(rows, H, HKV, D, scale, cos[n - R:n], sin[n - R:n])
    wide, buf = _append(dtype, H, HKV, D, R, n, n_keys=n)
    want_wide, want_buf = _expected(rows, n, ref, ref_bytes)
    assert _same_bits(wide, want_wide)                                # Q and K rotated, V and the sentinels untouched
    assert torch.equal(buf, want_buf)                                 # rows [n - R, n) written, everything else still 0x7F
    if D == 128:                                                      # the clamp was met: +-448 is the code 0x7E
        assert bool(((ref_bytes[:, :D] & 0x7F) == 0x7E).any()) and not bool(((ref_bytes[:, D:] & 0x7F) == 0x7F).any())
    if n > 1:
        assert not _same_bits(ref[:, :(H + HKV) * D], rows[:, :(H + HKV) * D])      # something was rotated


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_it_equals_the_torch_formula_and_the_oracle(dtype):
    """No GPU kernel in the reference: the rotate-half formula with torch ops on CPU tensors of the dtype (one rounding per op),
    then the C oracle's e4m3 quantizer."""
    from mquant_amd.full_prefill import _rope
    H, HKV, D, R, n = 28, 4, 128, 3, 65
    raw, scale, cos, sin = _inputs(dtype, H, HKV, D)
    wide, buf = _append(dtype, H, HKV, D, R, n, n_keys=n)
    rows = raw[n - R:n].cpu()
    c, s = cos[n - R:n].cpu()[:, None, :], sin[n - R:n].cpu()[:, None, :]
    qk = _rope(rows[:, :(H + HKV) * D].view(R, H + HKV, D), c, s)
    assert qk.dtype == dtype
    want = torch.cat([qk.reshape(R, -1), rows[:, (H + HKV) * D:]], dim=1)
    assert _same_bits(wide[:, :want.shape[1]].cpu(), want)
    want8 = oracle.kv_quant_fp8(want[:, H * D:].view(R, 2 * HKV, D).float().numpy(), scale.cpu().numpy())
    np.testing.assert_array_equal(buf[n - R:n, :2 * HKV * D].cpu().numpy(), want8.reshape(R, -1))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n_dev,acts_as", [("R", "R"), (40, 40), (96, 96), (9999, 96), (0, "R")])
def test_a_key_count_on_the_device(n_dev, acts_as, dtype):
    """n_keys as a tensor: the bits of the host-n call; beyond the capacity it acts as the capacity, below R as R."""
    H, HKV, D, R = 28, 4, 128, 3
    n_dev, n = (R if n_dev == "R" else n_dev), (R if acts_as == "R" else acts_as)
    nk = torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    wide, buf = _append(dtype, H, HKV, D, R, n, n_keys=nk)
    want_wide, want_buf = _append(dtype, H, HKV, D, R, n, n_keys=n)
    assert _same_bits(wide, want_wide) and torch.equal(buf, want_buf)
    assert int(nk.item()) == n_dev                                    # read, never written
    assert bool((buf[n - R:n, :2 * HKV * D] != 0x7F).any())


@pytest.mark.parametrize("as_tensor", [True, False], ids=["tensor", "int"])
@pytest.mark.parametrize("n,delta", [(40, 7), (40, -3), (96, 6), (40, 1000), (40, -1000), (2, -1)])
def test_a_rope_position_offset(n, delta, as_tensor):
    """Row r uses table row clamp(t + delta, 0, rows - 1): the host-side call on the table re-indexed that way.  (96, 6): rows 99,
    100, 101; (2, -1) at R = 2: rows 0 (clamped) and 0; +-1000 leave the table altogether."""
    H, HKV, D, R, dtype = 4, 1, 128, 2 if n == 2 else 3, torch.float16
    raw, scale, cos, sin = _inputs(dtype, H, HKV, D)
    idx = (torch.arange(TABLE_ROWS, device=DEV) + delta).clamp(0, TABLE_ROWS - 1)
    want_wide, want_buf = _append(dtype, H, HKV, D, R, n, n_keys=n, tables=(cos[idx].contiguous(), sin[idx].contiguous()))
    d = torch.tensor([delta], dtype=torch.int32, device=DEV) if as_tensor else delta
    nk = torch.tensor([n], dtype=torch.int32, device=DEV) if as_tensor else n
    wide, buf = _append(dtype, H, HKV, D, R, n, n_keys=nk, rope_delta=d)
    assert _same_bits(wide, want_wide) and torch.equal(buf, want_buf)
    if abs(delta) < 100:                                              # ... and the offset did something
        plain, _ = _append(dtype, H, HKV, D, R, n, n_keys=n)
        assert not _same_bits(wide, plain)
    if delta == 7:                                                    # the contiguous slice, literally
        w2, b2 = _append(dtype, H, HKV, D, R, n, n_keys=n, tables=(cos[7:], sin[7:]))
        assert _same_bits(wide, w2) and torch.equal(buf, b2)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("H,HKV,D", [(28, 4, 128), (2, 1, 16)])
def test_append_only(H, HKV, D, dtype):
    """cos = sin = None: qkv keeps its bits, the cache rows are kv_quant_fp8 of the K | V columns as they are."""
    R, n = 3, 65
    raw, scale, _, _ = _inputs(dtype, H, HKV, D)
    rows = raw[n - R:n]
    ref, ref_bytes = _reference(rows, H, HKV, D, scale)
    assert _same_bits(ref, rows)
    for nk in (n, torch.tensor([n], dtype=torch.int32, device=DEV)):
        wide, buf = _append(dtype, H, HKV, D, R, n, rotate=False, n_keys=nk, rope_delta=5)      # no table: the offset has nothing to move
        want_wide, want_buf = _expected(rows, n, rows, ref_bytes)
        assert _same_bits(wide, want_wide) and torch.equal(buf, want_buf)


def test_one_captured_graph_holds_a_whole_step():
    """advance(1), the append and the decode attention in ONE graph (one stream, no branches), replayed for three positions from 60
    keys: between the replays only the new raw qkv row is copied in."""
    from mquant_amd import ops
    from mquant_amd.kv_cache import Fp8KVCache
    H, HKV, D, dtype, n0 = 28, 4, 128, torch.float16, 60
    raw, scale, cos, sin = _inputs(dtype, H, HKV, D)
    kv = Fp8KVCache(1, CAP, HKV, D, [scale], cos, sin, DEV, dtype)
    cache = kv.caches[0]
    cache.view(torch.uint8)[:] = 0x7F                                 # nothing at or beyond n may matter
    pre, pre_bytes = _reference(raw[:n0], H, HKV, D, scale, cos[:n0], sin[:n0])
    kv.fill(0, pre[:, H * D:].view(n0, 2 * HKV, D))
    assert torch.equal(cache.view(torch.uint8)[:n0].reshape(n0, -1), pre_bytes)
    qkv = torch.zeros((1, (H + 2 * HKV) * D), dtype=dtype, device=DEV)
    out = torch.zeros((1, H * D), dtype=dtype, device=DEV)

    def one_step():
        kv.advance(1)
        kv.step(0, qkv, H, out=out)

    kv.set_length(n0)
    qkv.copy_(raw[n0:n0 + 1])
    one_step()                                                        # warm-up: the workspace and the scale check happen here
    kv.set_length(n0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_step()
    for t in (n0, n0 + 1, n0 + 2):                                    # the token this replay appends; n = t + 1 keys afterwards
        qkv.copy_(raw[t:t + 1])
        graph.replay()
        torch.cuda.synchronize()
        n = t + 1
        assert int(kv.n_keys.item()) == n
        ref, ref_bytes = _reference(raw[t:t + 1], H, HKV, D, scale, cos[t:t + 1], sin[t:t + 1])
        assert _same_bits(qkv, ref)
        bytes_now = cache.view(torch.uint8).reshape(CAP, -1)
        assert torch.equal(bytes_now[t:n], ref_bytes) and bool((bytes_now[n:] == 0x7F).all())
        q = ref[:, :H * D].clone().view(1, H, D)
        eager = ops.attn_decode_fp8kv(q, cache, scale, n_keys=kv.n_keys)
        assert torch.equal(out, eager)
        k, v = dequant_cache(cache[:n], scale)
        assert_within(out.clone(), *decode_reference(q, k, v, True), f"replay at n = {n}")


def test_the_cache_object_equals_the_ops_sequence():
    """Fp8KVCache, two layers: fill with 60 rows, then steps of 1, 1 and 2 rows -- cache contents and outputs of the ops-level
    sequence, and the last step once more through the fused-quantizer form."""
    from mquant_amd import ops
    from mquant_amd.kv_cache import Fp8KVCache
    H, HKV, D, dtype, n0 = 28, 4, 128, torch.bfloat16, 60
    raw0, scale0, cos, sin = _inputs(dtype, H, HKV, D)
    raws = [raw0, raw0.roll(5, dims=0).roll(64, dims=1)]
    scales = [scale0, (scale0 * 1.5).contiguous()]
    kv = Fp8KVCache(2, CAP, HKV, D, scales, cos, sin, DEV, dtype)
    mine = [torch.zeros((CAP, 2 * HKV, D), dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn) for _ in range(2)]
    nk = torch.zeros((1,), dtype=torch.int32, device=DEV)
    for layer in range(2):
        pre, _ = _reference(raws[layer][:n0], H, HKV, D, scales[layer], cos[:n0], sin[:n0])
        cols = pre[:, H * D:].view(n0, 2 * HKV, D)
        kv.fill(layer, cols)
        ops.kv_quant_fp8(cols, scales[layer], out=mine[layer][:n0])
    kv.set_length(n0)
    n = n0
    for R in (1, 1, 2):
        kv.advance(R)
        nk.fill_(n + R)
        for layer in range(2):
            a, b = raws[layer][n:n + R].clone(), raws[layer][n:n + R].clone()
            got = kv.step(layer, a, H)
            ops.kv_append_rope_fp8(b, H, mine[layer], scales[layer], cos, sin, n_keys=nk)
            want = ops.attn_decode_fp8kv(b[:, :H * D].view(R, H, D), mine[layer], scales[layer], n_keys=nk)
            assert _same_bits(a, b) and torch.equal(got, want) and got.shape == (R, H * D)
            assert torch.equal(kv.caches[layer].view(torch.uint8), mine[layer].view(torch.uint8))
        n += R
    assert int(kv.n_keys.item()) == 64 == n
    assert bool((kv.caches[0].view(torch.uint8)[64:] == 0).all()) and not torch.equal(kv.caches[0].view(torch.uint8), kv.caches[1].view(torch.uint8))
    # the same last step (rows 62, 63 again: the same bytes land in the same cache rows) with the next Linear's quantizer fused in
    s0 = float(want.float().abs().max()) / 127.0
    a, b = raws[1][62:64].clone(), raws[1][62:64].clone()
    got8 = kv.step_quant_i8(1, a, H, s0)
    ops.kv_append_rope_fp8(b, H, mine[1], scales[1], cos, sin, n_keys=nk)
    want8 = ops.attn_decode_quant_i8(b[:, :H * D].view(2, H, D), mine[1], scales[1], s0, n_keys=nk)
    assert torch.equal(got8, want8) and torch.equal(want8, ops.quantize_act_i8(want, s0)[0])
    assert torch.equal(kv.caches[1].view(torch.uint8), mine[1].view(torch.uint8))
