"""The generation step's append into a 16-bit cache (mq_kv_append_rope, csrc/kv_append.hip with KVB = 2; ops.kv_append_rope,
kv_cache.KVCache16) on the GPU, mirroring tests/test_gpu_kv_append.py.  The contract is bits: the Q and K columns of qkv receive
the bits of ``rope_inplace``, cache rows [n - R, n) the bits of those rotated K columns and then of the V columns -- nothing is
quantised -- so every comparison is exact and looks at WHOLE buffers: the sentinel columns behind qkv, its V columns, the padding
of the cache rows and every cache row outside [n - R, n) included.

Inputs as in tests/attn_decode_cases.make_case (gains 0.05 / 1 / 6 / 20 on the K / V heads) for any head_dim.  qkv sits in a wider
buffer (row stride = columns + 8), the cache is a slice of a wider buffer (row stride = 2 HKV D + 8 elements) pre-filled with a
canary.  The cache holds 96 rows throughout.  The cases of a property are walked inside one test; every assertion names its case."""
import functools

import pytest
import torch
import torch.nn.functional as F

from attn_decode_reference import decode_reference
from attn_reference import assert_within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
CAP = 96                    # cache rows
TABLE_ROWS = 104            # rows of cos / sin: a few more than the cache has, so that a small offset stays inside
SENTINEL = 7.0
CANARY = 0x7E5A             # as int16: a NaN in fp16, a large finite value in bf16; no input holds it
PAD = 8                     # elements of padding behind a cache row: rows stay 16-byte aligned
GEOMETRIES = [(28, 4, 128), (8, 8, 128), (4, 1, 128), (4, 2, 64), (2, 1, 16)]      # (28, 4, 128) at R = 8: nine workgroups


@functools.lru_cache(maxsize=None)
def _inputs(dtype, H, HKV, D):
    """(raw qkv [CAP, (H + 2 HKV) D], cos, sin [TABLE_ROWS, D]) made once per geometry and never written to"""
    from mquant_amd.full_prefill import _rope_tables
    g = torch.Generator(device=DEV).manual_seed(1000 * H + 10 * HKV + D)
    raw = (torch.randn(CAP, (H + 2 * HKV) * D, generator=g, device=DEV) * 0.8).to(dtype)
    gain = torch.tensor([0.05, 1.0, 6.0, 20.0] * HKV, device=DEV)[:2 * HKV].repeat_interleave(D)
    raw[:, H * D:] = (raw[:, H * D:].float() * gain).to(dtype)
    assert not bool((raw.view(torch.int16) == CANARY).any())
    cos, sin = _rope_tables(TABLE_ROWS, D, torch.device(DEV), dtype)
    return raw, cos[:, 0].contiguous(), sin[:, 0].contiguous()


def _buffers(rows, HKV, D):
    """(wide qkv buffer [R, cols + 8] holding `rows` and sentinels, its [R, cols] view, cache buffer [CAP, 2 HKV D + PAD] of canaries
    as int16, its cache view [CAP, 2 HKV, D] in rows' dtype)"""
    R, cols = rows.shape
    wide = torch.full((R, cols + 8), SENTINEL, dtype=rows.dtype, device=DEV)
    wide[:, :cols] = rows
    buf = torch.full((CAP, 2 * HKV * D + PAD), CANARY, dtype=torch.int16, device=DEV)
    cache = buf.view(rows.dtype)[:, :2 * HKV * D].unflatten(1, (2 * HKV, D))
    assert cache.data_ptr() == buf.data_ptr() and cache.stride() == (2 * HKV * D + PAD, D, 1)
    return wide, wide[:, :cols], buf, cache


def _reference(rows, H, HKV, D, cos_rows=None, sin_rows=None):
    """rope_inplace with one table row per qkv row: (rotated rows [R, cols], the cache rows' bits [R, 2 HKV D] as int16)"""
    from mquant_amd import ops
    ref = rows.clone()
    if cos_rows is not None:
        ops.rope_inplace(ref[:, :(H + HKV) * D], H + HKV, D, cos_rows.contiguous(), sin_rows.contiguous())
    return ref, ref[:, H * D:].contiguous().view(torch.int16)


def _expected(rows, n, ref, ref_bits):
    """the two whole buffers after an append of `rows` at key count n"""
    R, cols = rows.shape
    wide = torch.full((R, cols + 8), SENTINEL, dtype=rows.dtype, device=DEV)
    wide[:, :cols] = ref
    buf = torch.full((CAP, ref_bits.shape[1] + PAD), CANARY, dtype=torch.int16, device=DEV)
    buf[n - R:n, :ref_bits.shape[1]] = ref_bits
    return wide, buf


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _append(dtype, H, HKV, D, R, n_rows, rotate=True, **kw):
    """One call on fresh buffers with the raw rows [n_rows - R, n_rows): (wide, buf) afterwards."""
    from mquant_amd import ops
    raw, cos, sin = _inputs(dtype, H, HKV, D)
    wide, qkv, buf, cache = _buffers(raw[n_rows - R:n_rows], HKV, D)
    cos, sin = kw.pop("tables", (cos, sin) if rotate else (None, None))
    out = ops.kv_append_rope(qkv, H, cache, cos, sin, **kw)
    assert out is qkv
    return wide, buf


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_the_bits_of_rope_inplace_and_nothing_else_is_written(dtype):
    for H, HKV, D in GEOMETRIES:
        for R in (1, 3, 8):
            for n in (R, 65, 96):
                _bits(n, R, H, HKV, D, dtype)


def _bits(n, R, H, HKV, D, dtype):
    raw, cos, sin = _inputs(dtype, H, HKV, D)
    rows = raw[n - R:n]
    ref, ref_bits = _reference(rows, H, HKV, D, cos[n - R:n], sin[n - R:n])
    wide, buf = _append(dtype, H, HKV, D, R, n, n_keys=n)
    want_wide, want_buf = _expected(rows, n, ref, ref_bits)
    assert _same_bits(wide, want_wide)                                # Q and K rotated, V and the sentinels untouched
    assert torch.equal(buf, want_buf)                                 # rows [n - R, n) written, everything else still the canary
    assert _same_bits(wide[:, (H + HKV) * D:(H + 2 * HKV) * D], rows[:, (H + HKV) * D:])      # the V columns, said once more
    assert torch.equal(buf[n - R:n, HKV * D:2 * HKV * D], rows[:, (H + HKV) * D:].contiguous().view(torch.int16))     # V, not quantised
    if n > 1:
        assert not _same_bits(ref[:, :(H + HKV) * D], rows[:, :(H + HKV) * D])      # something was rotated


def test_a_key_count_on_the_device():
    """n_keys as a tensor: the bits of the host-n call; beyond the capacity it acts as the capacity, below R as R."""
    for dtype in DTYPES:
        for n_dev, acts_as in [("R", "R"), (40, 40), (96, 96), (9999, 96), (0, "R")]:
            _device_key_count(n_dev, acts_as, dtype)


def _device_key_count(n_dev, acts_as, dtype):
    H, HKV, D, R = 28, 4, 128, 3
    n_dev, n = (R if n_dev == "R" else n_dev), (R if acts_as == "R" else acts_as)
    nk = torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    wide, buf = _append(dtype, H, HKV, D, R, n, n_keys=nk)
    want_wide, want_buf = _append(dtype, H, HKV, D, R, n, n_keys=n)
    assert _same_bits(wide, want_wide) and torch.equal(buf, want_buf)
    assert int(nk.item()) == n_dev                                    # read, never written
    assert bool((buf[n - R:n, :2 * HKV * D] != CANARY).all()) and bool((buf[:n - R] == CANARY).all()) and bool((buf[n:] == CANARY).all())


def test_a_rope_position_offset():
    """Row r uses table row clamp(t + delta, 0, rows - 1): the host-side call on the table re-indexed that way.  (96, 6): rows 99,
    100, 101; (2, -1) at R = 2: rows 0 (clamped) and 0; +-1000 leave the table altogether."""
    for as_tensor in (True, False):
        for n, delta in [(40, 7), (40, -3), (96, 6), (40, 1000), (40, -1000), (2, -1)]:
            _position_offset(n, delta, as_tensor)


def _position_offset(n, delta, as_tensor):
    H, HKV, D, R, dtype = 4, 1, 128, 2 if n == 2 else 3, torch.float16
    raw, cos, sin = _inputs(dtype, H, HKV, D)
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


def test_append_only():
    """cos = sin = None: qkv keeps its bits, the cache rows are the K | V columns as they are."""
    for dtype in DTYPES:
        for H, HKV, D in [(28, 4, 128), (2, 1, 16)]:
            _append_only(H, HKV, D, dtype)
    _wrapper_wants_the_cache_in_qkvs_dtype()


def _append_only(H, HKV, D, dtype):
    R, n = 3, 65
    raw, _, _ = _inputs(dtype, H, HKV, D)
    rows = raw[n - R:n]
    ref, ref_bits = _reference(rows, H, HKV, D)
    assert _same_bits(ref, rows)
    for nk in (n, torch.tensor([n], dtype=torch.int32, device=DEV)):
        wide, buf = _append(dtype, H, HKV, D, R, n, rotate=False, n_keys=nk, rope_delta=5)      # no table: the offset has nothing to move
        want_wide, want_buf = _expected(rows, n, rows, ref_bits)
        assert _same_bits(wide, want_wide) and torch.equal(buf, want_buf)


def _wrapper_wants_the_cache_in_qkvs_dtype():
    from mquant_amd import ops
    qkv = torch.zeros((1, 6 * 128), dtype=torch.float16, device=DEV)
    for bad in (torch.zeros((8, 2, 128), dtype=torch.bfloat16, device=DEV),
                torch.zeros((8, 2, 128), dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)):
        with pytest.raises(AssertionError, match="kv_cache must have qkv's dtype"):
            ops.kv_append_rope(qkv, 4, bad)


# ---- rows beyond 2^31 bytes
LD_WIDE = 1 << 24           # elements: a 32 MiB row stride
WIDE_ROWS = 90


def test_an_append_beyond_2_gib():
    """A 90-row cache at a 32 MiB row stride (about 3 GiB): one row appended at row 89, 2.78 GiB from the base.  The bits are there,
    and the canaries in the row's padding, in the rows before and (in the buffer) behind it are untouched."""
    big = torch.empty(((WIDE_ROWS + 1) * LD_WIDE * 2,), dtype=torch.uint8, device=DEV)
    try:
        for dtype in DTYPES:
            _append_at_row_89(big, dtype)
    finally:
        del big
        torch.cuda.empty_cache()


def _append_at_row_89(big, dtype):
    from mquant_amd import ops
    H, HKV, D, n = 4, 2, 128, WIDE_ROWS
    raw, cos, sin = _inputs(dtype, H, HKV, D)
    row = 2 * HKV * D
    view = big.view(torch.int16)[:(WIDE_ROWS + 1) * LD_WIDE].view(WIDE_ROWS + 1, LD_WIDE)
    view[n - 2:n + 1, :row + 64] = CANARY
    cache = view[:n, :row].view(dtype).unflatten(1, (2 * HKV, D))
    assert cache.stride() == (LD_WIDE, D, 1) and cache[n - 1].data_ptr() - big.data_ptr() == (n - 1) * LD_WIDE * 2 > 1 << 31
    rows = raw[n - 1:n]
    ref, ref_bits = _reference(rows, H, HKV, D, cos[n - 1:n], sin[n - 1:n])
    for nk in (n, torch.tensor([n], dtype=torch.int32, device=DEV)):
        view[n - 1, :row] = CANARY
        qkv = rows.clone()
        ops.kv_append_rope(qkv, H, cache, cos, sin, n_keys=nk)
        assert _same_bits(qkv, ref)
        assert torch.equal(view[n - 1, :row], ref_bits[0])
        assert bool((view[n - 1, row:row + 64] == CANARY).all()) and bool((view[n - 2, :row + 64] == CANARY).all())
        assert bool((view[n, :row + 64] == CANARY).all())


# ---- a whole step
def _prefilled(dtype, H, HKV, D, n0):
    """(the rotated first n0 rows, their K | V columns [n0, 2 HKV, D])"""
    raw, cos, sin = _inputs(dtype, H, HKV, D)
    pre, _ = _reference(raw[:n0], H, HKV, D, cos[:n0], sin[:n0])
    return pre, pre[:, H * D:].view(n0, 2 * HKV, D)


def test_one_captured_graph_holds_a_whole_step():
    """A q|k|v projection (torch F.linear), the append and the decode attention in ONE graph (one stream, no branches), all three
    reading one n_keys; replayed for four positions from 60 keys, with only the hidden row copied in and n_keys incremented between
    the replays.  Cache bytes and outputs are those of the eager sequence."""
    from mquant_amd import ops
    H, HKV, D, dtype, n0, dim = 28, 4, 128, torch.float16, 60, 256
    raw, cos, sin = _inputs(dtype, H, HKV, D)
    g = torch.Generator(device=DEV).manual_seed(77)
    w = (torch.randn(((H + 2 * HKV) * D, dim), generator=g, device=DEV) * dim ** -0.5).to(dtype)
    hidden_all = torch.randn((8, dim), generator=g, device=DEV).to(dtype)
    _, kv_cols = _prefilled(dtype, H, HKV, D, n0)

    def fresh():
        cache = torch.full((CAP, 2 * HKV, D), float("nan"), dtype=dtype, device=DEV)      # nothing at or beyond n may matter
        cache[:n0] = kv_cols
        return cache, torch.tensor([n0], dtype=torch.int32, device=DEV)

    def step(hidden, cache, nk, out):
        nk.add_(1)
        qkv = F.linear(hidden, w)
        ops.kv_append_rope(qkv, H, cache, cos, sin, n_keys=nk)
        ops.attn_decode(qkv[:, :H * D].view(1, H, D), cache, n_keys=nk, out=out)

    eager_cache, eager_nk = fresh()
    eager_outs = []
    for t in range(4):
        out = torch.zeros((1, H * D), dtype=dtype, device=DEV)
        step(hidden_all[t:t + 1], eager_cache, eager_nk, out)
        eager_outs.append(out)

    cache, nk = fresh()
    hidden = hidden_all[4:5].clone()
    out = torch.zeros((1, H * D), dtype=dtype, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(hidden, cache, nk, out)                                  # warm-up: the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    cache[n0] = float("nan")
    nk.fill_(n0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(hidden, cache, nk, out)
    for t in range(4):
        hidden.copy_(hidden_all[t:t + 1])
        graph.replay()
        torch.cuda.synchronize()
        assert int(nk.item()) == n0 + t + 1
        assert _same_bits(out, eager_outs[t]), t
    assert _same_bits(cache[:n0 + 4], eager_cache[:n0 + 4]) and bool(torch.isnan(cache[n0 + 4:]).all())
    assert not _same_bits(eager_outs[0], eager_outs[3])
    q = F.linear(hidden_all[3:4], w)
    ops.rope_inplace(q[:, :H * D], H, D, cos[n0 + 3:n0 + 4].contiguous(), sin[n0 + 3:n0 + 4].contiguous())
    n = n0 + 4
    assert_within(out.clone(), *decode_reference(q[:, :H * D].view(1, H, D), cache[:n, :HKV], cache[:n, HKV:], True), f"replay at n = {n}")


def test_the_cache_object_equals_the_ops_sequence():
    """KVCache16, two layers: fill with 60 rows, then steps of 1, 1 and 2 rows -- cache contents and outputs of the ops-level
    sequence, and the last step once more through the fused-quantizer form."""
    from mquant_amd import KVCache16, ops
    H, HKV, D, dtype, n0 = 28, 4, 128, torch.bfloat16, 60
    raw0, cos, sin = _inputs(dtype, H, HKV, D)
    raws = [raw0, raw0.roll(5, dims=0).roll(64, dims=1)]
    kv = KVCache16(2, CAP, HKV, D, cos, sin, DEV, dtype)
    assert (kv.layers, kv.capacity, kv.kv_heads, kv.head_dim, kv.dtype, kv.rope_delta) == (2, CAP, HKV, D, dtype, None)
    assert all(c.shape == (CAP, 2 * HKV, D) and c.dtype == dtype and c.is_contiguous() for c in kv.caches)
    mine = [torch.zeros((CAP, 2 * HKV, D), dtype=dtype, device=DEV) for _ in range(2)]
    nk = torch.zeros((1,), dtype=torch.int32, device=DEV)
    for layer in range(2):
        pre, _ = _reference(raws[layer][:n0], H, HKV, D, cos[:n0], sin[:n0])
        cols = pre[:, H * D:].view(n0, 2 * HKV, D)                    # a strided view of the fused tensor
        kv.fill(layer, cols)
        mine[layer][:n0] = cols
    kv.set_length(n0)
    n = n0
    for R in (1, 1, 2):
        kv.advance(R)
        nk.fill_(n + R)
        for layer in range(2):
            a, b = raws[layer][n:n + R].clone(), raws[layer][n:n + R].clone()
            got = kv.step(layer, a, H)
            ops.kv_append_rope(b, H, mine[layer], cos, sin, n_keys=nk)
            want = ops.attn_decode(b[:, :H * D].view(R, H, D), mine[layer], n_keys=nk)
            assert _same_bits(a, b) and _same_bits(got, want) and got.shape == (R, H * D)
            assert _same_bits(kv.caches[layer], mine[layer])
        n += R
    assert int(kv.n_keys.item()) == 64 == n
    assert bool((kv.caches[0].view(torch.int16)[64:] == 0).all()) and not _same_bits(kv.caches[0], kv.caches[1])
    # the same last step (rows 62, 63 again: the same bits land in the same cache rows) with the next Linear's quantizer fused in
    s0 = float(want.float().abs().max()) / 127.0
    a, b = raws[1][62:64].clone(), raws[1][62:64].clone()
    got8 = kv.step_quant_i8(1, a, H, s0)
    ops.kv_append_rope(b, H, mine[1], cos, sin, n_keys=nk)
    want8 = ops.attn_decode_quant_i8(b[:, :H * D].view(2, H, D), mine[1], None, s0, n_keys=nk)
    assert torch.equal(got8, want8) and torch.equal(want8, ops.quantize_act_i8(want, s0)[0])
    assert _same_bits(kv.caches[1], mine[1])
    # a position offset set from the host reaches the append
    kv.set_rope_delta(3)
    kv.set_length(10)
    c = raws[0][9:10].clone()
    kv.step(0, c, H)
    ref, _ = _reference(raws[0][9:10], H, HKV, D, cos[12:13], sin[12:13])
    assert _same_bits(c, ref) and _same_bits(kv.caches[0][9], ref[0, H * D:].view(2 * HKV, D))
