"""Operands more than 2^31 and 2^32 bytes from their base, reached through ROW STRIDES: the 72B lm_head and embedding table are
2.49 GB, and the e4m3 cache kernels address rows with unsigned 32-bit buffer offsets up to their stated limit, (T + 32) x row
stride < 2^32 bytes.  One raw buffer of 4 GiB + 16 MiB is viewed with a 2 MiB, a 512 MiB or a 32 MiB row stride; each test writes
small operands into the view and compares BIT FOR BIT with the same call on compact tensors holding the same values -- no kernel's
arithmetic depends on a stride, so any difference is address arithmetic.  Only bytes a test wrote are ever read."""
import contextlib

import pytest
import torch

import attn_decode_cases as cases
import gemv_exact_cases as exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
BIG_BYTES = (4 << 30) + (16 << 20)
ROWS_2M, LD_2M = 2056, 1 << 20              # 2056 rows of 2^20 16-bit elements: rows >= 1024 start at or beyond 2^31 bytes, >= 2048 at 2^32
EDGE_ROWS = [1023, 1024, 2047, 2048, 2055]
ROWS_512M, LD_512M = 8, 1 << 28             # 8 rows 512 MiB apart: rows >= 4 lie beyond 2^31 bytes
POISON16 = -23131                           # 0xA5A5
H, HKV, D = 8, 2, 128
CAP, LD_CACHE = 95, 1 << 25                 # (95 + 32) 2^25 < 2^32: the largest cache of this stride the attention accepts
TABLE_ROWS = 104


@pytest.fixture(scope="module")
def big():
    buf = torch.empty((BIG_BYTES,), dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    yield buf
    del buf
    torch.cuda.empty_cache()


def bits(t):
    return t.contiguous().view(torch.int16)


def rows_2m(big, dtype):
    view = big.view(dtype).view(ROWS_2M, LD_2M)
    assert view.stride() == (LD_2M, 1) and view.data_ptr() == big.data_ptr()
    return view


def rows_512m(big, dtype):
    view = big.view(dtype)[:ROWS_512M * LD_512M].view(ROWS_512M, LD_512M)
    assert view.stride() == (LD_512M, 1) and view.data_ptr() == big.data_ptr()
    return view


# ---- 1. W with a 2 MiB row stride
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_gemv_reads_w_rows_beyond_2_and_4_gib(big, dtype):
    """the maximum of row m = 0 planted at each edge row in turn"""
    from mquant_amd import ops
    M, N, K = 3, ROWS_2M, 64
    w = rows_2m(big, dtype)[:, :K]
    assert w.stride() == (LD_2M, 1)
    for row in EDGE_ROWS:
        xi, wi = exact.draw(M, N, K)
        wi[row] = xi[0]                                               # |x[0]|^2
        want, want_tok = exact.expected(xi, wi, dtype)
        assert int(want_tok[0]) == row
        x, w_c = xi.to(dtype).to(DEV), wi.to(dtype).to(DEV)
        w.copy_(w_c)
        assert torch.equal(bits(w), bits(w_c))
        assert (w[row].data_ptr() - big.data_ptr() >= 1 << 31) == (row >= 1024)
        assert (w[row].data_ptr() - big.data_ptr() >= 1 << 32) == (row >= 2048)

        ref = ops.gemv_f16(x, w_c)
        got = ops.gemv_f16(x, w, out=torch.full((M, N), float("nan"), dtype=dtype, device=DEV))
        assert torch.equal(bits(got), bits(ref)) and exact.same_bits(got, want), row
        ref_tok = ops.gemv_f16_argmax(x, w_c)
        tok = ops.gemv_f16_argmax(x, w, token_out=torch.full((M,), -77, dtype=torch.int32, device=DEV))
        assert torch.equal(tok.cpu(), ref_tok.cpu()) and torch.equal(tok.cpu().long(), want_tok), row
        logits = torch.full((M, N), float("nan"), dtype=dtype, device=DEV)
        tok2 = ops.gemv_f16_argmax(x, w, logits=logits)
        assert torch.equal(bits(logits), bits(ref)) and torch.equal(tok2.cpu().long(), want_tok), row


# ---- 2. the embedding table with the same stride
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_embed_gather_reads_table_rows_beyond_2_and_4_gib(big, dtype):
    from mquant_amd import ops
    vocab, dim, log_rows = ROWS_2M, 2056, 16                          # 257 chunks: two workgroups per row
    ids = [0, 1023, 1024, 2047, 2048, 2055]
    g = torch.Generator(device=DEV).manual_seed(vocab + dim)
    table_c = torch.randn((vocab, dim), generator=g, device=DEV).to(dtype)
    table = rows_2m(big, dtype)[:, :dim]
    table.copy_(table_c)
    assert torch.equal(bits(table), bits(table_c))
    ids_dev = torch.tensor(ids, dtype=torch.int32, device=DEV)
    n_keys = torch.tensor([11], dtype=torch.int32, device=DEV)
    res = []
    for t in (table, table_c):
        out = torch.full((len(ids), dim + 8), 7.0, dtype=dtype, device=DEV)
        log = torch.full((log_rows,), -77, dtype=torch.int32, device=DEV)
        ops.embed_gather(t, ids_dev, out=out[:, :dim], id_log=log, n_keys=n_keys)
        res.append((out, log))
    (out, log), (out_c, log_c) = res
    assert torch.equal(bits(out), bits(out_c)) and torch.equal(log, log_c)
    assert torch.equal(bits(out[:, :dim]), bits(table_c[ids])) and bool((out[:, dim:] == 7.0).all())
    assert log.cpu().tolist() == [-77] * 5 + ids + [-77] * 5


# ---- 3. output rows 512 MiB apart
def _poison_rows(view, cols):
    """poison over the columns the call writes and the 64 bytes directly behind them"""
    view.view(torch.int16)[:, :cols + 32] = POISON16


def _poison_survived(view, cols):
    return bool((view.view(torch.int16)[:, cols:cols + 32] == POISON16).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_gemv_writes_logits_rows_512_mib_apart(big, dtype):
    from mquant_amd import ops
    M, N, K = 8, 1001, 64
    x, w, want, want_tok = exact.case(dtype, M, N, K)
    x, w = x.to(DEV), w.to(DEV)
    view = rows_512m(big, dtype)
    logits = view[:, :N]
    assert logits[4].data_ptr() - big.data_ptr() == 1 << 31
    ref = ops.gemv_f16(x, w)
    assert exact.same_bits(ref, want)

    _poison_rows(view, N)
    ops.gemv_f16(x, w, out=logits)
    assert torch.equal(bits(logits), bits(ref)) and _poison_survived(view, N)
    _poison_rows(view, N)
    tok = ops.gemv_f16_argmax(x, w, logits=logits)
    assert torch.equal(bits(logits), bits(ref)) and _poison_survived(view, N)
    assert torch.equal(tok.cpu().long(), want_tok)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_embed_gather_writes_rows_512_mib_apart(big, dtype):
    from mquant_amd import ops
    vocab, dim, R = 37, 2056, 8
    g = torch.Generator(device=DEV).manual_seed(vocab + dim)
    table = torch.randn((vocab, dim), generator=g, device=DEV).to(dtype)
    ids = [36, 0, 17, 5, 30, 1, 22, 9]
    ids_dev = torch.tensor(ids, dtype=torch.int32, device=DEV)
    view = rows_512m(big, dtype)
    out = view[:, :dim]
    _poison_rows(view, dim)
    ops.embed_gather(table, ids_dev, out=out)
    ref = ops.embed_gather(table, ids_dev)
    assert torch.equal(bits(out), bits(ref)) and torch.equal(bits(out), bits(table[ids]))
    assert _poison_survived(view, dim)


# ---- 4. the e4m3 cache with a 32 MiB row stride
@contextlib.contextmanager
def forced(plan):
    from mquant_amd import ops
    ops.attn_decode_debug_force(*plan)
    try:
        yield
    finally:
        ops.attn_decode_debug_force(0, 0)


def wide_cache(big, rows):
    """(byte view [rows, 2^25], its e4m3 cache [rows, 2 HKV, D])"""
    view = big[:rows * LD_CACHE].view(rows, LD_CACHE)
    cache = view[:, :2 * HKV * D].view(torch.float8_e4m3fn).unflatten(1, (2 * HKV, D))
    assert cache.data_ptr() == big.data_ptr() and cache.stride() == (LD_CACHE, D, 1)
    return view, cache


def _count(n, on_device):
    return torch.tensor([n], dtype=torch.int32, device=DEV) if on_device else n


def _sequence(cache, qkv, q, scale, cos, sin):
    """fill rows [0, 92), append three rows at n = 95 (host count, then device count), decode at n = 65 and 95 under three plans
    with both counts, prefill over all 95 rows -> every result by name"""
    from mquant_amd import ops
    res = {}
    kv = qkv[:, H * D:].view(CAP, 2 * HKV, D)
    raw = cache.view(torch.uint8)
    ops.kv_quant_fp8(kv[:92], scale, out=cache[:92])
    for on_device in (False, True):
        raw[92:] = 0x7F
        rows = qkv[92:].clone()
        ops.kv_append_rope_fp8(rows, H, cache, scale, cos, sin, n_keys=_count(CAP, on_device))
        res[f"appended qkv rows, device count {on_device}"] = rows.view(torch.int16)
        res[f"cache after the append, device count {on_device}"] = raw.clone()
    for n in (65, CAP):
        for plan in [(0, 0), (1, 0), (3, 0)]:
            for on_device in (False, True):
                with forced(plan):
                    o = ops.attn_decode_fp8kv(q[n - 3:n], cache, scale, n_keys=_count(n, on_device))
                res[f"decode n {n} plan {plan} device count {on_device}"] = o.view(torch.int16)
        res[f"decode to int8 n {n}"] = ops.attn_decode_quant_i8(q[n - 3:n], cache, scale, 0.05, n_keys=n)
    res["prefill"] = ops.attn_prefill_fp8kv(q, cache, scale).view(torch.int16)
    res["prefill to int8"] = ops.attn_prefill_quant_i8(q, 0.05, kv_cache=cache, kv_scale=scale)
    return res


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_the_cache_kernels_at_a_32_mib_row_stride(big, dtype):
    from mquant_amd import ops
    from mquant_amd.full_prefill import _rope_tables
    qkv, q, cache_all, scale = cases.make_case(CAP + H, CAP, H, HKV, dtype, DEV)
    cos, sin = _rope_tables(TABLE_ROWS, D, torch.device(DEV), dtype)
    cos, sin = cos[:, 0].contiguous(), sin[:, 0].contiguous()
    row_bytes = 2 * HKV * D

    view, cache = wide_cache(big, CAP)
    assert cache[64].data_ptr() - big.data_ptr() == 1 << 31
    view[:, :row_bytes + 64] = 0x7F                                   # an e4m3 NaN in every cache byte, and 64 bytes of poison behind
    got = _sequence(cache, qkv, q, scale, cos, sin)
    compact = torch.full((CAP, 2 * HKV, D), 0x7F, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    want = _sequence(compact, qkv, q, scale, cos, sin)
    assert list(got) == list(want) and len(got) == 4 + 2 * (3 * 2 + 1) + 2
    for name in got:
        assert got[name].shape == want[name].shape and torch.equal(got[name], want[name]), name
    assert torch.equal(cache.view(torch.uint8), compact.view(torch.uint8))
    assert bool((view[:, row_bytes:row_bytes + 64] == 0x7F).all())

    # the sequence itself, against the two entry points the append promises the bits of
    assert torch.equal(compact.view(torch.uint8)[:92], cache_all.view(torch.uint8)[:92])
    ref = qkv[92:].clone()
    ops.rope_inplace(ref[:, :(H + HKV) * D], H + HKV, D, cos[92:CAP].contiguous(), sin[92:CAP].contiguous())
    ref8 = ops.kv_quant_fp8(ref[:, H * D:].view(3, 2 * HKV, D), scale)
    for on_device in (False, True):
        assert torch.equal(got[f"appended qkv rows, device count {on_device}"], ref.view(torch.int16))
        assert torch.equal(got[f"cache after the append, device count {on_device}"][92:], ref8.view(torch.uint8))
    # and a result cannot be the same for every key count or plan by accident of being empty
    assert not torch.equal(got["decode n 65 plan (1, 0) device count False"], got[f"decode n {CAP} plan (1, 0) device count False"])


def test_one_more_row_reaches_4_gib_and_is_refused(big):
    from mquant_amd import ops
    from mquant_amd._lib import MQuantHipError
    rows = CAP + 1
    assert (rows + 32) * LD_CACHE == 1 << 32
    _, cache = wide_cache(big, rows)
    q = torch.zeros((rows, H, D), dtype=torch.float16, device=DEV)
    scale = torch.ones((2 * HKV,), dtype=torch.float32, device=DEV)
    out3 = torch.full((3, H * D), 7.0, dtype=torch.float16, device=DEV)
    out = torch.full((rows, H * D), 7.0, dtype=torch.float16, device=DEV)
    for on_device in (False, True):
        with pytest.raises(MQuantHipError, match=r"mq_attn_decode_fp8kv failed \(status -1\): .*must stay below 4 GiB"):
            ops.attn_decode_fp8kv(q[rows - 3:], cache, scale, n_keys=_count(rows, on_device), out=out3)
    with pytest.raises(MQuantHipError, match=r"mq_attn_decode_fp8kv_quant_i8 failed \(status -1\): .*must stay below 4 GiB"):
        ops.attn_decode_quant_i8(q[rows - 3:], cache, scale, 0.05, n_keys=rows)
    with pytest.raises(MQuantHipError, match=r"mq_attn_prefill_fp8kv failed \(status -1\): .*must stay below 4 GiB"):
        ops.attn_prefill_fp8kv(q, cache, scale, out=out)
    with pytest.raises(MQuantHipError, match=r"mq_attn_prefill_quant_i8 failed \(status -1\): .*must stay below 4 GiB"):
        ops.attn_prefill_quant_i8(q, 0.05, kv_cache=cache, kv_scale=scale)
    assert bool((out3 == 7.0).all()) and bool((out == 7.0).all())      # nothing was launched
