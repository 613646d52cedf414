"""Prefill attention at head dimensions 64 (InternViT-300M, InternVL2's vision tower: 16 heads, 1025 tokens with the class
token) and 104 (Qwen-VL's ViT: 16 heads, 1024 tokens), 16-bit K / V (``mq_attn_prefill`` and the 16-bit form of
``mq_attn_prefill_quant_i8``; mquant_amd/csrc/attn_prefill.hip).

64 has its own tile geometry, loader and V swizzle.  104 is no multiple of the first GEMM's k-step: the kernel contracts
over 112 with zeros it supplies itself on BOTH sides (the q operand of d 104 .. 111 is never loaded, the K tile's pad columns
are zeroed in LDS), and stores 104 columns.  The padding adds exact zeros, so the checker -- float64 softmax attention with a
bound for every output element, tests/attn_reference.py, generic in D -- is used unchanged, with no tolerance of its own
here.  What the padding could break is checked bit for bit: nothing outside a head's own D columns may reach it, neither
another head's q / K / V (NaN and Inf included: 0 x NaN = NaN) nor whatever follows the last V head in a wider allocation.
The e4m3 cache stays at 128, and every other width stays refused."""
import pytest
import torch
import torch.nn.functional as F

from attn_reference import assert_within, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
HOOKS = (0, 2, 4, 5)        # mq_attn_debug_waves: by shape, 2 waves, 4 waves with paired shallow tiles, 4 waves unpaired
DIMS = (64, 104)
DTYPES = (torch.float16, torch.bfloat16)


def _qkv(seed, T, H, HKV, D, dtype, extra_cols=0, fill=float("nan")):
    """One [T, (H + 2 HKV) D] tensor whose column slices are q, k and v, read in place; per-head K / V gains that differ by
    more than 100x.  extra_cols > 0: the tensor is itself a column slice of a wider allocation whose remaining columns --
    right after the last V head -- hold ``fill``."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    W = (H + 2 * HKV) * D
    src = torch.randn(T, W, generator=g, device=DEV) * 0.8
    gain = torch.tensor([0.05, 1.0, 6.0, 20.0] * HKV, device=DEV)[:2 * HKV].repeat_interleave(D)
    src[:, H * D:] *= gain
    if not extra_cols:
        return src.to(dtype)
    big = torch.full((T, W + extra_cols), fill, device=DEV, dtype=dtype)
    big[:, :W] = src.to(dtype)
    return big[:, :W]


def _split(qkv, H, HKV, D):
    T = qkv.shape[0]
    return (qkv[:, :H * D].view(T, H, D), qkv[:, H * D:(H + HKV) * D].view(T, HKV, D),
            qkv[:, (H + HKV) * D:(H + 2 * HKV) * D].view(T, HKV, D))


def _hooks():
    from mquant_amd._lib import call

    class _Hooks:
        def __iter__(self):
            for hook in HOOKS:
                call("mq_attn_debug_waves", hook)
                yield hook

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            call("mq_attn_debug_waves", 0)
    return _Hooks()


SHAPES = [(1, 2, 2, False), (33, 8, 8, True), (97, 8, 2, True), (161, 8, 2, True), (333, 8, 8, False)]
TOWER = {64: (1025, 16, 16, False), 104: (1024, 16, 16, False)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,T,H,HKV,causal", [(D,) + s for D in DIMS for s in SHAPES + [TOWER[D]]])
def test_every_element_within_its_bound(dtype, D, T, H, HKV, causal):
    """A single token, one key into the second block, GQA, an odd number of tiles with the paired shallow half, a ragged
    non-causal T and the tower's own shape (528 / 512 workgroups), through every launch form; one reference per case."""
    from mquant_amd import ops
    qkv = _qkv(T + 3 * H + D, T, H, HKV, D, dtype)
    q, k, v = _split(qkv, H, HKV, D)
    want, bound = reference(q, k, v, causal)
    with _hooks() as hooks:
        for hook in hooks:
            got = ops.attn_prefill(q, k, v, causal=causal)
            assert got.shape == (T, H * D) and got.dtype == q.dtype
            assert_within(got, want, bound, f"D={D} T={T} H={H} HKV={HKV} causal={causal} hook={hook}")


_BAD = (float("nan"), float("inf"), float("-inf"))


def _overwrite(cols, mode, seed):
    """other finite values, or NaN / +Inf / -Inf patterns, in place"""
    if mode == "finite":
        g = torch.Generator(device=DEV).manual_seed(seed)
        cols.copy_((torch.randn(cols.shape, generator=g, device=DEV) * 3.0).to(cols.dtype))
    else:
        idx = (torch.arange(cols.numel(), device=DEV) + seed) % 3
        cols.copy_(torch.tensor(_BAD, device=DEV)[idx].view(cols.shape).to(cols.dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("group", [1, 4])
@pytest.mark.parametrize("extra_cols", [0, 64])
def test_nothing_outside_a_heads_own_columns_reaches_it(dtype, D, group, extra_cols):
    """Overwrite q of every head but h and K / V of every kv head but h's -- with other finite values, then with NaN and
    +-Inf -- and head h's output columns keep their bits.  extra_cols: q|k|v is a column slice of a wider allocation with
    NaN right after the last V head, exactly where a loaded pad of the last kv head would read."""
    from mquant_amd import ops
    T, HKV = 161, 2
    H = HKV * group
    qkv = _qkv(T + group + D, T, H, HKV, D, dtype, extra_cols)
    q, k, v = _split(qkv, H, HKV, D)
    with _hooks() as hooks:
        for hook in hooks:
            for causal in (True, False):
                base = ops.attn_prefill(q, k, v, causal=causal)
                assert bool(torch.isfinite(base).all()), (hook, causal)
                for h in sorted({0, H // 2, H - 1}):
                    g = h // group
                    cols = slice(h * D, (h + 1) * D)
                    for mode in ("finite", "nonfinite"):
                        big = qkv._base.clone() if extra_cols else qkv.clone()
                        qkv2 = big[:, :qkv.shape[1]]
                        for x in range(H):
                            if x != h:
                                _overwrite(qkv2[:, x * D:(x + 1) * D], mode, 7 * x + h)
                        for x in range(HKV):
                            if x != g:
                                _overwrite(qkv2[:, (H + x) * D:(H + x + 1) * D], mode, 11 * x + h)
                                _overwrite(qkv2[:, (H + HKV + x) * D:(H + HKV + x + 1) * D], mode, 13 * x + h)
                        q2, k2, v2 = _split(qkv2, H, HKV, D)
                        got = ops.attn_prefill(q2, k2, v2, causal=causal)
                        assert torch.equal(got[:, cols], base[:, cols]), (hook, causal, h, mode)
                        assert not torch.equal(got.view(torch.int16), base.view(torch.int16)), (hook, causal, h, mode)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("T", [33, 65, 161])
def test_future_keys_cannot_change_a_row(dtype, D, T):
    """Causal: overwrite K and V of every key after t0 with other finite values; rows <= t0 keep their bits, in the 16-bit
    output and in the fused int8 store, and rows > t0 change."""
    from mquant_amd import ops
    H, HKV = 8, 2                                                      # 512 / 832 int8 columns: whole 64-column groups
    qkv = _qkv(T * 7 + D, T, H, HKV, D, dtype)
    q, k, v = _split(qkv, H, HKV, D)
    sel = (torch.arange(T, device=DEV) % 3 == 1).to(torch.uint8)
    n = (T + 31) // 32
    deep_from = (n - n // 2) * 32                                      # first row of the deep half of the tiles
    t0s = sorted({t for t in (0, 31, 32, deep_from - 1, T - 2) if 0 <= t <= T - 2})
    with _hooks() as hooks:
        for hook in hooks:
            base = ops.attn_prefill(q, k, v, causal=True)
            s0 = float(base.float().abs().max()) / 127.0 * 0.8
            base_i8 = ops.attn_prefill_quant_i8(q, s0, 0.5 * s0, k=k, v=v, causal=True, row_sel=sel)
            for t0 in t0s:
                qkv2 = qkv.clone()
                qkv2[t0 + 1:, H * D:] *= 8
                q2, k2, v2 = _split(qkv2, H, HKV, D)
                got = ops.attn_prefill(q2, k2, v2, causal=True)
                assert torch.equal(got[:t0 + 1], base[:t0 + 1]), (hook, t0)
                assert not torch.equal(got[t0 + 1:], base[t0 + 1:]), (hook, t0)
                got_i8 = ops.attn_prefill_quant_i8(q2, s0, 0.5 * s0, k=k2, v=v2, causal=True, row_sel=sel)
                assert torch.equal(got_i8[:t0 + 1], base_i8[:t0 + 1]), (hook, t0)
                assert not torch.equal(got_i8[t0 + 1:], base_i8[t0 + 1:]), (hook, t0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("T", [97, 333])
@pytest.mark.parametrize("tiled", [True, False])
def test_fused_int8_store_equals_attention_then_quantize(dtype, D, T, tiled):
    """mq_attn_prefill_quant_i8 writes the bytes mq_quantize_act_i8 makes of the 16-bit attention output: two scales
    selected per row, levels spread with some clamped, row-major and tiled destinations, causal and not."""
    from mquant_amd import ops
    H, HKV = 8, 2
    qkv = _qkv(T + H + D, T, H, HKV, D, dtype)
    q, k, v = _split(qkv, H, HKV, D)
    sel = (torch.arange(T, device=DEV) % 3 == 1).to(torch.uint8)
    with _hooks() as hooks:
        for hook in hooks:
            for causal in (True, False):
                o = ops.attn_prefill(q, k, v, causal=causal)
                s0 = float(o.float().abs().max()) / 127.0 * 0.8          # some rows saturate
                s1 = 0.37 * s0
                want, _ = ops.quantize_act_i8(o, s0, s1, row_sel=sel, tiled=tiled)
                got = ops.attn_prefill_quant_i8(q, s0, s1, k=k, v=v, causal=causal, row_sel=sel, tiled=tiled)
                a = got.to_rows() if tiled else got
                b = want.to_rows() if tiled else want
                # the stand-alone quantizer pads its columns to a multiple of 128 with zeros (832 -> 896); the fused store
                # holds exactly heads * D
                assert a.shape == (T, H * D) and b.shape == (T, (H * D + 127) // 128 * 128)
                assert torch.equal(a, b[:, :H * D]), (hook, causal)
                assert not bool(b[:, H * D:].any())
                assert int(a.abs().max()) >= 127


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", DIMS)
def test_output_guard_and_strides(dtype, D):
    """out as a column slice of a wider sentinel-filled tensor: the slice equals the contiguous result and every sentinel
    survives.  q with a row stride of its own (a contiguous copy, k / v still slices of the fused tensor) is served, as at
    128: q and K / V carry separate strides."""
    from mquant_amd import ops
    T, H, HKV = 200, 8, 2
    qkv = _qkv(T + D, T, H, HKV, D, dtype)
    q, k, v = _split(qkv, H, HKV, D)
    with _hooks() as hooks:
        for hook in hooks:
            for causal in (True, False):
                want = ops.attn_prefill(q, k, v, causal=causal)
                wide = torch.full((T + 32, H * D + 64), 7.0, device=DEV, dtype=dtype)
                ops.attn_prefill(q, k, v, causal=causal, out=wide[:T, :H * D])
                assert torch.equal(wide[:T, :H * D], want), (hook, causal)
                wide[:T, :H * D] = 7.0
                assert bool((wide == 7.0).all()), (hook, causal)
                qc = q.contiguous()
                assert qc.stride(0) != k.stride(0)
                assert torch.equal(ops.attn_prefill(qc, k, v, causal=causal), want), (hook, causal)
                s0 = float(want.float().abs().max()) / 127.0 * 0.8
                want_i8 = ops.attn_prefill_quant_i8(q, s0, k=k, v=v, causal=causal)
                bi = torch.full((T + 32, H * D + 64), 99, device=DEV, dtype=torch.int8)
                ops.attn_prefill_quant_i8(q, s0, k=k, v=v, causal=causal, out=bi[:T, :H * D])
                assert torch.equal(bi[:T, :H * D], want_i8), (hook, causal)
                bi[:T, :H * D] = 99
                assert bool((bi == 99).all()), (hook, causal)


def test_refusals_that_stay():
    from mquant_amd import ops
    from mquant_amd._lib import MQuantHipError
    T, H, HKV = 16, 4, 2
    for D in (48, 96, 112):
        q, k, v = _split(_qkv(D, T, H, HKV, D, torch.float16), H, HKV, D)
        with pytest.raises(MQuantHipError, match="head_dim"):
            ops.attn_prefill(q, k, v)
        with pytest.raises(MQuantHipError, match="head_dim"):
            ops.attn_prefill_quant_i8(q, 0.1, k=k, v=v, out=torch.empty(T, 64 * ((H * D + 63) // 64), device=DEV, dtype=torch.int8))
    # the e4m3 cache stays at 128
    q = torch.randn(T, H, 64, device=DEV, dtype=torch.float16)
    cache = torch.zeros(T, 2 * HKV, 64, device=DEV, dtype=torch.float8_e4m3fn)
    scale = torch.ones(2 * HKV, device=DEV)
    with pytest.raises((MQuantHipError, AssertionError)):
        ops.attn_prefill_fp8kv(q, cache, scale)
    with pytest.raises((MQuantHipError, AssertionError)):
        ops.attn_prefill_quant_i8(q, 0.1, kv_cache=cache, kv_scale=scale)
    # 4 heads of 104 = 416 columns: no whole 64-column groups for the int8 layout
    q, k, v = _split(_qkv(5, T, 4, 2, 104, torch.float16), 4, 2, 104)
    with pytest.raises(MQuantHipError, match="out must hold exactly heads \\* head_dim"):
        ops.attn_prefill_quant_i8(q, 0.1, k=k, v=v)


@pytest.mark.parametrize("D", DIMS)
def test_it_agrees_with_sdpa_in_half_precision(D):
    """The path it replaces at the two towers: permutes to [1, H, T, D], torch SDPA, permutes back."""
    from mquant_amd import ops
    T, H, HKV, causal = TOWER[D]
    qkv = _qkv(11 + D, T, H, HKV, D, torch.float16)
    q, k, v = _split(qkv, H, HKV, D)
    got = ops.attn_prefill(q, k, v, causal=causal).float()
    o = F.scaled_dot_product_attention(q.permute(1, 0, 2)[None], k.permute(1, 0, 2)[None], v.permute(1, 0, 2)[None],
                                       is_causal=causal)
    o = o[0].permute(1, 0, 2).reshape(T, H * D).float()
    assert float((got - o).abs().max() / o.abs().max()) < 5e-3       # two fp16 pipelines, each ~1e-3 from the exact result
    assert float(F.cosine_similarity(got.flatten(), o.flatten(), dim=0)) > 0.999999
