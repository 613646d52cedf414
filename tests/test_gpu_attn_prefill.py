"""Prefill attention that reads the e4m3 KV cache directly (``mq_attn_prefill_fp8kv``).  The reference
has no attention kernel and no cache quantizer: PARITY UNPINNED.  The checker (tests/attn_reference.py) is softmax
attention in float64 over the DEQUANTISED cache (value * per-head scale), which is what dequantise-on-read followed by SDPA
computes; the kernel multiplies the e4m3 values themselves and folds the scales into the score / output scale, so the two
differ by floating-point rounding only (P and the output are rounded to q's dtype, accumulation is fp32) -- held to a
bound for EVERY output element, derived from those roundings.  Properties that hold bit for bit (causality, head
isolation, nothing read past T or written outside the output, scale folding, the e4m3 decode) are checked with no
tolerance at all."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from attn_reference import assert_within, dequant_cache, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
HOOKS = (0, 2, 4, 5)        # mq_attn_debug_waves: by shape, 2 waves, 4 waves with paired shallow tiles, 4 waves unpaired
_RATIOS = {}                # dtype -> largest error / bound seen (printed at the end with MQ_ATTN_BOUND_REPORT=1)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if os.environ.get("MQ_ATTN_BOUND_REPORT"):
        for k, (r, what) in sorted(_RATIOS.items()):
            print(f"\nlargest error / bound, {k}: {r:.3f} ({what})")


def _within(got, o, bound, what):
    """every element within its bound (tests/attn_reference.py)"""
    r = assert_within(got, o, bound, what)
    key = str(got.dtype).replace("torch.", "")
    if r > _RATIOS.get(key, (-1.0, None))[0]:
        _RATIOS[key] = (r, what)
    return r


def _case(seed, T, H, HKV, dtype, q_gain=1.0):
    from mquant_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    D = 128
    qkv = (torch.randn(T, (H + 2 * HKV) * D, generator=g, device=DEV) * 0.8).to(dtype)
    qkv[:, :H * D] *= q_gain
    # per-head magnitudes differ by > 100x: a scale that is wrong for one head shows immediately
    gain = torch.tensor([0.05, 1.0, 6.0, 20.0] * HKV, device=DEV)[:2 * HKV].repeat_interleave(D)
    qkv[:, H * D:] = (qkv[:, H * D:].float() * gain).to(dtype)
    q = qkv[:, :H * D].view(T, H, D)                                   # column slices of the fused output, read in place
    kv = qkv[:, H * D:].view(T, 2 * HKV, D)
    scale = ops.kv_scale_from_absmax(kv)
    cache = ops.kv_quant_fp8(kv, scale)
    return q, cache, scale


def _ref(q, cache, scale, causal, softmax_scale=None):
    """float64 softmax attention over the dequantised cache -> (o, bound) [T, H * D]"""
    return reference(q, *dequant_cache(cache, scale), causal, softmax_scale)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("T,H,HKV,causal", [(768, 28, 4, True), (768, 64, 8, True), (1, 4, 2, True), (33, 8, 8, True),
                                            (129, 4, 1, True), (500, 8, 2, False), (2048, 8, 2, True),
                                            (4096, 28, 4, True)])
def test_attention_over_the_fp8_cache_equals_attention_over_the_dequantised_cache(dtype, T, H, HKV, causal):
    from mquant_amd import ops
    q, cache, scale = _case(T + H, T, H, HKV, dtype)
    got = ops.attn_prefill_fp8kv(q, cache, scale, causal=causal)
    assert got.shape == (T, H * 128) and got.dtype == dtype
    want, bound = _ref(q, cache, scale, causal)
    _within(got, want, bound, f"e4m3 T={T} H={H} HKV={HKV} causal={causal}")
    err = (got.double() - want).abs()
    # per head: the rounding of P and of the output to 10 (fp16) / 7 (bf16) mantissa bits, relative to the head's range
    tol = 2.5e-3 if dtype == torch.float16 else 1.6e-2
    per_head = want.view(T, H, 128).abs().amax(dim=(0, 2)).clamp_min(1e-9)
    rel = err.view(T, H, 128).amax(dim=(0, 2)) / per_head
    assert float(rel.max()) < tol, rel.cpu().numpy()
    cos = F.cosine_similarity(got.double().flatten(), want.flatten(), dim=0)
    assert float(cos) > (0.999999 if dtype == torch.float16 else 0.99995)


def test_peaked_scores_and_the_first_rows():
    """Large logits (one key dominates), and the causal rows 0 and 1 that attend to one and two keys."""
    from mquant_amd import ops
    T, H, HKV = 300, 4, 2
    q, cache, scale = _case(5, T, H, HKV, torch.float16, q_gain=6.0)
    got16 = ops.attn_prefill_fp8kv(q, cache, scale, causal=True)
    got = got16.double()
    want, bound = _ref(q, cache, scale, True)
    _within(got16, want, bound, "peaked scores")
    assert torch.isfinite(got).all()
    v0 = cache.float().double()[0, HKV:] * scale.double()[HKV:, None]   # row 0 attends to key 0 only: O = V[0]
    np.testing.assert_allclose(got[0].view(H, 128).cpu().numpy(), v0.repeat_interleave(H // HKV, dim=0).cpu().numpy(),
                               rtol=2 ** -10, atol=1e-6)
    per_head = want.view(T, H, 128).abs().amax(dim=(0, 2))
    rel = (got - want).abs().view(T, H, 128).amax(dim=(0, 2)) / per_head
    assert float(rel.max()) < 4e-3, rel


def test_it_agrees_with_dequantise_then_sdpa_in_half_precision():
    """The path it replaces: mq_kv_dequant_fp8 -> fp16 K / V in HBM -> torch SDPA."""
    from mquant_amd import ops
    T, H, HKV = 768, 28, 4
    q, cache, scale = _case(11, T, H, HKV, torch.float16)
    got = ops.attn_prefill_fp8kv(q, cache, scale, causal=True).float()
    kvd = ops.kv_dequant_fp8(cache, scale, torch.float16)
    k, v = kvd[:, :HKV], kvd[:, HKV:]
    rep = H // HKV
    o = F.scaled_dot_product_attention(q.permute(1, 0, 2)[None], k.repeat_interleave(rep, 1).permute(1, 0, 2)[None],
                                       v.repeat_interleave(rep, 1).permute(1, 0, 2)[None], is_causal=True)
    o = o[0].permute(1, 0, 2).reshape(T, H * 128).float()
    assert float((got - o).abs().max() / o.abs().max()) < 5e-3       # two fp16 pipelines, each ~1e-3 from the exact result
    assert float(F.cosine_similarity(got.flatten(), o.flatten(), dim=0)) > 0.999999


def test_out_buffer_and_strides():
    from mquant_amd import ops
    T, H, HKV = 200, 8, 2
    q, cache, scale = _case(2, T, H, HKV, torch.float16)
    wide = torch.full((T, H * 128 + 64), 7.0, device=DEV, dtype=torch.float16)
    ops.attn_prefill_fp8kv(q, cache, scale, out=wide[:, :H * 128])
    want = ops.attn_prefill_fp8kv(q.contiguous(), cache, scale)
    assert torch.equal(wide[:, :H * 128], want) and bool((wide[:, H * 128:] == 7.0).all())


def test_bad_arguments_are_refused():
    from mquant_amd import ops
    from mquant_amd._lib import MQuantHipError as MQuantError
    q, cache, scale = _case(1, 16, 4, 2, torch.float16)
    with pytest.raises((MQuantError, AssertionError)):
        ops.attn_prefill_fp8kv(q.float(), cache, scale)
    with pytest.raises((MQuantError, AssertionError)):
        ops.attn_prefill_fp8kv(q[:, :, :64].contiguous(), cache[:, :, :64].contiguous(), scale)
    with pytest.raises((MQuantError, AssertionError)):
        ops.attn_prefill_fp8kv(q[:, :3].contiguous(), cache, scale)     # 3 heads over 2 kv heads


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("T,H,HKV,causal,D", [(768, 28, 4, True, 128), (768, 64, 8, True, 128), (1, 4, 2, True, 128),
                                              (97, 8, 8, True, 128), (500, 8, 2, False, 128), (1500, 4, 1, True, 128),
                                              (1024, 16, 16, False, 80), (333, 4, 4, False, 80), (200, 6, 2, True, 80),
                                              (1, 2, 2, False, 80), (4096, 28, 4, True, 128)])
def test_attention_over_unquantised_k_v(dtype, T, H, HKV, causal, D):
    """mq_attn_prefill: the same kernel with 16-bit K / V read in place from the fused q|k|v output (head_dim 128: the
    decoder; 80: Qwen2-VL's vision tower, non-causal); checker = float64 softmax attention."""
    from mquant_amd import ops
    g = torch.Generator(device=DEV).manual_seed(T + 3 * H)
    qkv = (torch.randn(T, (H + 2 * HKV) * D, generator=g, device=DEV) * 0.9).to(dtype)
    q = qkv[:, :H * D].view(T, H, D)
    k = qkv[:, H * D:(H + HKV) * D].view(T, HKV, D)
    v = qkv[:, (H + HKV) * D:].view(T, HKV, D)
    got = ops.attn_prefill(q, k, v, causal=causal)
    want, bound = reference(q, k, v, causal)
    _within(got, want, bound, f"16-bit T={T} H={H} HKV={HKV} D={D} causal={causal}")
    tol = 2.5e-3 if dtype == torch.float16 else 1.6e-2
    assert float((got.double() - want).abs().max() / want.abs().max()) < tol
    # and against torch SDPA in the same dtype (the op it replaces in the whole-prefill glue)
    o = F.scaled_dot_product_attention(q.permute(1, 0, 2)[None], k.permute(1, 0, 2)[None], v.permute(1, 0, 2)[None],
                                       is_causal=causal, enable_gqa=True)[0].permute(1, 0, 2).reshape(T, H * D)
    assert float((got.float() - o.float()).abs().max() / o.float().abs().max()) < 2 * tol


@pytest.mark.parametrize("variant,T,H,HKV,D,causal", [("fp16", 768, 28, 4, 128, True), ("fp8", 768, 28, 4, 128, True),
                                                      ("fp16", 1024, 16, 16, 80, False), ("fp16", 77, 4, 2, 128, True),
                                                      ("fp8", 130, 8, 8, 128, False), ("bf16", 300, 8, 4, 80, True)])
@pytest.mark.parametrize("tiled", [True, False])
def test_fused_output_quantizer_equals_attention_then_quantize(variant, T, H, HKV, D, causal, tiled):
    """mq_attn_prefill_quant_i8: the int8 levels of the next Linear's static quantizer straight from the attention store
    -- bit for bit what mq_quantize_act_i8 makes of the 16-bit attention output, two scales selected by the token-type
    mask (MSQ), tiled and row-major destinations."""
    from mquant_amd import ops
    dtype = torch.bfloat16 if variant == "bf16" else torch.float16
    g = torch.Generator(device=DEV).manual_seed(T + H + D)
    qkv = (torch.randn(T, (H + 2 * HKV) * D, generator=g, device=DEV) * 0.9).to(dtype)
    q = qkv[:, :H * D].view(T, H, D)
    k = qkv[:, H * D:(H + HKV) * D].view(T, HKV, D)
    v = qkv[:, (H + HKV) * D:].view(T, HKV, D)
    sel = (torch.arange(T, device=DEV) % 3 == 1).to(torch.uint8)
    if variant == "fp8":
        kv = qkv[:, H * D:].view(T, 2 * HKV, D)
        scale = ops.kv_scale_from_absmax(kv)
        cache = ops.kv_quant_fp8(kv, scale)
        o = ops.attn_prefill_fp8kv(q, cache, scale, causal=causal)
        kw = dict(kv_cache=cache, kv_scale=scale)
    else:
        o = ops.attn_prefill(q, k, v, causal=causal)
        kw = dict(k=k, v=v)
    s0 = float(o.float().abs().max()) / 127.0 * 0.8          # some rows saturate
    s1 = 0.37 * s0
    want, _ = ops.quantize_act_i8(o, s0, s1, row_sel=sel, tiled=tiled)
    got = ops.attn_prefill_quant_i8(q, s0, s1, causal=causal, row_sel=sel, tiled=tiled, **kw)
    a = got.to_rows() if tiled else got
    b = want.to_rows() if tiled else want
    assert a.shape == b.shape == (T, H * D)
    assert torch.equal(a, b)
    assert int(a.abs().max()) >= 127


@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("variant,T,H,HKV,D,causal", [("fp8", 768, 28, 4, 128, True), ("fp16", 333, 8, 2, 128, True),
                                                      ("fp16", 1024, 16, 16, 80, False), ("fp8", 65, 4, 4, 128, False)])
def test_both_workgroup_widths_give_the_same_attention(waves, variant, T, H, HKV, D, causal):
    """The keys are split over 4 or 2 waves of a workgroup (chosen by shape; forced here through the test hook): each split
    against the float64 checker, and the two against each other within half-precision rounding (the partial softmax states
    merge in a different grouping)."""
    from mquant_amd import ops
    from mquant_amd._lib import call
    g = torch.Generator(device=DEV).manual_seed(T + D)
    qkv = (torch.randn(T, (H + 2 * HKV) * D, generator=g, device=DEV) * 0.9).half()
    q = qkv[:, :H * D].view(T, H, D)
    k = qkv[:, H * D:(H + HKV) * D].view(T, HKV, D)
    v = qkv[:, (H + HKV) * D:].view(T, HKV, D)
    try:
        call("mq_attn_debug_waves", waves)
        if variant == "fp8":
            kv = qkv[:, H * D:].view(T, 2 * HKV, D)
            scale = ops.kv_scale_from_absmax(kv)
            cache = ops.kv_quant_fp8(kv, scale)
            got = ops.attn_prefill_fp8kv(q, cache, scale, causal=causal)
            want, bound = _ref(q, cache, scale, causal)
        else:
            got = ops.attn_prefill(q, k, v, causal=causal)
            want, bound = reference(q, k, v, causal)
    finally:
        call("mq_attn_debug_waves", 0)
    _within(got, want, bound, f"{waves} waves, {variant} T={T}")
    assert float((got.double() - want).abs().max() / want.abs().max()) < 2.5e-3


@pytest.mark.parametrize("variant", ["fp16", "bf16", "fp8"])
@pytest.mark.parametrize("T", [33, 64, 65, 97, 160, 161, 352, 1000])
def test_paired_shallow_tiles_cover_every_tile_count(variant, T):
    """Causal launches may give a workgroup TWO query tiles of the shallow half (round 6; taken by shape at the 7B prefill, forced
    here through the test hook: 4 = paired, 5 = one tile per workgroup).  Tile counts 2, 3, 5, 6, 11 and 32 walk every branch of
    the row map -- an odd shallow half leaves its middle tile alone --; ragged last tiles; each form against the float64 checker,
    and the fused int8 store against attention-then-quantize under the pairing."""
    from mquant_amd import ops
    from mquant_amd._lib import call
    H, HKV, D = 6, 2, 128
    dtype = torch.bfloat16 if variant == "bf16" else torch.float16
    g = torch.Generator(device=DEV).manual_seed(T)
    qkv = (torch.randn(T, (H + 2 * HKV) * D, generator=g, device=DEV) * 0.9).to(dtype)
    q = qkv[:, :H * D].view(T, H, D)
    k = qkv[:, H * D:(H + HKV) * D].view(T, HKV, D)
    v = qkv[:, (H + HKV) * D:].view(T, HKV, D)
    out = {}
    try:
        for hook in (4, 5):
            call("mq_attn_debug_waves", hook)
            if variant == "fp8":
                kv = qkv[:, H * D:].view(T, 2 * HKV, D)
                scale = ops.kv_scale_from_absmax(kv)
                cache = ops.kv_quant_fp8(kv, scale)
                out[hook] = ops.attn_prefill_fp8kv(q, cache, scale, causal=True)
                want, bound = _ref(q, cache, scale, True)
                kw = dict(kv_cache=cache, kv_scale=scale)
            else:
                out[hook] = ops.attn_prefill(q, k, v, causal=True)
                want, bound = reference(q, k, v, True)
                kw = dict(k=k, v=v)
            _within(out[hook], want, bound, f"hook {hook}, {variant} T={T}")
            tol = 1.6e-2 if variant == "bf16" else 2.5e-3
            assert float((out[hook].double() - want).abs().max() / want.abs().max()) < tol, hook
            if hook == 4:
                s0 = float(out[4].float().abs().max()) / 127.0 * 0.8
                sel = (torch.arange(T, device=DEV) % 2).to(torch.uint8)
                lv, _ = ops.quantize_act_i8(out[4], s0, 0.5 * s0, row_sel=sel, tiled=True)
                fused = ops.attn_prefill_quant_i8(q, s0, 0.5 * s0, causal=True, row_sel=sel, tiled=True, **kw)
                assert torch.equal(fused.to_rows(), lv.to_rows())
    finally:
        call("mq_attn_debug_waves", 0)
    # the deepest half of the tiles takes the same path in both forms: identical bits there
    n = (T + 31) // 32
    deep_from = (n - n // 2) * 32
    assert torch.equal(out[4][deep_from:], out[5][deep_from:])


def test_random_shapes_through_every_launch_form():
    """Seeded sweep over token counts, head geometries, causal / not, the three K / V forms and the four launch forms (by shape, 2 waves,
    4 waves with paired shallow tiles, 4 waves unpaired): the row map of the grid -- heads in x, second round reversed, paired rows -- must
    visit every (head, query tile) exactly once whatever the counts are; each result against the float64 checker."""
    from mquant_amd import ops
    from mquant_amd._lib import call
    rng = np.random.default_rng(20260)
    try:
        for case in range(36):
            D = 80 if case % 6 == 5 else 128
            HKV = int(rng.choice([1, 2, 4, 8]))
            H = HKV * int(rng.choice([1, 2, 7]))
            T = int(rng.choice([1, 31, 32, 63, 64, 96, 127, 192, 250, 383, 640, 900, 1111]))
            causal = bool(rng.integers(0, 2))
            variant = "fp16" if D == 80 else str(rng.choice(["fp16", "bf16", "fp8"]))
            hook = int(rng.choice([0, 2, 4, 5]))
            dtype = torch.bfloat16 if variant == "bf16" else torch.float16
            g = torch.Generator(device=DEV).manual_seed(1000 + case)
            qkv = (torch.randn(T, (H + 2 * HKV) * D, generator=g, device=DEV) * 0.9).to(dtype)
            q = qkv[:, :H * D].view(T, H, D)
            k = qkv[:, H * D:(H + HKV) * D].view(T, HKV, D)
            v = qkv[:, (H + HKV) * D:].view(T, HKV, D)
            call("mq_attn_debug_waves", hook)
            if variant == "fp8":
                kv = qkv[:, H * D:].view(T, 2 * HKV, D)
                scale = ops.kv_scale_from_absmax(kv)
                cache = ops.kv_quant_fp8(kv, scale)
                got = ops.attn_prefill_fp8kv(q, cache, scale, causal=causal)
                want, bound = _ref(q, cache, scale, causal)
            else:
                got = ops.attn_prefill(q, k, v, causal=causal)
                want, bound = reference(q, k, v, causal)
            what = (case, T, H, HKV, D, causal, variant, hook)
            _within(got, want, bound, what)
            tol = 1.6e-2 if variant == "bf16" else 2.5e-3
            err = float((got.double() - want).abs().max() / want.abs().max())
            assert err < tol, (what, err)
    finally:
        call("mq_attn_debug_waves", 0)


def test_size_independent_properties_at_full_size():
    """Properties that need no checker: (i) scaling V by a power of two scales the output exactly (the V scale rides in the
    output scale / the values themselves, the softmax does not see it); (ii) a query whose keys all carry the same V row
    returns that row (softmax weights sum to one) within half-precision rounding; (iii) T = 0 is accepted."""
    from mquant_amd import ops
    T, H, HKV, D = 768, 28, 4, 128
    g = torch.Generator(device=DEV).manual_seed(99)
    qkv = (torch.randn(T, (H + 2 * HKV) * D, generator=g, device=DEV) * 0.7).half()
    q = qkv[:, :H * D].view(T, H, D)
    k = qkv[:, H * D:(H + HKV) * D].view(T, HKV, D)
    v = qkv[:, (H + HKV) * D:].view(T, HKV, D)
    a = ops.attn_prefill(q, k, v, causal=True)
    kc = k.contiguous()                                   # k and v must share their token stride
    b = ops.attn_prefill(q, kc, (v.float() * 4.0).half(), causal=True)
    # exact up to fp16 subnormals: an output below 2^-14 is rounded on a coarser grid than four times itself
    d = (b.float() - a.float() * 4.0).abs()
    assert float(d.max()) <= 3e-7 and bool((d[a.float().abs() >= 2.0 ** -14] == 0).all())
    kv = qkv[:, H * D:].view(T, 2 * HKV, D)
    scale = ops.kv_scale_from_absmax(kv)
    cache = ops.kv_quant_fp8(kv, scale)
    scale4 = scale.clone()
    scale4[HKV:] *= 4.0                                   # the V heads' scales
    a8 = ops.attn_prefill_fp8kv(q, cache, scale, causal=True)
    b8 = ops.attn_prefill_fp8kv(q, cache, scale4, causal=True)
    assert float((b8.float() - a8.float() * 4.0).abs().max()) <= float(a8.float().abs().max()) * 4.0 * 2 ** -10
    row = torch.randn(1, HKV, D, generator=g, device=DEV).half()
    const_v = row.expand(T, HKV, D).contiguous()
    c = ops.attn_prefill(q, kc, const_v, causal=True).view(T, H, D).float()
    want = row[0].float().repeat_interleave(H // HKV, dim=0)[None].expand(T, H, D)
    assert float((c - want).abs().max()) <= float(want.abs().max()) * 3e-3
    e = torch.empty((0, H, D), device=DEV, dtype=torch.float16)
    assert ops.attn_prefill(e, e[:, :HKV], e[:, :HKV]).shape == (0, H * D)


def test_scales_that_would_silently_break_the_softmax_are_refused():
    """The running maximum is taken over raw scores and the scale applied afterwards: zero, negative and non-finite softmax /
    K-V scales must be errors, not wrong probabilities (advisor finding, round 3)."""
    from mquant_amd import ops
    from mquant_amd._lib import MQuantHipError
    T, H, HKV, D = 33, 4, 2, 128
    q = torch.randn(T, H, D, device=DEV, dtype=torch.float16)
    k = torch.randn(T, HKV, D, device=DEV, dtype=torch.float16)
    v = torch.randn(T, HKV, D, device=DEV, dtype=torch.float16)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(MQuantHipError):
            ops.attn_prefill(q, k, v, softmax_scale=bad)
    cache = torch.zeros(T, 2 * HKV, D, device=DEV, dtype=torch.float8_e4m3fn)
    for scales in (torch.tensor([1.0, 1.0, 0.0, 1.0]), torch.tensor([1.0, -1.0, 1.0, 1.0]), torch.tensor([1.0, 1.0, 1.0])):
        with pytest.raises(AssertionError):
            ops.attn_prefill_fp8kv(q, cache, scales.to(DEV))


@pytest.mark.parametrize("variant", ["fp16", "bf16", "fp8"])
@pytest.mark.parametrize("softmax_scale", [0.03, 0.25])
def test_softmax_scales_other_than_the_default(variant, softmax_scale):
    """The softmax scale (and the e4m3 K scale with it) is folded into one fp32 factor of the exponent: a flatter and a
    sharper softmax than the default 128^-0.5 = 0.088, on the 16-bit path and on the e4m3 cache, per element against the
    float64 checker."""
    from mquant_amd import ops
    T, H, HKV, D = 700, 8, 2, 128
    dtype = torch.bfloat16 if variant == "bf16" else torch.float16
    g = torch.Generator(device=DEV).manual_seed(T + int(softmax_scale * 100))
    qkv = (torch.randn(T, (H + 2 * HKV) * D, generator=g, device=DEV) * 0.9).to(dtype)
    q, k, v = _split(qkv, H, HKV, D)
    if variant == "fp8":
        kv = qkv[:, H * D:].view(T, 2 * HKV, D)
        scale = ops.kv_scale_from_absmax(kv)
        cache = ops.kv_quant_fp8(kv, scale)
        got = ops.attn_prefill_fp8kv(q, cache, scale, causal=True, softmax_scale=softmax_scale)
        want, bound = _ref(q, cache, scale, True, softmax_scale)
    else:
        got = ops.attn_prefill(q, k, v, causal=True, softmax_scale=softmax_scale)
        want, bound = reference(q, k, v, True, softmax_scale)
    _within(got, want, bound, f"{variant} softmax_scale={softmax_scale}")
    tol = 1.6e-2 if dtype == torch.bfloat16 else 2.5e-3
    assert float((got.double() - want).abs().max() / want.abs().max()) < tol


# ---- exact properties: torch.equal, no tolerance --------------------------------------------------------------------------
# K / V forms: (variant, head_dim); "fp8" = the e4m3 cache under fp16 q ("fp8bf": under bf16 q)
FORMS = [("fp16", 128), ("bf16", 128), ("fp8", 128), ("fp16", 80), ("bf16", 80)]
E4M3_NAN = (0x7F, 0xFF)


def _split(qkv, H, HKV, D):
    T = qkv.shape[0]
    return (qkv[:, :H * D].view(T, H, D), qkv[:, H * D:(H + HKV) * D].view(T, HKV, D),
            qkv[:, (H + HKV) * D:(H + 2 * HKV) * D].view(T, HKV, D))


def _dtype(variant):
    return torch.bfloat16 if variant in ("bf16", "fp8bf") else torch.float16


def _qkv(seed, T, H, HKV, D, variant):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(T, (H + 2 * HKV) * D, generator=g, device=DEV) * 0.9).to(_dtype(variant))


def _cache_of(qkv, H, HKV, D):
    from mquant_amd import ops
    kv = qkv[:, H * D:(H + 2 * HKV) * D].view(qkv.shape[0], 2 * HKV, D)
    scale = ops.kv_scale_from_absmax(kv)
    return ops.kv_quant_fp8(kv, scale), scale


def _random_codes(shape, seed):
    """e4m3 cache bytes, every code but the two NaN codes"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    b = torch.randint(0, 254, shape, generator=g, device=DEV, dtype=torch.int32)
    b = b + (b >= 0x7F).int() + (b >= 0xFE).int()                     # skip 0x7F and 0xFF
    return b.to(torch.uint8)


def _run(variant, q, kv, causal, softmax_scale=None, out=None, quant=None):
    """kv = (k, v) for the 16-bit forms, (cache, scale) for the e4m3 cache; quant = (s0, row-major int8 out or None)"""
    from mquant_amd import ops
    if variant.startswith("fp8"):
        kw = dict(kv_cache=kv[0], kv_scale=kv[1])
    else:
        kw = dict(k=kv[0], v=kv[1])
    if quant is not None:
        s0, qout = quant
        sel = (torch.arange(q.shape[0], device=DEV) % 3 == 1).to(torch.uint8)
        return ops.attn_prefill_quant_i8(q, s0, 0.5 * s0, causal=causal, softmax_scale=softmax_scale, row_sel=sel,
                                         out=qout, **kw)
    if variant.startswith("fp8"):
        return ops.attn_prefill_fp8kv(q, kw["kv_cache"], kw["kv_scale"], causal=causal, softmax_scale=softmax_scale, out=out)
    return ops.attn_prefill(q, kw["k"], kw["v"], causal=causal, softmax_scale=softmax_scale, out=out)


def _kv(variant, qkv, H, HKV, D, cache=None):
    if variant.startswith("fp8"):
        return cache
    _, k, v = _split(qkv, H, HKV, D)
    return (k, v)


@pytest.mark.parametrize("variant,D", FORMS)
@pytest.mark.parametrize("T", [33, 64, 65, 97, 161, 352, 1000])
def test_future_keys_cannot_change_a_row(variant, D, T):
    """Causal: overwrite K and V of every key after t0 with other finite values; rows <= t0 keep their bits, in the 16-bit
    output and in the fused int8 store.  Exact: a masked score is replaced before the maximum is taken, exp2 turns it into
    0 and 0 times a finite value adds nothing; a rescale triggered by another row of the wave multiplies this one by
    exp2(0) = 1.  t0 at the first row, around the first tile boundary, around the boundary between the deep and the paired
    shallow half of the tiles, and at the next-to-last row; every launch form."""
    from mquant_amd._lib import call
    H, HKV = (6 if D == 128 else 8), 2                                 # the int8 store takes whole 64-column groups
    qkv = _qkv(T * 7 + D, T, H, HKV, D, variant)
    q = _split(qkv, H, HKV, D)[0]
    cache = _cache_of(qkv, H, HKV, D) if variant.startswith("fp8") else None
    n = (T + 31) // 32
    deep_from = (n - n // 2) * 32
    t0s = sorted({t for t in (0, 30, 31, 32, 33, deep_from - 1, deep_from, T - 2) if 0 <= t <= T - 2})
    try:
        for hook in HOOKS:
            call("mq_attn_debug_waves", hook)
            base = _run(variant, q, _kv(variant, qkv, H, HKV, D, cache), True)
            s0 = float(base.float().abs().max()) / 127.0 * 0.8
            base_i8 = _run(variant, q, _kv(variant, qkv, H, HKV, D, cache), True, quant=(s0, None))
            for t0 in t0s:
                if cache is not None:
                    c2 = cache[0].view(torch.uint8).clone()
                    c2[t0 + 1:] = _random_codes(c2[t0 + 1:].shape, t0 + hook)
                    kv2 = (c2.view(torch.float8_e4m3fn), cache[1])
                    qkv2 = qkv
                else:
                    qkv2 = qkv.clone()
                    qkv2[t0 + 1:, H * D:] *= 8
                    kv2 = _kv(variant, qkv2, H, HKV, D)
                got = _run(variant, q, kv2, True)
                assert torch.equal(got[:t0 + 1], base[:t0 + 1]), (hook, t0)
                assert not torch.equal(got[t0 + 1:], base[t0 + 1:]), (hook, t0)           # the overwrite did reach the kernel
                got_i8 = _run(variant, q, kv2, True, quant=(s0, None))
                assert torch.equal(got_i8[:t0 + 1], base_i8[:t0 + 1]), (hook, t0)
    finally:
        call("mq_attn_debug_waves", 0)


@pytest.mark.parametrize("variant,D", FORMS)
@pytest.mark.parametrize("group", [1, 2, 7])
def test_other_heads_cannot_change_a_head(variant, D, group):
    """Perturb q of every head but h and K / V of every kv head but h's: head h's columns keep their bits (the grid's head
    map and the kv head of a query head, GQA groups of 1, 2 and 7), causal and not, every launch form."""
    from mquant_amd._lib import call
    T, HKV = 161, 2
    H = HKV * group
    qkv = _qkv(T + group + D, T, H, HKV, D, variant)
    q = _split(qkv, H, HKV, D)[0]
    cache = _cache_of(qkv, H, HKV, D) if variant.startswith("fp8") else None
    try:
        for hook in HOOKS:
            call("mq_attn_debug_waves", hook)
            for causal in (True, False):
                base = _run(variant, q, _kv(variant, qkv, H, HKV, D, cache), causal)
                for h in sorted({0, H - 1, H // 2}):
                    g = h // group
                    qkv2 = qkv.clone()
                    others = [x for x in range(H) if x != h]
                    for x in others:
                        qkv2[:, x * D:(x + 1) * D] *= -2
                    kvh = [x for x in range(HKV) if x != g]
                    if cache is not None:
                        c2 = cache[0].view(torch.uint8).clone()
                        for x in kvh:
                            c2[:, x] = _random_codes(c2[:, x].shape, 10 * h + x)
                            c2[:, HKV + x] = _random_codes(c2[:, x].shape, 10 * h + x + 5)
                        kv2 = (c2.view(torch.float8_e4m3fn), cache[1])
                    else:
                        for x in kvh:
                            qkv2[:, (H + x) * D:(H + x + 1) * D] *= 3
                            qkv2[:, (H + HKV + x) * D:(H + HKV + x + 1) * D] *= -5
                        kv2 = _kv(variant, qkv2, H, HKV, D)
                    got = _run(variant, _split(qkv2, H, HKV, D)[0], kv2, causal)
                    cols = slice(h * D, (h + 1) * D)
                    assert torch.equal(got[:, cols], base[:, cols]), (hook, causal, h)
                    if others:
                        assert not torch.equal(got, base), (hook, causal, h)
    finally:
        call("mq_attn_debug_waves", 0)


def _padded(variant, T, H, HKV, D, fill, extra_cols=0, seed=0):
    """q|k|v (or q and the cache) as the first T rows of allocations with 32 more rows holding ``fill``"""
    W = (H + 2 * HKV) * D
    dtype = _dtype(variant)
    src = _qkv(seed, T, H, HKV, D, variant)
    big = torch.full((T + 32, W + extra_cols), fill, device=DEV, dtype=dtype)
    big[:T, :W] = src
    qkv = big[:T]
    q = _split(qkv, H, HKV, D)[0]
    if not variant.startswith("fp8"):
        return q, _kv(variant, qkv, H, HKV, D)
    cache, scale = _cache_of(src, H, HKV, D)
    cb = torch.full((T + 32, 2 * HKV + (1 if extra_cols else 0), D), 0x7F if fill != 0 else 0, device=DEV, dtype=torch.uint8)
    cb[:T, :2 * HKV] = cache.view(torch.uint8)
    return q, (cb.view(torch.float8_e4m3fn)[:T, :2 * HKV], scale)


@pytest.mark.parametrize("variant,D", FORMS)
@pytest.mark.parametrize("T", [1, 31, 33, 100, 1000])
def test_nothing_past_t_is_read(variant, D, T):
    """The 32 rows after the last token (and, second form, a spare head slot of the cache / NaN padding columns after the last
    V head) hold NaN: the result must equal the same call over zeros there.  The ragged last key block goes through the
    buffer descriptors' range check (attn_prefill.hip:207-209); the spare rows are inside the allocation, so even a
    descriptor that wrongly covers the whole last block reads allocated memory."""
    from mquant_amd._lib import call
    H, HKV = 4, 2
    try:
        for hook in HOOKS:
            call("mq_attn_debug_waves", hook)
            for causal in (True, False):
                for extra in (0, 64):
                    q0, kv0 = _padded(variant, T, H, HKV, D, 0.0, extra, seed=T + D)
                    qn, kvn = _padded(variant, T, H, HKV, D, float("nan"), extra, seed=T + D)
                    want = _run(variant, q0, kv0, causal)
                    got = _run(variant, qn, kvn, causal)
                    assert torch.equal(got, want), (hook, causal, extra)
    finally:
        call("mq_attn_debug_waves", 0)


@pytest.mark.parametrize("variant,D", FORMS)
def test_nothing_outside_the_output_is_written(variant, D):
    """out as big[:T, :H D] of a sentinel-filled buffer with 32 more rows and 64 more columns, for the 16-bit store and for
    the row-major int8 store: everything outside keeps the sentinel, everything inside equals the plain call."""
    from mquant_amd._lib import call
    H, HKV = 4, 2
    try:
        for hook in HOOKS:
            call("mq_attn_debug_waves", hook)
            for T in (1, 33, 100):
                qkv = _qkv(T + hook, T, H, HKV, D, variant)
                q = _split(qkv, H, HKV, D)[0]
                kv = _kv(variant, qkv, H, HKV, D, _cache_of(qkv, H, HKV, D) if variant.startswith("fp8") else None)
                want = _run(variant, q, kv, True)
                big = torch.full((T + 32, H * D + 64), -7.0, device=DEV, dtype=q.dtype)
                _run(variant, q, kv, True, out=big[:T, :H * D])
                assert torch.equal(big[:T, :H * D], want), (hook, T)
                big[:T, :H * D] = -7.0
                assert bool((big == -7.0).all()), (hook, T)
                s0 = float(want.float().abs().max()) / 127.0 * 0.8
                want_i8 = _run(variant, q, kv, True, quant=(s0, None))
                bi = torch.full((T + 32, H * D + 64), 99, device=DEV, dtype=torch.int8)
                _run(variant, q, kv, True, quant=(s0, bi[:T, :H * D]))
                assert torch.equal(bi[:T, :H * D], want_i8), (hook, T)
                bi[:T, :H * D] = 99
                assert bool((bi == 99).all()), (hook, T)
    finally:
        call("mq_attn_debug_waves", 0)


@pytest.mark.parametrize("variant,D", FORMS + [("fp8bf", 128)])
def test_scales_fold_exactly(variant, D):
    """(2 q, softmax_scale / 2) gives the bits of (q, softmax_scale): the scale folds into one fp32 factor and powers of
    two commute with every rounding.  e4m3: (K scales x 2, softmax_scale / 2) gives the unscaled bits, and V scales x 2
    give exactly twice the output wherever it is a normal number (the tighter companion of the 2^-10 check at full size)."""
    from mquant_amd._lib import call
    T, H, HKV = 300, 8, 2
    ss = D ** -0.5
    qkv = _qkv(T + D, T, H, HKV, D, variant)
    q = _split(qkv, H, HKV, D)[0]
    kv = _kv(variant, qkv, H, HKV, D, _cache_of(qkv, H, HKV, D) if variant.startswith("fp8") else None)
    tiny = torch.finfo(q.dtype).tiny
    try:
        for hook in HOOKS:
            call("mq_attn_debug_waves", hook)
            for causal in (True, False):
                base = _run(variant, q, kv, causal, ss)
                assert torch.equal(_run(variant, (q * 2).contiguous(), kv, causal, ss / 2), base), (hook, causal)
                if variant.startswith("fp8"):
                    cache, scale = kv
                    sk = scale.clone()
                    sk[:HKV] *= 2
                    assert torch.equal(_run(variant, q, (cache, sk), causal, ss / 2), base), (hook, causal)
                    sv = scale.clone()
                    sv[HKV:] *= 2
                    b2 = _run(variant, q, (cache, sv), causal, ss)
                    normal = base.float().abs() >= tiny
                    assert bool(normal.float().mean() > 0.99)
                    assert torch.equal(b2[normal], base[normal] * 2), (hook, causal)
    finally:
        call("mq_attn_debug_waves", 0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_every_e4m3_code_through_the_kernel(dtype):
    """T = 1, q = 0: every score is 0, so p = 1 and l = 1 and the output is the V value times its head's scale, rounded once
    to q's dtype.  The two V heads' 128 dims hold all 256 byte codes; NaN codes give NaN.  Values are compared, not bits:
    the accumulator starts at +0, so code 0x80 comes out as +0."""
    import oracle
    from mquant_amd import ops
    from mquant_amd._lib import call
    HKV, H, D = 2, 4, 128
    codes = torch.arange(256, device=DEV, dtype=torch.int32).to(torch.uint8)
    dec = torch.from_numpy(oracle.fp8_e4m3fn_decode(codes.cpu().numpy())).to(DEV)         # float32
    cache = torch.empty((1, 2 * HKV, D), device=DEV, dtype=torch.uint8)
    cache[0, :HKV] = _random_codes((HKV, D), 3)
    cache[0, HKV:] = codes.view(HKV, D)
    cache = cache.view(torch.float8_e4m3fn)
    q = torch.zeros((1, H, D), device=DEV, dtype=dtype)
    nan = torch.isnan(dec).view(HKV, D).repeat_interleave(H // HKV, 0).flatten()
    assert int(nan.sum()) == 2 * (H // HKV)
    try:
        for hook in HOOKS:
            call("mq_attn_debug_waves", hook)
            for s_v in (1.0, 0.3719):
                scale = torch.tensor([0.02, 0.5, s_v, s_v], device=DEV, dtype=torch.float32)
                want = (dec * torch.tensor(s_v, device=DEV, dtype=torch.float32)).to(dtype)
                want = want.view(HKV, D).repeat_interleave(H // HKV, 0).flatten()
                for causal in (True, False):
                    got = ops.attn_prefill_fp8kv(q, cache, scale, causal=causal)[0]
                    assert torch.equal(torch.isnan(got), nan), (hook, s_v)
                    assert torch.equal(got[~nan], want[~nan]), (hook, s_v)
    finally:
        call("mq_attn_debug_waves", 0)
