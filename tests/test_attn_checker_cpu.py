"""The per-element bound of tests/attn_reference.py has teeth (CPU only, seconds).

``emulate`` restates the prefill attention kernel's arithmetic (mquant_amd/csrc/attn_prefill.hip) in fp32 on the CPU: fp32
scores, the softmax scale (and the e4m3 K scale) folded with log2(e) into one fp32 factor, keys split over four waves in
32-key blocks with a running maximum per wave, P rounded to q's dtype against that running maximum, l summed from the
unrounded p, fp32 accumulation, the waves' states merged by exp2(m_w - M), one rounding of acc * (s_v / L) at the store.
A correct kernel must stay well inside the bound; the same emulation with a wrong causal mask, a wrong merge weight or a
dropped key block must break it -- in fp16, where the bound is tight enough to see the merge weight, and for the mask in
bf16 as well."""
import pytest
import torch

from attn_reference import assert_within, bound_ratio, dequant_cache, reference

KB, NW = 32, 4
LOG2E = 1.4426950408889634


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def emulate(q, k, v, causal, softmax_scale=None, s_k=1.0, s_v=1.0, defect=None):
    """q [T, H, D] in fp16 / bf16; k, v [T, HKV, D] holding the values the kernel multiplies (q's dtype, or the e4m3 byte
    values with per-head scales s_k / s_v, lists of HKV floats) -> [T, H * D] in q's dtype.  ``defect``: "mask" (rows of
    the deep half of the query tiles also admit key t + 1 inside their diagonal block, as a causal kmax one too large does;
    a key past T is the range check's zero), "merge" (the last wave's state weighs 5 % too much in the merge, deep half),
    "drop" (the deep half of the tiles skips key block 1)."""
    T, H, D = q.shape
    HKV = k.shape[1]
    dtype = q.dtype
    n = (T + KB - 1) // KB
    Tp = n * KB
    scale = D ** -0.5 if softmax_scale is None else softmax_scale
    s_k = [s_k] * HKV if isinstance(s_k, float) else s_k
    s_v = [s_v] * HKV if isinstance(s_v, float) else s_v
    kp = torch.zeros(Tp, HKV, D)                                     # rows past T: the buffer range check's zeros
    vp = torch.zeros(Tp, HKV, D)
    kp[:T], vp[:T] = k.float(), v.float()
    rows, keys = torch.arange(T), torch.arange(Tp)
    qt = rows // KB
    deep = qt >= n // 2
    adm = (keys[None, :] <= rows[:, None]) if causal else (keys[None, :] < T).expand(T, Tp)
    if defect == "mask":
        adm = adm | ((keys[None, :] == rows[:, None] + 1) & (keys[None, :] // KB == qt[:, None]) & deep[:, None])
    n_blocks = (qt + 1) if causal else torch.full((T,), n)
    out = torch.empty(T, H, D, dtype=dtype)
    for h in range(H):
        g = h // (H // HKV)
        sc = _f32(s_k[g]) * _f32(scale) * _f32(LOG2E)                 # fp32, in this order (attn_prefill.hip:173)
        S = q[:, h].float() @ kp[:, g].T                             # fp32 scores
        S = torch.where(adm, S, _f32(-1.0e30))
        ms, ls, Os = [], [], []
        for w in range(NW):
            m = torch.full((T,), -1.0e30)
            l = torch.zeros(T)
            O = torch.zeros(T, D)
            for kb in range(w, n, NW):
                act = kb < n_blocks
                if defect == "drop":
                    act = act & ~(deep & (kb == 1))
                Sb = S[:, kb * KB:(kb + 1) * KB]
                m_new = torch.maximum(m, Sb.amax(dim=1) * sc)
                p = torch.exp2((Sb.double() * sc.double() - m_new.double()[:, None]).float())   # fma: one rounding
                alpha = torch.exp2(m - m_new)
                l = torch.where(act, l * alpha + p.sum(dim=1), l)
                pv = p.to(dtype).float() @ vp[kb * KB:(kb + 1) * KB, g]
                O = torch.where(act[:, None], O * alpha[:, None] + pv, O)
                m = torch.where(act, m_new, m)
            ms.append(m), ls.append(l), Os.append(O)
        M = torch.stack(ms).amax(dim=0)
        fw = [torch.exp2(m - M) for m in ms]
        if defect == "merge":
            fw[NW - 1] = torch.where(deep, fw[NW - 1] * _f32(1.05), fw[NW - 1])
        L = sum(lw * f for lw, f in zip(ls, fw))
        acc = sum(O * f[:, None] for O, f in zip(Os, fw))
        f = _f32(s_v[g]) / L
        out[:, h] = (acc * f[:, None]).to(dtype)
    return out.view(T, H * D)


def _inputs(seed, T, H, HKV, dtype, q_gain=1.0, D=128):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(T, (H + 2 * HKV) * D, generator=g) * 0.9).to(dtype)
    qkv[:, :H * D] = (qkv[:, :H * D].float() * q_gain).to(dtype)
    return qkv[:, :H * D].view(T, H, D), qkv[:, H * D:(H + HKV) * D].view(T, HKV, D), qkv[:, (H + HKV) * D:].view(T, HKV, D)


def _fp8_inputs(seed, T, H, HKV, dtype):
    """The e4m3 path: cache bytes as torch.float8_e4m3fn with absmax / 448 per-head scales, as kv_scale_from_absmax."""
    q, k, v = _inputs(seed, T, H, HKV, dtype)
    kv = torch.cat([k, v], dim=1).float()
    scale = (kv.abs().amax(dim=(0, 2)).clamp_min(1e-8) / 448.0).float()
    cache = (kv / scale[None, :, None]).to(torch.float8_e4m3fn)
    return q, cache, scale


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("T,H,HKV,causal,q_gain,D,scale", [(300, 4, 2, True, 1.0, 128, None), (777, 2, 1, False, 1.0, 128, None),
                                                           (300, 2, 2, True, 6.0, 128, None), (1000, 2, 1, True, 3.0, 128, None),
                                                           (200, 4, 2, True, 1.0, 80, None), (333, 2, 2, False, 1.0, 128, 0.3)])
def test_the_kernel_roundings_stay_inside_the_bound(dtype, T, H, HKV, causal, q_gain, D, scale):
    q, k, v = _inputs(T + H, T, H, HKV, dtype, q_gain, D)
    got = emulate(q, k, v, causal, scale)
    o, bound = reference(q, k, v, causal, scale)
    assert bound_ratio(got, o, bound) <= 0.6
    assert_within(got, o, bound, "emulation")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("causal", [True, False])
def test_the_e4m3_path_stays_inside_the_bound(dtype, causal):
    T, H, HKV = 300, 4, 2
    q, cache, scale = _fp8_inputs(7, T, H, HKV, dtype)
    k8, v8 = cache[:, :HKV].float(), cache[:, HKV:].float()
    got = emulate(q, k8, v8, causal, None, s_k=scale[:HKV].tolist(), s_v=scale[HKV:].tolist())
    o, bound = reference(q, *dequant_cache(cache, scale), causal, dtype=dtype)
    assert bound_ratio(got, o, bound) <= 0.6


@pytest.mark.parametrize("defect", ["mask", "merge", "drop"])
def test_each_defect_breaks_the_bound_in_fp16(defect):
    T, H, HKV = 1000, 8, 2
    q, k, v = _inputs(1, T, H, HKV, torch.float16)
    o, bound = reference(q, k, v, True)
    assert bound_ratio(emulate(q, k, v, True), o, bound) <= 0.6
    assert bound_ratio(emulate(q, k, v, True, defect=defect), o, bound) > 1.0


def test_a_causal_mask_one_key_too_wide_breaks_the_bound_in_bf16():
    T, H, HKV = 1000, 8, 2
    q, k, v = _inputs(1, T, H, HKV, torch.bfloat16)
    o, bound = reference(q, k, v, True)
    assert bound_ratio(emulate(q, k, v, True), o, bound) <= 0.6
    assert bound_ratio(emulate(q, k, v, True, defect="mask"), o, bound) > 1.0
