"""tests/attn_decode_reference.py is tests/attn_reference.py restricted to the last R rows, and its bound has teeth for the
decode kernel's split and ordered merge (CPU only, seconds).

``emulate`` restates the arithmetic of mquant_amd/csrc/attn_decode.hip in fp32 on the CPU, modelled on
test_attn_checker_cpu.emulate: the keys cut into ranges of keys_per_split, each range's 32-key blocks dealt to four waves with a
running maximum of their own, P rounded to q's dtype against that running maximum, l summed from the unrounded p, fp32
accumulation, the four waves merged by exp2(m_w - M), then the ranges merged IN INDEX ORDER by the same rule, and one rounding of
acc * (s_v / L) at the store.  A correct kernel must stay well inside the bound; the same emulation must break it in fp16 with a
dropped range, with a merge weight 5 % off, and with an empty range merged as (m, l) = (0, 0) -- what a zero-filled workspace
would supply if the merge read the slot of a range that starts beyond n."""
import pytest
import torch

from attn_decode_reference import decode_reference, dequant_cache
from attn_reference import assert_within, bound_ratio, reference

KB, NW = 32, 4
LOG2E = 1.4426950408889634


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def emulate(q, k, v, causal, keys_per_split, softmax_scale=None, s_k=1.0, s_v=1.0, defect=None):
    """q [R, H, D] fp16 / bf16 (the last R positions); k, v [n, HKV, D] holding the values the kernel multiplies (the e4m3 byte
    values with per-head scales s_k / s_v, or plain values with scales 1) -> [R, H * D] in q's dtype.  ``defect``: "drop" (the
    merge skips range 1), "merge" (the last range weighs 5 % too much), "empty" (one more range, beyond n, is merged with the
    state (m, l, acc) = (0, 0, 0) of a zero-filled workspace)."""
    R, H, D = q.shape
    n, HKV = k.shape[0], k.shape[1]
    dtype = q.dtype
    scale = D ** -0.5 if softmax_scale is None else softmax_scale
    s_k = [s_k] * HKV if isinstance(s_k, float) else s_k
    s_v = [s_v] * HKV if isinstance(s_v, float) else s_v
    assert keys_per_split % KB == 0
    splits = -(-n // keys_per_split)
    npad = splits * keys_per_split
    kp, vp = torch.zeros(npad, HKV, D), torch.zeros(npad, HKV, D)      # rows at or beyond n: the buffer range check's zeros
    kp[:n], vp[:n] = k.float(), v.float()
    last = (n - R + torch.arange(R)) if causal else torch.full((R,), n - 1)
    adm = torch.arange(npad)[None, :] <= last[:, None]
    out = torch.empty(R, H, D, dtype=dtype)
    for h in range(H):
        g = h // (H // HKV)
        sc = _f32(s_k[g]) * _f32(scale) * _f32(LOG2E)
        S = torch.where(adm, q[:, h].float() @ kp[:, g].T, _f32(float("-inf")))
        parts = []
        for s in range(splits):
            k0, k1 = s * keys_per_split, min((s + 1) * keys_per_split, n)
            nb = -(-(k1 - k0) // KB)
            ms, ls, Os = [], [], []
            for w in range(NW):
                m, l, O = torch.full((R,), -1.0e30), torch.zeros(R), torch.zeros(R, D)
                for kb in range(w, nb, NW):
                    lo = k0 + kb * KB
                    Sb = S[:, lo:lo + KB]
                    m_new = torch.maximum(m, Sb.amax(dim=1) * sc)
                    p = torch.exp2((Sb.double() * sc.double() - m_new.double()[:, None]).float())      # fma: one rounding
                    alpha = torch.exp2(m - m_new)
                    l = l * alpha + p.sum(dim=1)
                    O = O * alpha[:, None] + p.to(dtype).float() @ vp[lo:lo + KB, g]
                    m = m_new
                ms.append(m), ls.append(l), Os.append(O)
            M = torch.stack(ms).amax(dim=0)
            fw = [torch.exp2(m - M) for m in ms]
            parts.append((M, sum(l * f for l, f in zip(ls, fw)), sum(O * f[:, None] for O, f in zip(Os, fw))))
        if defect == "drop":
            del parts[1]
        if defect == "empty":
            parts.append((torch.zeros(R), torch.zeros(R), torch.zeros(R, D)))
        M = torch.stack([p[0] for p in parts]).amax(dim=0)
        fw = [torch.exp2(p[0] - M) for p in parts]
        if defect == "merge":
            fw[-1] = fw[-1] * _f32(1.05)
        L = sum(p[1] * f for p, f in zip(parts, fw))
        acc = sum(p[2] * f[:, None] for p, f in zip(parts, fw))
        f = torch.where(L > 0, _f32(s_v[g]) / L, torch.zeros(R))
        out[:, h] = (acc * f[:, None]).to(dtype)
    return out.view(R, H * D)


def _inputs(seed, n, H, HKV, dtype, q_gain=1.0, D=128):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(n, (H + 2 * HKV) * D, generator=g) * 0.9).to(dtype)
    qkv[:, :H * D] = (qkv[:, :H * D].float() * q_gain).to(dtype)
    return qkv[:, :H * D].view(n, H, D), qkv[:, H * D:(H + HKV) * D].view(n, HKV, D), qkv[:, (H + HKV) * D:].view(n, HKV, D)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_the_decode_checker_is_the_prefill_checker_on_the_last_rows(dtype, causal, R):
    T, H, HKV = 97, 4, 2
    q, k, v = _inputs(3, T, H, HKV, dtype)
    o, bound = reference(q, k, v, causal)
    od, bd = decode_reference(q[T - R:], k, v, causal)
    torch.testing.assert_close(od, o[T - R:], rtol=1e-12, atol=0)
    torch.testing.assert_close(bd, bound[T - R:], rtol=1e-12, atol=0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n,R,H,HKV,causal,kps,q_gain", [(1000, 1, 8, 2, True, 128, 1.0), (1000, 1, 8, 2, True, 1024, 1.0),
                                                         (300, 3, 4, 2, True, 96, 1.0), (300, 8, 2, 2, False, 128, 1.0),
                                                         (777, 2, 4, 1, True, 32, 6.0), (65, 2, 4, 2, True, 64, 3.0)])
def test_the_split_and_the_ordered_merge_stay_inside_the_bound(dtype, n, R, H, HKV, causal, kps, q_gain):
    q, k, v = _inputs(n + H, n, H, HKV, dtype, q_gain)
    got = emulate(q[n - R:], k, v, causal, kps)
    o, bound = decode_reference(q[n - R:], k, v, causal)
    assert bound_ratio(got, o, bound) <= 0.6
    assert_within(got, o, bound, "emulation")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_the_e4m3_path_stays_inside_the_bound(dtype):
    n, R, H, HKV = 300, 2, 4, 2
    q, k, v = _inputs(7, n, H, HKV, dtype)
    kv = torch.cat([k, v], dim=1).float()
    scale = (kv.abs().amax(dim=(0, 2)).clamp_min(1e-8) / 448.0).float()
    cache = (kv / scale[None, :, None]).to(torch.float8_e4m3fn)
    got = emulate(q[n - R:], cache[:, :HKV].float(), cache[:, HKV:].float(), True, 128, s_k=scale[:HKV].tolist(), s_v=scale[HKV:].tolist())
    o, bound = decode_reference(q[n - R:], *dequant_cache(cache, scale), True, dtype=dtype)
    assert bound_ratio(got, o, bound) <= 0.6


@pytest.mark.parametrize("defect", ["drop", "merge"])
def test_a_dropped_range_and_a_wrong_merge_weight_break_the_bound_in_fp16(defect):
    n, R, H, HKV = 1000, 1, 8, 2
    q, k, v = _inputs(1, n, H, HKV, torch.float16)
    o, bound = decode_reference(q[n - R:], k, v, True)
    assert bound_ratio(emulate(q[n - R:], k, v, True, 256), o, bound) <= 0.6
    assert bound_ratio(emulate(q[n - R:], k, v, True, 256, defect=defect), o, bound) > 1.0


def test_an_empty_range_merged_as_zeros_breaks_the_bound_in_fp16():
    """A state (m, l) = (0, 0) is NOT neutral: m is a log2-domain maximum, and 0 is a large one when every real score is far
    below it.  Keys that all point away from the query (scores near -230 in the log2 domain): with the zero state in the merge
    M becomes 0, every real weight exp2(m_s - 0) underflows to an exact fp32 zero, L is 0 and the row comes out as zeros."""
    n, R, H, HKV = 300, 1, 4, 2
    q, k, v = _inputs(5, n, H, HKV, torch.float16)
    away = torch.zeros(128)
    away[:16] = 12.0
    q = (q.float() * 0.05 + away).to(torch.float16)
    k = (k.float() * 0.05 - away).to(torch.float16)
    o, bound = decode_reference(q[n - R:], k, v, True)
    assert bound_ratio(emulate(q[n - R:], k, v, True, 128), o, bound) <= 0.6
    assert bound_ratio(emulate(q[n - R:], k, v, True, 128, defect="empty"), o, bound) > 1.0
