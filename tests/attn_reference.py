"""Float64 softmax attention with a bound for every output element: the checker of the prefill attention kernels
(``mq_attn_prefill``, ``mq_attn_prefill_fp8kv``, ``mq_attn_prefill_quant_i8``; mquant_amd/csrc/attn_prefill.hip).

A plain helper module like ``golden_inputs.py``.  ``reference`` computes, one head at a time (T = 4096 needs a 128 MiB
float64 score matrix per head), on the device its inputs live on:

    o[t, h, d] = sum_k p_k v[k, g, d] / sum_k p_k,    p_k = exp(s_k - max s),    s_k = softmax_scale * q[t, h] . k[k, g]

over the keys row t may attend to (causal: k <= t), with g = h // (H / HKV) the kv head of query head h (GQA), and

    bound[t, h, d] = u |o|  +  c sum_k max(u p_k, eta) |v_kd| / sum_k p_k  +  n_t 2^-24 sum_k p_k |v_kd| / sum_k p_k

u = 2^-11 (fp16) / 2^-8 (bf16) is the unit roundoff of q's dtype, eta = 2^-25 (fp16) / 0 (bf16), c = 2, n_t the number of
keys row t attends to.  For the e4m3 cache, k and v are the DEQUANTISED values (byte value times the head's scale).

Where each term comes from in the kernel (line numbers of attn_prefill.hip):

* u |o|: the store rounds ``acc * f`` to q's dtype once (lines 382 and 405 / 420; f = s_v / L).  The fp32 product before
  it adds 2^-24 |o|, inside the last term.
* c sum_k max(u p_k, eta) |v_kd| / sum_k p_k: P is packed to q's dtype (``pack2``, line 312) before the second MFMA, one
  rounding per probability.  It is rounded against the RUNNING maximum m_run, so the packed value is
  p_k' = p_k exp(M - m_run) >= p_k, and every later rescale multiplies it by exp(m_run - M) <= 1 in fp32.  A rounding error
  of at most max(u p_k', eta) therefore reaches the output as at most max(u p_k, eta exp(m_run - M)) <= max(u p_k, eta):
  relative u while p_k' is a normal number, and at most half the spacing of fp16 subnormals (2^-25) below 2^-14; bf16 has
  fp32's exponent range, so eta = 0.  ``psum`` sums the UNROUNDED p (line 311), so L does not carry these errors and
  nothing cancels them in the quotient: the full sum divided by L.  c = 2 is this rounding once plus the same size again
  for the fp32 scores, the folded scale (line 173) and exp2 (V_EXP_F32, 1 ulp), which perturb each p_k by a relative
  O(2^-24 |s_k|) -- an order below u at the scores of these tests -- and for a correct kernel whose individual P roundings
  happen to line up.
* n_t 2^-24 sum_k p_k |v_kd| / sum_k p_k: MFMA accumulates P V in fp32, and so do the key blocks of a wave, the rescales
  by alpha (line 315), the merge of the waves' partial states (lines 378-397) and psum / l_run.  The worst case of n_t
  fp32 additions is n_t 2^-24 times the sum of the magnitudes, for the numerator and for L alike; both errors grow as
  sqrt(n_t) 2^-24 in practice, so the one term covers the two.
* Masked keys contribute nothing: a masked score is -1e30 before the maximum (line 295), exp2 turns it into an exact 0,
  and 0 times a finite V is 0.  Keys past T come back as zeros from the buffer range check (lines 207-209).

tests/test_attn_checker_cpu.py emulates these roundings on the CPU and shows that the emulation stays well inside the
bound, and that a wrong mask, a wrong merge weight or a dropped key block breaks it.
"""
import torch

C = 2.0
UNIT_ROUNDOFF = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
ETA = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}
FP32_U = 2.0 ** -24


def dequant_cache(cache: torch.Tensor, kv_scale: torch.Tensor):
    """e4m3 cache [T, 2 HKV, D] (K heads, then V heads) and its [2 HKV] scales -> float64 K, V [T, HKV, D]."""
    hkv = cache.shape[1] // 2
    kvd = cache.float().double() * kv_scale.double()[None, :, None]
    return kvd[:, :hkv], kvd[:, hkv:]


def reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool, softmax_scale: float = None,
              dtype: torch.dtype = None, c: float = C):
    """q [T, H, D], k / v [T, HKV, D] (any float dtype; the e4m3 cache through ``dequant_cache``) -> (o, bound), both
    float64 [T, H * D] on q's device.  ``dtype``: the kernel's P / output dtype, default q's."""
    T, H, D = q.shape
    HKV = k.shape[1]
    assert H % HKV == 0 and k.shape == v.shape == (T, HKV, D)
    dtype = dtype or q.dtype
    u, eta = UNIT_ROUNDOFF[dtype], ETA[dtype]
    scale = D ** -0.5 if softmax_scale is None else float(softmax_scale)
    rep = H // HKV
    dev = q.device
    qd, kd, vd = q.double(), k.double(), v.double()
    o = torch.empty((T, H, D), dtype=torch.float64, device=dev)
    bound = torch.empty((T, H, D), dtype=torch.float64, device=dev)
    rows = torch.arange(T, device=dev)
    masked = (rows[None, :] > rows[:, None]) if causal else None        # [query, key]
    n_t = (rows + 1 if causal else torch.full((T,), T, device=dev)).double()[:, None]
    for h in range(H):
        g = h // rep
        p = (qd[:, h] @ kd[:, g].T).mul_(scale)                       # scores [T, T]
        if causal:
            p.masked_fill_(masked, float("-inf"))
        p.sub_(p.amax(dim=1, keepdim=True)).exp_()                    # p_k; masked -> 0
        l = p.sum(dim=1, keepdim=True)
        va = vd[:, g].abs()
        oh = (p @ vd[:, g]) / l
        pva = (p @ va) / l
        w = p.mul_(u)                                                 # p is not needed any more
        if eta > 0:
            w.clamp_(min=eta)
            if causal:
                w.masked_fill_(masked, 0.0)
        o[:, h] = oh
        bound[:, h] = u * oh.abs() + c * (w @ va) / l + n_t * FP32_U * pva
        del p, w
    return o.view(T, H * D), bound.view(T, H * D)


def bound_ratio(got: torch.Tensor, o: torch.Tensor, bound: torch.Tensor) -> float:
    """max over elements of |got - o| / bound (NaN anywhere in got counts as infinitely far)."""
    err = (got.double().reshape(o.shape) - o).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max()) if err.numel() else 0.0


def assert_within(got: torch.Tensor, o: torch.Tensor, bound: torch.Tensor, what=None) -> float:
    """Every element of got within its bound; returns the largest error / bound ratio."""
    r = bound_ratio(got, o, bound)
    if not r <= 1.0:
        err = (got.double().reshape(o.shape) - o).abs()
        err = torch.where(err == 0, torch.zeros_like(err), err / bound)
        i = int(torch.argmax(torch.nan_to_num(err, nan=float("inf")).flatten()))
        t, col = divmod(i, o.shape[1])
        raise AssertionError(f"{what}: error / bound {r:.3g} > 1 at row {t}, column {col} "
                             f"(got {float(got.reshape(o.shape)[t, col])}, want {float(o[t, col])}, bound {float(bound[t, col]):.3g})")
    return r
