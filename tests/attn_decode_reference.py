"""Float64 softmax attention of R query rows over the first n keys, with a bound for every output element: the checker of the
decode attention kernels (``mq_attn_decode_fp8kv``, ``mq_attn_decode_fp8kv_quant_i8``; mquant_amd/csrc/attn_decode.hip).

The formula and the constants are those of tests/attn_reference.py (``C``, ``UNIT_ROUNDOFF``, ``ETA``; its docstring derives
every term), evaluated for the R rows alone -- the LAST R positions of a sequence of n tokens -- so that a long cache costs
R x n scores per head instead of n x n:

    o[r, h, d] = sum_k p_k v[k, g, d] / sum_k p_k,    p_k = exp(s_k - max s),    s_k = softmax_scale * q[r, h] . k[k, g]

over the keys row r attends to (causal: k <= n - R + r; else all n), g = h // (H / HKV), and

    bound[r, h, d] = u |o|  +  c sum_k max(u p_k, eta) |v_kd| / sum_k p_k  +  n_r 2^-24 sum_k p_k |v_kd| / sum_k p_k

with n_r the number of keys row r attends to.  The derivation does not depend on how the keys are grouped: the decode kernel
packs P against a running maximum per wave exactly as the prefill kernel does, and its merges -- four waves through LDS, then
the key ranges in a second launch -- are fp32 products and sums that the last term counts like any other of the n_r additions.
tests/test_attn_decode_checker_cpu.py pins this module to ``attn_reference.reference`` and shows that an emulation of the split
and the ordered merge stays inside the bound while a dropped range, a wrong merge weight or an empty range merged as (0, 0) do
not."""
import torch

from attn_reference import C, ETA, UNIT_ROUNDOFF, dequant_cache  # noqa: F401  (dequant_cache: re-exported for the tests)

FP32_U = 2.0 ** -24


def decode_reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool, softmax_scale: float = None,
                     dtype: torch.dtype = None, c: float = C):
    """q [R, H, D] (the last R positions), k / v [n, HKV, D] (any float dtype; the e4m3 cache through ``dequant_cache``)
    -> (o, bound), both float64 [R, H * D] on q's device.  ``dtype``: the kernel's P / output dtype, default q's."""
    R, H, D = q.shape
    n, HKV = k.shape[0], k.shape[1]
    assert H % HKV == 0 and k.shape == v.shape == (n, HKV, D) and n >= R
    dtype = dtype or q.dtype
    u, eta = UNIT_ROUNDOFF[dtype], ETA[dtype]
    scale = D ** -0.5 if softmax_scale is None else float(softmax_scale)
    rep = H // HKV
    dev = q.device
    qd, kd, vd = q.double(), k.double(), v.double()
    o = torch.empty((R, H, D), dtype=torch.float64, device=dev)
    bound = torch.empty((R, H, D), dtype=torch.float64, device=dev)
    last = (n - R + torch.arange(R, device=dev)) if causal else torch.full((R,), n - 1, device=dev)     # last key of a row
    masked = torch.arange(n, device=dev)[None, :] > last[:, None]                                          # [row, key]
    n_r = (last + 1).double()[:, None]
    for h in range(H):
        g = h // rep
        p = (qd[:, h] @ kd[:, g].T).mul_(scale)
        p.masked_fill_(masked, float("-inf"))
        p.sub_(p.amax(dim=1, keepdim=True)).exp_()
        l = p.sum(dim=1, keepdim=True)
        va = vd[:, g].abs()
        oh = (p @ vd[:, g]) / l
        pva = (p @ va) / l
        w = p.mul_(u)
        if eta > 0:
            w.clamp_(min=eta)
            w.masked_fill_(masked, 0.0)
        o[:, h] = oh
        bound[:, h] = u * oh.abs() + c * (w @ va) / l + n_r * FP32_U * pva
    return o.view(R, H * D), bound.view(R, H * D)
