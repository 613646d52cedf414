"""The cases of tests/test_gpu_attn_decode.py, as plain data: tests/test_attn_decode_plan_cpu.py shows on any machine that the
plans they reach cover every path of the launch (one and several key ranges, one and several passes over the keys).

Inputs are those of test_gpu_attn_prefill._case, restated in ``make_case``: q and K|V are column slices of one fused [rows, (H + 2
HKV) * 128] tensor, the K / V heads carry gains 0.05 / 1 / 6 / 20 (a scale that is wrong for one head shows at once), the scales
come from ``kv_scale_from_absmax`` and the cache from ``kv_quant_fp8``."""
import itertools

KEY_BLOCK = 32                     # AD_KB of mquant_amd/csrc/attn_decode.hip
ROWS_PER_PASS = 16                 # AD_M
HEADS = [(28, 4), (64, 8), (8, 8), (4, 1), (4, 2)]
N_KEYS = [1, 2, 63, 64, 65, 130, 1000]
# (splits, keys_per_split) for mq_attn_decode_debug_force; (0, 0) = the heuristic, (0, 32) = keys_per_split at its minimum
PLANS = [(0, 0), (1, 0), (2, 0), (3, 0), (0, KEY_BLOCK)]
LONG = dict(R=1, n=8197, heads=28, kv_heads=4, causal=True, plan=(0, 0))


def plan_is_refused(n, plan):
    """What attn_decode_plan (attn_decode.hip) refuses: a forced pair that does not cut n keys into non-empty ranges."""
    splits, kps = plan
    if splits == 0:
        return False
    if kps == 0:
        kps = -(-(-(-n // splits)) // KEY_BLOCK) * KEY_BLOCK
    return not (splits * kps >= n > (splits - 1) * kps)


# parity, one row: every dtype x head pair x n x plan the plan function accepts
PARITY = [dict(R=1, n=n, heads=h, kv_heads=g, causal=True, plan=plan)
          for (h, g), n, plan in itertools.product(HEADS, N_KEYS, PLANS) if not plan_is_refused(n, plan)]
# several rows: causal and not, n from R itself, forced 1 and 3 ranges; (64, 8) at R = 3 is 24 (row, head) pairs = two passes
ROWS = [dict(R=R, n=n, heads=h, kv_heads=g, causal=causal, plan=plan)
        for (R, h, g) in [(2, 28, 4), (3, 64, 8), (8, 4, 2), (3, 4, 1)]
        for n in (R, 65, 300) for causal in (True, False) for plan in [(1, 0), (3, 0)] if not plan_is_refused(n, plan)]
HEURISTIC = [c for c in PARITY + ROWS + [LONG] if c["plan"] == (0, 0)] + \
            [dict(R=3, n=300, heads=64, kv_heads=8, causal=True, plan=(0, 0))]


def case_id(c):
    return f"R{c['R']}-n{c['n']}-h{c['heads']}x{c['kv_heads']}-{'causal' if c['causal'] else 'full'}-s{c['plan'][0]}k{c['plan'][1]}"


def make_case(seed, rows, H, HKV, dtype, device, q_gain=1.0):
    """-> (qkv [rows, (H + 2 HKV) * 128], q [rows, H, 128] (a slice of it), cache [rows, 2 HKV, 128] e4m3, scale [2 HKV])."""
    import torch
    from mquant_amd import ops
    g = torch.Generator(device=device).manual_seed(seed)
    D = 128
    qkv = (torch.randn(rows, (H + 2 * HKV) * D, generator=g, device=device) * 0.8).to(dtype)
    qkv[:, :H * D] *= q_gain
    gain = torch.tensor([0.05, 1.0, 6.0, 20.0] * HKV, device=device)[:2 * HKV].repeat_interleave(D)
    qkv[:, H * D:] = (qkv[:, H * D:].float() * gain).to(dtype)
    q = qkv[:, :H * D].view(rows, H, D)
    kv = qkv[:, H * D:].view(rows, 2 * HKV, D)
    scale = ops.kv_scale_from_absmax(kv)
    cache = ops.kv_quant_fp8(kv, scale)
    return qkv, q, cache, scale
