#!/usr/bin/env python3
"""vision-tower attention: mq_attn_prefill (q / k / v read in place from the fused [T, q|k|v] tensor, [T, heads * D] out) against what a user
would otherwise run on the same tensors -- the permutes to [1, heads, T, D], torch SDPA, and the permute + copy back to [T, heads * D] -- in one
process, fp16 and bf16; median of 30 replays of a captured graph of 10 calls, us per call"""
import os, sys
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
torch.set_grad_enabled(False)
from mquant_amd import ops
dev = "cuda:0"

def timed(fn, iters=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(10):
            fn()
    g.replay(); torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 100.0)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]

for name, T, H, D in (("Qwen2-VL ViT", 1024, 16, 80), ("InternViT-300M", 1025, 16, 64), ("Qwen-VL ViT", 1024, 16, 104)):
    for dtype in (torch.float16, torch.bfloat16):
        qkv = torch.randn(T, 3 * H * D, device=dev).to(dtype)
        q, k, v = (qkv[:, i * H * D:(i + 1) * H * D].view(T, H, D) for i in range(3))
        out = torch.empty(T, H * D, device=dev, dtype=dtype)
        def sdpa():
            o = F.scaled_dot_product_attention(q.permute(1, 0, 2)[None], k.permute(1, 0, 2)[None], v.permute(1, 0, 2)[None])
            out.view(T, H, D).copy_(o[0].permute(1, 0, 2))
        a = timed(lambda: ops.attn_prefill(q, k, v, causal=False, out=out))
        mine = out.float().clone()
        b = timed(sdpa)
        err = float((mine - out.float()).abs().max() / out.float().abs().max())
        print(f"{name:15s} T={T:5d} H={H:3d} D={D:3d} {str(dtype)[6:]:9s}: mq_attn_prefill {a[0]:7.2f} us (min {a[1]:7.2f} max {a[2]:7.2f}) | "
              f"permute + SDPA + permute-copy {b[0]:7.2f} us (min {b[1]:7.2f} max {b[2]:7.2f}) | max difference / max {err:.1e}")
