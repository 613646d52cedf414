#!/usr/bin/env python3
"""What sits between q|k|v and o_proj in a generation step, for B sequences: (a) B single-sequence append + decode attention pairs
back to back (``ops.kv_append_rope*`` + ``ops.attn_decode*`` on each sequence's cache, its key count and RoPE offset read on the
device) against (b) ONE batched pair (``Fp8KVCacheBatch.step`` / ``KVCache16Batch.step``) over the same caches.  Per geometry (28 / 4
and 64 / 8 heads), cache length (768, 4096, 32768 keys), storage (e4m3, 16-bit) and B = 1, 2, 4, 8; G layers' worth of caches per
graph.  Both graphs are captured once and timed in alternating rounds in this process: medians and the range over the rounds, per
layer.  The key counts stand at the capacity, where the kernels clamp them: every round attends over the same keys.
usage (GPU box): python3 tools/decode_batch_bench.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mquant_amd import ops  # noqa: E402
from mquant_amd.full_prefill import _rope_tables  # noqa: E402
from mquant_amd.kv_cache import Fp8KVCacheBatch, KVCache16Batch  # noqa: E402
from tools.decode_step_bench import alternating  # noqa: E402

dev = torch.device("cuda:0")
G = 4
D = 128


def main():
    dtype = torch.float16
    for heads, kv_heads in ((28, 4), (64, 8)):
        for n_keys in (768, 4096, 32768):
            cos, sin = (t[:, 0].contiguous() for t in _rope_tables(n_keys, D, dev, dtype))
            for storage in ("e4m3", "16-bit"):
                for B in (1, 2, 4, 8):
                    scale = torch.full((2 * kv_heads,), 0.01, device=dev)
                    if storage == "e4m3":
                        kvc = Fp8KVCacheBatch(B, G, n_keys, kv_heads, D, [scale] * G, cos, sin, dev, dtype, rope_delta=[0] * B)
                    else:
                        kvc = KVCache16Batch(B, G, n_keys, kv_heads, D, cos, sin, dev, dtype, rope_delta=[0] * B)
                    for c in kvc.caches:
                        c.view(torch.uint8).copy_(torch.randn(c.shape, device=dev).clamp_(-4, 4).to(c.dtype).view(torch.uint8))
                    kvc.set_length([n_keys] * B)
                    qkv = torch.randn((B, (heads + 2 * kv_heads) * D), device=dev, dtype=dtype)
                    out = torch.empty((B, heads * D), dtype=dtype, device=dev)

                    def singles():
                        kvc.advance(1)
                        for g in range(G):
                            for b in range(B):
                                row, n, d = qkv[b:b + 1], kvc.n_keys[b:b + 1], kvc.rope_delta[b:b + 1]
                                q = row[:, :heads * D].view(1, heads, D)
                                if storage == "e4m3":
                                    ops.kv_append_rope_fp8(row, heads, kvc.caches[g][b], scale, cos, sin, n_keys=n, rope_delta=d)
                                    ops.attn_decode_fp8kv(q, kvc.caches[g][b], scale, n_keys=n, out=out[b:b + 1])
                                else:
                                    ops.kv_append_rope(row, heads, kvc.caches[g][b], cos, sin, n_keys=n, rope_delta=d)
                                    ops.attn_decode(q, kvc.caches[g][b], n_keys=n, out=out[b:b + 1])

                    def batched():
                        kvc.advance(1)
                        for g in range(G):
                            kvc.step(g, qkv, heads, out=out)

                    res = alternating({"singles": singles, "batched": batched})
                    plan = ops.attn_decode_batch_plan(B, 1, n_keys, heads, kv_heads)
                    (sm, sl, sh), (bm, bl, bh) = res["singles"], res["batched"]
                    print(f"{heads:2d}/{kv_heads} heads, {n_keys:5d} keys, {storage:6s}, B={B}: {B} single pairs {sm / G:7.1f} us [{sl / G:.1f} .. {sh / G:.1f}]"
                          f" | one batched pair {bm / G:7.1f} us [{bl / G:.1f} .. {bh / G:.1f}] ({plan['splits']} x {plan['keys_per_split']} keys,"
                          f" {plan['grid']} workgroups) -> x{sm / bm:.2f}", flush=True)
                    del kvc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
