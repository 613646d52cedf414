#!/usr/bin/env python3
"""Decode attention over the e4m3 KV cache (mq_attn_decode_fp8kv) against the path it replaces -- kv_dequant_fp8 -> repeat_interleave ->
torch SDPA, which writes a 16-bit copy of the whole cache to HBM and reads it back -- at the generation step (R = 1) of the Qwen2-VL-7B
(28 / 4 heads) and -72B (64 / 8) geometries, n in {768, 4096, 32768} keys, fp16 and bf16.  Both are captured into one hipGraph each that
walks over COPIES of the cache (a layer's cache is not the one the previous launch left in the caches: 28 or 80 layers take their turn
in a real step; the copies here add up to 512 MiB where 64 of them suffice, else 64 copies: the small shapes stay resident in the
Infinity Cache either way) and timed per replay with events; the figure is the MEDIAN of the replays divided by the number of copies.
bytes: what the kernel must move -- the n keys' K and V bytes once, q and the output -- divided by its time.
Beside it the same kernel over a 16-BIT cache (mq_attn_decode; the reference's default k_bits = v_bits = 16) holding the same values:
twice the bytes per key under the same plan, against ITS baseline -- repeat_interleave -> SDPA over the 16-bit cache, what HF does.
usage (GPU box): python3 tools/decode_attn_bench.py [--reps 30]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mquant_amd import ops  # noqa: E402

dev = torch.device("cuda:0")


def graph_median_us(fn, reps):
    """median over `reps` replays of the graph that holds fn(), in microseconds"""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st, capture_error_mode="thread_local"):
            fn()
        for _ in range(3):
            graph.replay()
        st.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record(st)
        for i in range(reps):
            graph.replay()
            ev[i + 1].record(st)
        st.synchronize()
    return statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(reps)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    print(f"{'geometry':>9} {'dtype':>5} {'n':>6} {'plan':>10} {'copies':>6} | {'decode us':>9} {'TB/s':>6} | {'dequant+SDPA us':>15} | ratio "
          f"|| {'kv16 us':>8} {'TB/s':>6} {'/ e4m3':>6} | {'SDPA us':>8} | ratio", flush=True)
    for H, HKV in ((28, 4), (64, 8)):
        rep = H // HKV
        for dtype in (torch.float16, torch.bfloat16):
            for n in (768, 4096, 32768):
                row = 2 * HKV * 128
                copies = max(1, min(64, (512 << 20) // (n * row)))
                kv = torch.randn((n, 2 * HKV, 128), device=dev, dtype=dtype)
                scale = ops.kv_scale_from_absmax(kv)
                caches = [ops.kv_quant_fp8(torch.randn((n, 2 * HKV, 128), device=dev, dtype=dtype), scale) for _ in range(copies)]
                caches16 = [ops.kv_dequant_fp8(c, scale, dtype) for c in caches]      # the same values at two bytes each
                q = torch.randn((1, H, 128), device=dev, dtype=dtype)
                out = torch.empty((1, H * 128), device=dev, dtype=dtype)
                kvd = torch.empty((n, 2 * HKV, 128), device=dev, dtype=dtype)
                qs = q.permute(1, 0, 2)[None]
                plan = ops.attn_decode_plan(1, n, H, HKV)

                def decode():
                    for c in caches:
                        ops.attn_decode_fp8kv(q, c, scale, out=out)

                def replaced():
                    for c in caches:
                        ops.kv_dequant_fp8(c, scale, dtype, out=kvd)
                        k = kvd[:, :HKV].repeat_interleave(rep, 1).permute(1, 0, 2)[None]
                        v = kvd[:, HKV:].repeat_interleave(rep, 1).permute(1, 0, 2)[None]
                        F.scaled_dot_product_attention(qs, k, v, is_causal=False)

                def decode16():
                    for c in caches16:
                        ops.attn_decode(q, c, out=out)

                def replaced16():
                    for c in caches16:
                        k = c[:, :HKV].repeat_interleave(rep, 1).permute(1, 0, 2)[None]
                        v = c[:, HKV:].repeat_interleave(rep, 1).permute(1, 0, 2)[None]
                        F.scaled_dot_product_attention(qs, k, v, is_causal=False)

                t_new = graph_median_us(decode, args.reps) / copies
                t_old = graph_median_us(replaced, args.reps) / copies
                t_new16 = graph_median_us(decode16, args.reps) / copies
                t_old16 = graph_median_us(replaced16, args.reps) / copies
                moved = n * row + 2 * H * 128 * 2
                moved16 = 2 * n * row + 2 * H * 128 * 2
                print(f"{H:>5}/{HKV:<3} {'fp16' if dtype == torch.float16 else 'bf16':>5} {n:>6} "
                      f"{plan['splits']:>4}x{plan['keys_per_split']:<5} {copies:>6} | {t_new:>9.2f} {moved / t_new / 1e6:>6.2f} | {t_old:>15.2f} | "
                      f"{t_old / t_new:>5.1f}x{'' if t_new < t_old else '  SLOWER THAN THE PATH IT REPLACES'} "
                      f"|| {t_new16:>8.2f} {moved16 / t_new16 / 1e6:>6.2f} {t_new16 / t_new:>5.2f}x | {t_old16:>8.2f} | "
                      f"{t_old16 / t_new16:>5.1f}x{'' if t_new16 < t_old16 else '  SLOWER THAN SDPA'}", flush=True)
                del caches, caches16, kv, kvd
    print("stream rate for comparison: mq_gemv_f16 reaches 6.8 TB/s on the lm_head weights", flush=True)


if __name__ == "__main__":
    main()
