#!/usr/bin/env python3
"""One decoder layer's hot path at generation shapes (M rows): the four quantize(+Hadamard) launches and the four W4A8 GEMMs of a Qwen2-VL-7B
layer (q|k|v, o_proj, gate|up, down_proj with its online Hadamard over 19968 padded channels), replayed from one hipGraph over 8 copies of
the weights (cold weights), and -- lines of their own, M <= 8 -- what sits between q|k|v and o_proj, three ways over the same e4m3 caches:
  append:        kv_quant_fp8 of the step's K|V rows into place + decode attention (no RoPE: the line of earlier reports);
  rope + append: rope_inplace on the M rows + kv_quant_fp8 + decode attention -- what a step with host-side positions launches;
  fused:         Fp8KVCache.advance (once per step) + kv_append_rope_fp8 + decode attention, the key count read on the device -- the
                 step that is captured once and replayed while the cache grows.
The three graphs are captured once and timed in alternating rounds in this process (median, and the range over the rounds).  The fused
graph runs with its device-side key count at the capacity, where the kernels clamp it: every round attends over the same N_KEYS keys as
the other two.  usage (GPU box): python3 tools/decode_step_bench.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fake_quant import hadamard_utils as hu  # noqa: E402
from mquant_amd import ops  # noqa: E402
from mquant_amd.full_prefill import _rope_tables  # noqa: E402
from mquant_amd.kv_cache import Fp8KVCache  # noqa: E402

dev = torch.device("cuda:0")
G = 8
N_KEYS = 4096     # keys in the cache at the timed step


def capture(fn):
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
    return graph, st


def replay_time(graph, st, reps=20):
    with torch.cuda.stream(st):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            graph.replay()
        e1.record(st)
        st.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def graph_time(fn, reps=20):
    return replay_time(*capture(fn), reps)


def alternating(fns, rounds=7, reps=20):
    """name -> (median, min, max) us per replay: every graph captured once, then timed round-robin"""
    graphs = {k: capture(fn) for k, fn in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (graph, st) in graphs.items():
            times[k].append(replay_time(graph, st, reps))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}


def main():
    ops.splitk_workspace(dev, 512 << 20)
    shapes = {"qkv": (4608, 3584), "o": (3584, 3584), "gate_up": (37888, 3584), "down": (3584, 19968)}
    imgs = {k: [ops.prepack(torch.randint(-8, 8, (n, kk), dtype=torch.int8, device=dev), 4) for _ in range(G)] for k, (n, kk) in shapes.items()}
    s_w = {k: torch.full((n,), 0.01, device=dev) for k, (n, _) in shapes.items()}
    _, K = hu.get_hadK(19968)
    bits = hu.had_sign_bits(K, dev)
    kv_scale = torch.full((8,), 0.01, device=dev)
    cos, sin = (t[:, 0].contiguous() for t in _rope_tables(N_KEYS, 128, dev, torch.float16))
    kvc = Fp8KVCache(G, N_KEYS, 4, 128, [kv_scale] * G, cos, sin, dev, torch.float16)
    caches = kvc.caches                      # one cache per weight copy; the three attention lines read and write the same ones
    for c in caches:
        c.view(torch.uint8).copy_(torch.randn((N_KEYS, 8, 128), device=dev).mul_(100).clamp_(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
    for M in (1, 4, 16, 64):
        x = torch.randn((M, 3584), device=dev, dtype=torch.float16)
        xd = torch.randn((M, 18944), device=dev, dtype=torch.float16)
        a3584 = ops.TiledAct.empty(M, 3584, dev)
        a_down = ops.TiledAct.empty(M, 19968, dev)
        outs = {k: torch.empty((M, n), dtype=torch.float16, device=dev) for k, (n, _) in shapes.items()}

        def quant_only():
            for g in range(G):
                for _ in range(3):
                    ops.quantize_act_i8(x, 0.05, out=a3584)
                ops.hadamard_quant_i8(xd, 19968, K, bits, 0.05, out=a_down)

        def gemm_only():
            for g in range(G):
                for k in ("qkv", "o", "gate_up"):
                    ops.gemm_w4a8(a3584, imgs[k][g], 4, shapes[k][0], 0.02, s_w[k], out=outs[k])
                ops.gemm_w4a8(a_down, imgs["down"][g], 4, 3584, 0.02, s_w["down"], out=outs["down"])

        def layer():
            for g in range(G):
                for k in ("qkv", "o", "gate_up"):
                    ops.quantize_act_i8(x, 0.05, out=a3584)
                    ops.gemm_w4a8(a3584, imgs[k][g], 4, shapes[k][0], 0.02, s_w[k], out=outs[k])
                ops.hadamard_quant_i8(xd, 19968, K, bits, 0.05, out=a_down)
                ops.gemm_w4a8(a_down, imgs["down"][g], 4, 3584, 0.02, s_w["down"], out=outs["down"])
        tq, tg, tl = graph_time(quant_only) / G, graph_time(gemm_only) / G, graph_time(layer) / G
        print(f"M={M:3d}: quantizers + Hadamard {tq:6.1f} us | GEMMs {tg:6.1f} us | layer (8 launches + reduces) {tl:6.1f} us "
              f"-> {28 * tl / 1e3:5.2f} ms per token-step of 28 layers (weights alone at 6.3 TB/s: 0.53 ms)", flush=True)
        if M <= 8:
            # what sits between q|k|v and o_proj: the cache append (the step's K|V rows quantized into place) and the decode attention of the
            # M newest positions over the e4m3 cache, one cache per weight copy
            kv_new = outs["qkv"][:, 3584:].view(M, 8, 128)
            qk_new = outs["qkv"][:, :3584 + 512]
            q_new = outs["qkv"][:, :3584].view(M, 28, 128)
            attn_out = torch.empty((M, 3584), dtype=torch.float16, device=dev)
            cos_m, sin_m = cos[N_KEYS - M:N_KEYS].contiguous(), sin[N_KEYS - M:N_KEYS].contiguous()

            def append():
                for g in range(G):
                    ops.kv_quant_fp8(kv_new, kv_scale, out=caches[g][N_KEYS - M:N_KEYS])
                    ops.attn_decode_fp8kv(q_new, caches[g], kv_scale, out=attn_out)

            def rope_append():
                for g in range(G):
                    ops.rope_inplace(qk_new, 32, 128, cos_m, sin_m)
                    ops.kv_quant_fp8(kv_new, kv_scale, out=caches[g][N_KEYS - M:N_KEYS])
                    ops.attn_decode_fp8kv(q_new, caches[g], kv_scale, out=attn_out)

            def fused():
                kvc.advance(M)
                for g in range(G):
                    kvc.step(g, outs["qkv"], 28, out=attn_out)

            kvc.set_length(N_KEYS)
            res = alternating({"append": append, "rope + append": rope_append, "fused": fused})
            what = {"append": "cache append + decode attention", "rope + append": "rope_inplace + cache append + decode attention",
                    "fused": "advance + fused rope/append (device key count) + decode attention"}
            for k, (med, lo, hi) in res.items():
                print(f"M={M:3d}: {what[k]} over {N_KEYS} keys (e4m3 cache, 28 / 4 heads) {med / G:6.1f} us [{lo / G:.1f} .. {hi / G:.1f}] "
                      f"-> {28 * med / G / 1e3:5.2f} ms per token-step of 28 layers", flush=True)

if __name__ == "__main__":
    main()
