#!/usr/bin/env python3
"""The two ends of a generation step at M = 1 -- logits -> token -> next hidden row -- over the two lm_head shapes of the supported
models (152064 x 3584, 92553 x 4096; the embedding table is the same tensor: only one of its rows is read), fp16 and bf16, as graph
replays in alternating rounds in this process (median and the range over the rounds):
  gemv:            mq_gemv_f16 alone, logits written;
  argmax +logits:  mq_gemv_f16_argmax alone (its GEMV launch and the merge), logits written;
  argmax:          the same with logits=None;
  (a) replaced:    gemv_f16 + torch.argmax + index_select of the embedding -- the host loop's path without its .item();
  (b) fused:       gemv_f16_argmax with logits + embed_gather;
  (c) fused, no logits.
The weights (1.09 GB / 0.76 GB) exceed every cache, so each replay streams them from HBM.  A measurement, not a gate.
usage (GPU box): python3 tools/decode_head_bench.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mquant_amd import ops  # noqa: E402

dev = torch.device("cuda:0")


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


def replay_time(graph, st, reps):
    with torch.cuda.stream(st):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            graph.replay()
        e1.record(st)
        st.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def alternating(fns, rounds=9, reps=20):
    """name -> (median, min, max) us per replay: every graph captured once, then timed round-robin"""
    graphs = {k: capture(fn) for k, fn in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, (graph, st) in graphs.items():
            times[k].append(replay_time(graph, st, reps))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}


def main():
    for N, K in ((152064, 3584), (92553, 4096)):
        for dtype in (torch.float16, torch.bfloat16):
            g = torch.Generator(device=dev).manual_seed(N + K)
            w = torch.empty((N, K), dtype=dtype, device=dev)
            for r0 in range(0, N, 16384):                             # filled in slices: no fp32 copy of the whole matrix
                w[r0:r0 + 16384] = (torch.randn((min(16384, N - r0), K), generator=g, device=dev) * 0.02).to(dtype)
            x = torch.randn((1, K), generator=g, device=dev).to(dtype)
            logits = torch.empty((1, N), dtype=dtype, device=dev)
            hidden = torch.empty((1, K), dtype=dtype, device=dev)
            tok = torch.zeros((1,), dtype=torch.int32, device=dev)

            def replaced():
                ops.gemv_f16(x, w, out=logits)
                torch.index_select(w, 0, torch.argmax(logits, dim=1), out=hidden)

            def fused(with_logits):
                ops.gemv_f16_argmax(x, w, logits=logits if with_logits else None, token_out=tok)
                ops.embed_gather(w, tok, out=hidden)

            res = alternating({
                "gemv": lambda: ops.gemv_f16(x, w, out=logits),
                "argmax +logits": lambda: ops.gemv_f16_argmax(x, w, logits=logits, token_out=tok),
                "argmax": lambda: ops.gemv_f16_argmax(x, w, token_out=tok),
                "(a) replaced": replaced,
                "(b) fused": lambda: fused(True),
                "(c) fused, no logits": lambda: fused(False),
            })
            want = int(torch.argmax(logits.float(), dim=1))
            assert int(tok) == want and torch.equal(hidden, w[want][None]), "the timed graphs disagree"
            name = f"{N} x {K} {'fp16' if dtype == torch.float16 else 'bf16'}"
            for k, (med, lo, hi) in res.items():
                print(f"{name}: {k:22s} {med:7.1f} us [{lo:.1f} .. {hi:.1f}]  ({N * K * 2 / med / 1e6:5.2f} TB/s of weight bytes)", flush=True)
            spread = res["gemv"][2] - res["gemv"][1]
            for k in ("argmax +logits", "argmax"):
                print(f"{name}: {k} - gemv = {res[k][0] - res['gemv'][0]:+.1f} us (gemv's range over the rounds: {spread:.1f} us)", flush=True)
            print(f"{name}: (a) - (b) = {res['(a) replaced'][0] - res['(b) fused'][0]:+.1f} us, (a) - (c) = "
                  f"{res['(a) replaced'][0] - res['(c) fused, no logits'][0]:+.1f} us", flush=True)
            del w, logits


if __name__ == "__main__":
    main()
