#!/usr/bin/env python3
"""Weight-group W4A8 GEMM at generation steps (M = 1, 8, 16 rows; groups of 128, symmetric and asymmetric, fp16 output): the streaming
kernel with the group fold (gemm_skinny.hip, tile 61) against the tiled kernel the same call took before it existed, and against the
per-channel GEMM of the shape -- the floor the fold pays against.  In the manner of tools/decode_gemm_bench.py: cold weights through 8
copies of the image (and of the group tables) per captured graph, device events around graph replays.  One process alternates

  (a) the call with tile 61 forced -- what the plan launches wherever it selects the streaming kernel (column `plan`);
  (b) the same call with the tiled kernel forced: the wave-specialised fold the plan names at 17 rows for symmetric groups, the round-1
      kernel (26) for asymmetric ones;
  (c) ops.gemm_w4a8 of the shape (per-channel scales),

three times over, and reports the median and the spread (max - min) of each.  `gain` says whether (a) beats (b) by more than the spread
of (a)'s three repetitions: the plan (wgroup_stream_gains, csrc/gemm_w4a8.hip) may select the streaming kernel for a shape class only
where it does.  Asymmetric groups: the mq_act_group_rowsum_i32 launch is in NEITHER timed call (the sums are taken once, in front).
hbm: the packed weights plus the scale table (and the int16 offsets) at 6.3 TB/s.
usage (GPU box): python3 tools/decode_wgroup_bench.py [--small] [--group G]   (--small adds the short reductions of a toy decoder and a
two-group call; --group: another group size than 128)"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mquant_amd import ops  # noqa: E402
from tools.decode_gemm_bench import graph_time  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = {"llm.qkv": (4608, 3584), "llm.o": (3584, 3584), "llm.gate_up": (37888, 3584), "llm.down": (3584, 19968)}
SMALL = {"toy.qkv": (1024, 512), "toy.gate_up": (2048, 512), "toy.down": (512, 1024), "k256": (4608, 256)}
COPIES, GROUP, REPS = 8, 128, 3


def main():
    global GROUP
    shapes = dict(SHAPES, **SMALL) if "--small" in sys.argv else SHAPES
    if "--group" in sys.argv:
        GROUP = int(sys.argv[sys.argv.index("--group") + 1])
    print(f"groups of {GROUP}", flush=True)
    ops.splitk_workspace(dev, 512 << 20)
    print(f"{'shape':12s} {'N':>6s} {'K':>6s} {'M':>3s} {'groups':>6s} | {'(a) stream':>16s} {'(b) tiled':>20s} {'(c) per-channel':>16s} | "
          f"{'hbm':>6s} {'a/b':>5s} {'a/c':>5s} gain plan   [us: median +- spread of {REPS}]", flush=True)
    for name, (N, K) in shapes.items():
        G = K // GROUP
        q = torch.randint(-8, 8, (N, K), dtype=torch.int8, device=dev)
        imgs = [ops.prepack(q, 4) for _ in range(COPIES)]
        tbls = [torch.rand((G, N), device=dev) * 0.01 + 0.001 for _ in range(COPIES)]
        offs = [torch.randint(-7, 9, (G, N), device=dev).to(torch.int16) for _ in range(COPIES)]
        s_w = torch.full((N,), 0.01, device=dev)
        for asym in (False, True):
            hbm_us = (N * K / 2 + G * N * (6 if asym else 4)) / 6.3e12 * 1e6
            for M in (1, 8, 16):
                a = ops.TiledAct.from_rows(torch.randint(-128, 128, (M, K), dtype=torch.int8, device=dev))
                sums = ops.act_group_rowsum(a, GROUP, G)
                out = torch.empty((M, N), dtype=torch.float16, device=dev)
                ops.gemm_debug_force(-1, 0)
                plan = ops.gemm_group_plan(M, N, K, GROUP, asym=asym)
                tiled = ops.gemm_group_plan(17, N, K, GROUP, asym=asym)

                def grouped(g):
                    if asym:
                        ops.gemm_w4a8_wgroupscale_asym(a, imgs[g], 4, N, tbls[g], offs[g], sums, GROUP, s_x0=0.02, out=out)
                    else:
                        ops.gemm_w4a8_wgroupscale(a, imgs[g], 4, N, tbls[g], GROUP, s_x0=0.02, out=out)
                t = {"a": [], "b": [], "c": []}
                for _ in range(REPS):
                    for key, force in (("a", 61), ("b", tiled), ("c", -1)):
                        try:
                            ops.gemm_debug_force(force, 0)
                            if key != "c":
                                assert ops.gemm_group_plan(M, N, K, GROUP, asym=asym) == force, (key, force)
                            t[key].append(graph_time(grouped if key != "c" else (lambda g: ops.gemm_w4a8(a, imgs[g], 4, N, 0.02, s_w, out=out)), COPIES))
                        finally:
                            ops.gemm_debug_force(-1, 0)
                med = {k: statistics.median(v) for k, v in t.items()}
                spr = {k: max(v) - min(v) for k, v in t.items()}
                gain = med["a"] + spr["a"] < med["b"]
                print(f"{name:12s} {N:6d} {K:6d} {M:3d} {'asym' if asym else 'sym':>6s} | {med['a']:8.2f} +- {spr['a']:5.2f} {med['b']:8.2f} +- {spr['b']:5.2f} ({tiled:2d}) "
                      f"{med['c']:8.2f} +- {spr['c']:5.2f} | {hbm_us:6.2f} {med['a'] / med['b']:5.2f} {med['a'] / med['c']:5.2f} {'yes' if gain else 'NO ':3s}  {plan:3d}", flush=True)


if __name__ == "__main__":
    main()
