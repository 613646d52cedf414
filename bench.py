#!/usr/bin/env python3
"""Headline benchmark: W4A8 prefill tokens/s of the hot path on the Qwen2-VL-7B workload
(1 x 448^2 image + 512-token prompt => 1024 vision tokens, 768 LLM positions).

A "step" is one pass of the hot path over one image+prompt: every wrapped Linear of the
prefill (ViT 32 blocks x 4 + patch_embed + merger x 2, LLM 28 layers x 7 = 327 Linears), each
as [online Hadamard +] static int8 quantize -> int8 x int4 MFMA GEMM with fused dequant,
inputs resident in HBM.  Attention, norms, RoPE and lm_head are outside the path (SURVEY.md
section 8) and are not executed.  Weights are random with the real shapes; data is synthetic.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints the line (metric, value, unit, ms_per_step, ...).
--dump-outputs DIR: what the last timed step returned (the last Linear's output, the logits) as DIR/<name>.npy, float32.
--full: also the measurements and checks beyond the headline figure -- kernel attribution and roofline (sustained int8
peak, floor model), whole-prefill TTFT, CPU baselines, the secondary configurations, the multi-rank logits checks.
N > 1: one rank per GPU over RCCL.  Started under torch.distributed.run (the driver's command) the
process is a rank; started plainly with --gpus N it spawns the N ranks itself as FRESH child
processes (before anything touches the GPU) and returns their exit code.  Every rank prefills its
own image+prompt sample (batch sharding, sample i -> rank i % N, weak scaling); the ranks exchange
their real last-token logits with one RCCL all_gather per step, and (--full) rank 0 checks the gathered
logits against its own single-GPU computation of every sample.  Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_INT8_TOPS = 5000.0   # dense int8 MFMA, 2 x the 2.5 PF bf16 dense peak (MI355X_MICROARCH.md)
VOCAB = 152064
VOCABS = {"qwen2vl_7b": 152064, "qwen2vl_72b": 152064, "qwenvl_7b": 151936, "internvl2_8b": 92553}   # lm_head rows (public configs)


def cpu_baseline_reference(budget_s: float = 40.0):
    """The reference's CPU path timed on the host cores: this repository's ``fake_quant`` package in
    its SIMULATED mode (fp32 torch ops on fake-quantized tensors, pinned to the reference's forward by
    the goldens of tests/test_fake_quant_cpu.py / test_gpu_wrapper_golden.py), CPU tensors,
    torch.set_num_threads(all cores), the full row count, ONE instance of each of the 14 layer shapes
    including zero pad + matmul_hadU + split; scaled by the instance counts to one prefill."""
    import functools
    import torch
    from fake_quant import hadamard_utils as hu, quant_utils as qu, utils as fq_utils
    from fake_quant.gptq.rtn import rtn_module
    from mquant_amd import workload

    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    torch.set_grad_enabled(False)
    class A:
        skip_names = []

    def build(sp, seed):
        g = torch.Generator().manual_seed(seed)
        lin = torch.nn.Linear(sp.k, sp.n, bias=sp.bias)
        lin.weight.data = torch.randn((sp.n, sp.k), generator=g) * 0.02
        wrap = qu.ActQuantWrapper(lin)
        if sp.had_K:
            hadK, Kh = hu.get_hadK(sp.k)
            wrap.online_full_had, wrap.had_K, wrap.K = True, hadK, Kh
        if sp.split:
            wrap.split = True
            wrap.split_weights()
        if sp.k != sp.k_in:
            wrap.register_forward_pre_hook(functools.partial(fq_utils.revise_down_input, new_size=sp.k))
        rtn_module(wrap, "layer", 4, True, False, [], {})
        wrap.real_quant = False                       # the simulated (reference) evaluation, not the HIP backend
        wrap.simulate_on_cpu = True                   # explicit opt-in: the wrapper has no CPU fallback of its own
        wrap.quantizer.configure(bits=8, sym=True, static=True, observer_type="minmax")
        x = torch.randn((sp.M, sp.k_in), generator=g)
        qu.calib_layer(wrap, [x[: min(sp.M, 64)]], A())
        wrap(x[:8])                                   # first-call setup outside the timing
        return wrap, x

    specs = workload.qwen2vl_7b_specs(msq=False)
    # "all cores" is not the fastest setting on a many-core host (the elementwise ops of the simulated path
    # and the affinity mask of a container over-subscribe): time the wrapper itself (the o_proj shape) at a
    # few thread counts and use the best one; ``cores`` reports the threads actually used
    probe = next((sp for sp in specs if sp.name == "llm.o_proj"), specs[0])
    wrap, x = build(probe, 99)
    best, cores = None, 1
    for t in sorted({c for c in (8, 16, 32, 64, 128) if c <= avail} | ({avail} if avail < 8 else set())):
        torch.set_num_threads(t)
        wrap(x)
        t0 = time.perf_counter()
        wrap(x)
        wrap(x)
        dt = time.perf_counter() - t0
        if best is None or dt < best:
            best, cores = dt, t
        elif dt > 1.5 * best:
            break                                    # past the knee: more threads only over-subscribe
    torch.set_num_threads(cores)
    del wrap, x

    t_begin = time.perf_counter()
    est, measured, detail, skipped = 0.0, 0.0, [], []
    for sp in specs:
        if time.perf_counter() - t_begin > budget_s:
            skipped.append(sp.name)
            continue
        wrap, x = build(sp, len(detail))
        reps, t0 = 0, time.perf_counter()
        while reps < 8 and (reps == 0 or time.perf_counter() - t0 < 1.0):   # ~1 s per shape, 10-20 s in all
            wrap(x)
            reps += 1
        spent = time.perf_counter() - t0
        dt = spent / reps
        measured += spent
        est += dt * sp.count
        detail.append(f"{sp.name} {dt * 1e3:.0f} ms x{sp.count}")
        del wrap, x
    if skipped:      # bounded run: the shapes not reached are charged at the measured seconds per op
        done_ops = sum(2.0 * sp.M * sp.k * sp.n * sp.count for sp in workload.qwen2vl_7b_specs(msq=False) if sp.name not in skipped)
        all_ops = sum(2.0 * sp.M * sp.k * sp.n * sp.count for sp in workload.qwen2vl_7b_specs(msq=False))
        est *= all_ops / done_ops
    return {"value": round(768.0 / est, 3), "unit": "tokens/s", "cores": cores, "kind": "reference",
            "sample": f"fake_quant simulated ActQuantWrapper.forward (== reference, pinned by goldens) on CPU fp32 tensors, "
                      f"torch {cores} threads, full rows, one instance per layer shape, {measured:.1f} s measured, scaled by "
                      f"instance count to the 327-Linear prefill ({est:.1f} s per prefill)"
                      + (f"; not reached within the time budget and charged pro rata by ops: {', '.join(skipped)}" if skipped else "")
                      + "; " + ", ".join(detail)}


def cpu_baseline(prefill_ops_total: float):
    """Time the CPU oracle ("port" of the reference's fake-quant path, integer form) on a
    bounded sample: one LLM layer's 7 Linears restricted to 256 of the 768 rows."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import oracle
    from golden_inputs import make_w, make_x

    rows = 256
    t = np.load(os.path.join(ROOT, "tests", "golden", "hadk_table.npz"))
    hk = np.unpackbits(t["had156"])[: 156 * 156].reshape(156, 156).astype(np.int8) * 2 - 1
    shapes = [(3584, 3584, 3584, 0), (3584, 3584, 512, 0), (3584, 3584, 512, 0),
              (3584, 3584, 3584, 0), (3584, 3584, 18944, 0), (3584, 3584, 18944, 0),
              (18944, 19968, 3584, 156)]
    prepared = []
    pool = np.random.RandomState(950).randint(-8, 8, size=19968 * 3584 + 8 * 19968, dtype=np.int8)
    for i, (k_in, k, n, hK) in enumerate(shapes):
        x = make_x(900 + i, (rows, k_in))
        w = pool[i * 19968: i * 19968 + n * k].reshape(n, k)   # untimed preparation
        s_w = np.full((n,), 0.003, dtype=np.float32)
        prepared.append((x, w, s_w, k, hK))
    ops_sample, reps = 0.0, 0
    t0 = time.perf_counter()
    while reps < 16 and (reps == 0 or time.perf_counter() - t0 < 5.0):      # ~5 s of CPU work
        for x, w, s_w, k, hK in prepared:
            if hK:
                x = oracle.hadamard(x, k, hK, hk, mid_round=1, out_round=1)
            q = oracle.quant_static(x, np.float32(0.05))
            acc = oracle.gemm_i32(q, w)
            oracle.epilogue(acc, np.float32(0.05), s_w)
            ops_sample += 2.0 * rows * k * w.shape[0]
        reps += 1
    dt = time.perf_counter() - t0
    est_step = dt * prefill_ops_total / ops_sample
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return {"value": round(768.0 / est_step, 3), "unit": "tokens/s", "cores": cores, "kind": "port",
            "sample": f"oracle/mq_oracle.c (OpenMP, {cores} threads): LLM layer 0, 7 Linears incl. "
                      f"pad+Hadamard(156x128)+quant, {rows} of 768 rows, {reps} repetition(s), {dt:.1f} s measured; "
                      f"extrapolated by GEMM ops to the full 327-Linear prefill"}


def full_prefill_report(pf, dev, args, geometry=None, kv_fp8=False, attn_fp8=False, variants=True):
    """TTFT of the WHOLE synthetic prefill -- the W4A8 Linears chained through
    torch glue (RMS norm, RoPE, SDPA, activations, fp16 lm_head on the last position) -- one
    hipGraph replay per sample, HIP events around each replay.  Secondary to ``value``.
    ``variants`` = False: the fused form only (the secondary lines' budget)."""
    import torch
    from mquant_amd import workload
    from mquant_amd.full_prefill import FullPrefill
    try:
        def measure(fused, rope_fused=True, act_in_gemm=True):
            fp = FullPrefill(pf, fused_glue=fused, geometry=geometry, kv_fp8=kv_fp8, attn_fp8=attn_fp8)
            fp.rope_fused = fused and rope_fused          # the decoder's RoPE in the q|k|v GEMM's store (round 5) or its own launch
            fp.act_in_gemm = fused and act_in_gemm        # silu(gate)*up / QuickGELU in the producing GEMM's store (round 6) or in the Hadamard kernel's prologue
            fp.calibrate()
            if args.no_graph:
                run = fp.step
            else:
                fp.step()
                torch.cuda.synchronize(dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    fp.step()
                run = g.replay
            for _ in range(20):
                run()
            torch.cuda.synchronize(dev)
            times = []
            for _ in range(max(args.ttft_iters, 5)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            times.sort()
            med = times[len(times) // 2]
            p90 = times[min(len(times) - 1, int(round(0.9 * (len(times) - 1))))]
            return med, p90, len(times), bool(torch.isfinite(fp.logits.float()).all().item())
        if not variants:
            med, p90, iters, finite = measure(True)
            return {"what": "whole synthetic prefill, fused glue" + (", fp8 (e4m3) KV cache written by the q|k|v GEMM's consumers and READ by the "
                            "prefill attention (mq_attn_prefill_fp8kv)" if kv_fp8 and attn_fp8 else ""),
                    "ttft_ms_median": round(med, 4), "ttft_ms_p90": round(p90, 4), "iters": iters, "kv_fp8": bool(kv_fp8),
                    "attn_fp8": bool(attn_fp8), "llm_tokens_per_s": round(workload.M_LLM / (med * 1e-3), 1), "logits_finite": finite}
        med_u, p90_u, _, _ = measure(False)
        med, p90, iters, finite = measure(True)
        med_rope = measure(True, rope_fused=False)[0]     # same process, same box: what the separate RoPE launch costs
        med_actp = measure(True, act_in_gemm=False)[0]    # same process, same box: round 5's form of the activations
        # informational: the same prefill with the NON-DEFAULT fast Hadamard stage (K x K stage on the half-precision matrix
        # core; ~1e-7 of the int8 levels differ from the exact kernel -- DESIGN 4.2).  The flag lives in the layer descriptors
        # of THIS model object (workload.set_had_fast); it is cleared again before returning, and nothing process-wide exists.
        med_fast = None
        try:
            pf.set_had_fast(True)
            try:
                med_fast = measure(True)[0]
            finally:
                pf.set_had_fast(bool(args.had_fast))
        except Exception:
            med_fast = None
        return {"what": "whole synthetic prefill: W4A8 Linears (this repo's kernels) + attention (mq_attn_prefill on the q|k|v GEMM "
                        "outputs in place: decoder head_dim 128 causal, vision tower head_dim 80) and fp16 lm_head on the last position; "
                        "RMS norm -> quantize, residual adds (GEMM epilogue), SiLU*up / QuickGELU (in the store of the PRODUCING gate|up / fc1 "
                        "GEMM, mq_gemm_w4a8_act_ws: down_proj / fc2 then run their plain Hadamard -> quantize launch) and "
                        "RoPE (the decoder's in the q|k|v GEMM's store, the vision tower's as one in-place launch) run fused; "
                        "ttft_ms_median_act_in_hadamard_prologue = the same with the activations in the Hadamard kernel's prologue (round 5's form); "
                        "ttft_ms_median_unfused_glue = the same dataflow with those steps as separate torch ops and torch SDPA everywhere; "
                        "ttft_ms_median_rope_as_its_own_launch = fused glue with the decoder's RoPE launched separately (round 4's form)",
                "ttft_ms_median": round(med, 4), "ttft_ms_p90": round(p90, 4), "iters": iters,
                "ttft_ms_median_unfused_glue": round(med_u, 4), "ttft_ms_p90_unfused_glue": round(p90_u, 4),
                "ttft_ms_median_rope_as_its_own_launch": round(med_rope, 4),
                "ttft_ms_median_act_in_hadamard_prologue": round(med_actp, 4),
                "ttft_ms_median_fast_hadamard_NON_DEFAULT": None if med_fast is None else round(med_fast, 4),
                "llm_tokens_per_s": round(workload.M_LLM / (med * 1e-3), 1),
                "all_tokens_per_s": round((workload.M_LLM + workload.M_VIS) / (med * 1e-3), 1),
                "logits_finite": finite}
    except Exception as exc:      # a report, never a reason to lose the bench line
        return {"error": repr(exc)}



#: the other BASELINE.json configurations and the reference's FIRST canonical command (docs/qwen2vl.md:19: W8A8 vision tower +
#: W4A8 LLM), run as bounded CHILD processes behind the headline so that the driver's one bench line carries them
#: (VERDICT r5 "next" 3).  name -> (extra command line, what it is)
SECONDARY = {
    "qwenvl_7b": (["--workload", "qwenvl_7b"], "BASELINE config 2: Qwen-VL-7B W4A8 full prefill Linears, online Hadamard 172x64 + 2^13"),
    "internvl2_8b_batch4": (["--workload", "internvl2_8b", "--batch", "4"],
                            "BASELINE config 4, the per-GPU share of batch 32 over 8 GPUs: InternVL2-8B W4A8, 4 samples per step"),
    "qwen2vl_72b_kv_fp8": (["--workload", "qwen2vl_72b", "--ttft-kv-fp8"],
                           "BASELINE config 5 on ONE GPU: Qwen2-VL-72B W4A8 MSQ (35.8 GB of W4) + whole-prefill TTFT with the fp8 KV cache"),
    "qwen2vl_7b_visual_w8": (["--workload", "qwen2vl_7b", "--visual-w-bits", "8"],
                             "the reference's first canonical command (docs/qwen2vl.md:19): W8A8 vision tower + W4A8 LLM, Qwen2-VL-7B"),
}


def run_secondary(budget_s: float, t_start: float, steps: int = 10, warmup: int = 3):
    """Each entry of SECONDARY as a fresh child process (its own GPU context; a crash, a hang or an out-of-memory kill costs
    that entry only), bounded by what is left of ``budget_s`` since ``t_start``.  Returns name -> compact summary."""
    out = {}
    for name, (extra, what) in SECONDARY.items():
        left = budget_s - (time.perf_counter() - t_start)
        if left < 30.0:
            out[name] = {"what": what, "skipped": f"time budget spent ({budget_s:.0f} s for the whole bench)"}
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(steps), "--warmup", str(warmup), "--full", "--no-cpu-baseline",
               "--no-secondary"] + (["--no-full-prefill"] if "--ttft-kv-fp8" not in extra else []) + extra
        t0 = time.perf_counter()
        try:
            env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
            proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, start_new_session=True)
            try:
                so, se = proc.communicate(timeout=left - 10.0)
            except subprocess.TimeoutExpired:
                os.killpg(proc.pid, 9)                      # the exact process group this call started
                proc.communicate()
                out[name] = {"what": what, "error": f"timed out after {time.perf_counter() - t0:.0f} s"}
                continue
            js = [ln for ln in so.splitlines() if ln.startswith("{")]
            if proc.returncode != 0 or not js:
                out[name] = {"what": what, "error": f"rc {proc.returncode}: {se.strip().splitlines()[-1] if se.strip() else 'no output'}"}
                continue
            d = json.loads(js[-1])
            r = d.get("roofline", {})
            ent = {"what": what, "value": d.get("value"), "unit": d.get("unit"), "ms_per_step": d.get("ms_per_step"),
                   "frac": r.get("frac"), "step_frac": r.get("step_frac"), "gemm_ms_per_step": r.get("gemm_ms_per_step"),
                   "quant_hadamard_ms_per_step": r.get("quant_hadamard_ms_per_step"),
                   "gemm_TOP_per_step": d.get("config", {}).get("gemm_TOP_per_step"), "weights_GB": d.get("config", {}).get("weights_GB"),
                   "steps": d.get("steps"), "path": d.get("config", {}).get("path"), "wall_s": round(time.perf_counter() - t0, 1),
                   "command": "python bench.py " + " ".join(cmd[2:])}
            if "full_prefill_kv_fp8" in d:
                ent["full_prefill_kv_fp8"] = d["full_prefill_kv_fp8"]
            out[name] = ent
        except Exception as exc:      # a report, never a reason to lose the bench line
            out[name] = {"what": what, "error": repr(exc)}
    return out


def sustained_int8_peak(pf, dev):
    """The dense int8 matrix rate THIS box sustains under its package power limit on the benchmark's own operand bytes
    (mq_bench_mfma_burn, csrc/bench_probe.hip -> libmquant_bench.so, bench-only: register-only MFMA chains on every CU, no memory traffic).  The GEMM family runs
    at the power limit -- the same launch is 10-30 % slower on real operand bytes than on zeros,
    profiles/r5_clock_reconciliation.txt -- so this, not the nominal 5 POP/s at 2.4 GHz, is what the matrix cores can deliver here.
    Reported beside the nominal peak; the nominal stays the denominator of ``frac``."""
    import ctypes
    import torch
    from mquant_amd import _lib, ops
    L = max(pf.layers, key=lambda l: l.lin.gemm_ops(l.spec.M))           # the dominant launch (gate|up)
    a, _ = L.lin.quantize(L.x, L.row_sel)
    a_bytes = (a.data if isinstance(a, ops.TiledAct) else a).reshape(-1)[: 4 * 1024].contiguous().view(torch.int32)
    words = L.lin.w_img.reshape(-1)[: 2 * 1024].contiguous().view(torch.int32)
    w_bytes = torch.stack(((words << 4) & -0x0F0F0F10, words & -0x0F0F0F10), dim=1).reshape(-1)   # the two nibble planes, high nibble
    operands = torch.cat((a_bytes, w_bytes)).contiguous()
    assert operands.numel() == 8 * 64 * 4
    sink = torch.zeros(4, dtype=torch.int32, device=dev)
    out = {}
    for kind, name in ((1, "mfma_i32_16x16x64_i8"), (0, "mfma_i32_32x32x32_i8")):
        rate = ctypes.c_double(0.0)
        _lib.call_bench("mq_bench_mfma_burn", kind, operands.data_ptr(), 2000, 60, sink.data_ptr(), ctypes.addressof(rate), ops._stream())
        out[name] = round(rate.value / 1e12, 1)
    zeros = torch.zeros_like(operands)
    rate = ctypes.c_double(0.0)
    _lib.call_bench("mq_bench_mfma_burn", 1, zeros.data_ptr(), 2000, 60, sink.data_ptr(), ctypes.addressof(rate), ops._stream())
    out["mfma_i32_16x16x64_i8_all_zero_operands"] = round(rate.value / 1e12, 1)
    return out

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--tiny", action="store_true", help="small shapes (debug only; not a valid bench line)")
    ap.add_argument("--no-graph", action="store_true", help="launch kernels one by one instead of replaying a hipGraph")
    ap.add_argument("--no-fuse", action="store_true", help="one GEMM per Linear (no q/k/v, gate/up fusion)")
    ap.add_argument("--direct-engines", action="store_true",
                    help="assemble the integer engines directly (workload.Prefill) instead of building the prefill THROUGH the "
                         "drop-in API (module tree -> add_actquant -> RTN -> calibration protocol -> model_quant -> "
                         "ActQuantWrapper.forward), which is the default for the Qwen2-VL-7B workload")
    ap.add_argument("--via-wrappers", action="store_true", help="(default for qwen2vl_7b; kept for explicit command lines)")
    ap.add_argument("--workload", default="qwen2vl_7b", choices=["qwen2vl_7b", "qwenvl_7b", "internvl2_8b", "qwen2vl_72b"],
                    help="qwen2vl_7b is the benchmark configuration (BASELINE.json); the others are labelled secondary lines")
    ap.add_argument("--no-full-prefill", action="store_true",
                    help="skip the secondary report: whole synthetic prefill incl. attention/norms (torch glue)")
    ap.add_argument("--no-logits", action="store_true",
                    help="leave the per-step logits (fp16 lm_head on the last position, side stream) out of the step")
    ap.add_argument("--had-fast", action="store_true",
                    help="non-default Hadamard mode: K x K stage on the fp16 matrix core (not bit-identical; labelled)")
    ap.add_argument("--w-groupsize", type=int, default=-1,
                    help="NON-DEFAULT, labelled secondary line: group-wise weight scales of this many input channels (what a --w_groupsize GPTQ run "
                         "leaves behind; synthetic weights get them from a group-wise RTN), GEMMs on mq_gemm_w4a8_wgroupscale")
    ap.add_argument("--visual-w-bits", type=int, default=None, choices=[4, 8],
                    help="weight bits of everything in front of the language model (the reference's --visual_w_bits; default = 4 like the "
                         "LLM: the benchmark configuration is W4A8 + W4A8).  8 = the reference's first canonical command, docs/qwen2vl.md:19: "
                         "a labelled secondary line")
    ap.add_argument("--ttft-kv-fp8", action="store_true",
                    help="secondary lines: also report the whole-prefill TTFT with the fp8 (e4m3) KV cache read by the prefill attention "
                         "(Qwen2-VL geometries only)")
    ap.add_argument("--no-floor-model", action="store_true",
                    help="skip the per-shape launch timings and the floor model (profiling runs: keeps the kernel trace to the step's own launches)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the bounded secondary block (the other BASELINE configurations + the W8A8-vision line as child processes)")
    ap.add_argument("--secondary-budget", type=float, default=420.0,
                    help="wall-clock seconds the WHOLE default bench may take; secondary entries that would not fit are skipped")
    ap.add_argument("--ttft-iters", type=int, default=100)
    ap.add_argument("--batch", type=int, default=1,
                    help="image+prompt samples per GPU and step (the benchmark configuration is 1; >1 is a scaling study)")
    ap.add_argument("--cpu-selftest", action="store_true",
                    help="launcher / sharding self-test without a GPU: the ranks gather fake logits over gloo")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure and check everything else: kernel attribution and roofline (sustained int8 "
                         "peak, floor model), whole-prefill TTFT, CPU baselines, the secondary configurations, the multi-rank logits "
                         "checks (the --no-* options above switch single parts off again)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (the last Linear's output, the logits) "
                         "as DIR/<name>.npy in float32")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    t_process = time.perf_counter()

    # ---- rank launcher: before torch.cuda / HIP is touched, and never by re-exec ---------------------
    # a rank of torch.distributed.run (any world size, 1 included) carries the whole rendezvous environment; a scheduler that only
    # exports WORLD_SIZE must not push a plain `python bench.py` into init_process_group (it runs as a single process, noted)
    torchrun_env = all(k in os.environ for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")) or "TORCHELASTIC_RUN_ID" in os.environ
    stray_world = (not torchrun_env) and "WORLD_SIZE" in os.environ
    if not torchrun_env:
        if args.gpus > 1:
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
                   "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
            env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            sys.exit(subprocess.call(cmd, env=env))       # fresh children; this process never initialised a GPU
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']} (start one rank per GPU)")

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1")) if torchrun_env else 1
    rank = int(os.environ.get("RANK", "0")) if torchrun_env else 0
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if torchrun_env else 0
    # under torch.distributed.run the process group exists at EVERY world size, 1 included: the RCCL
    # initialisation and the all_gather then run on a one-GPU box too (tests/test_gpu_multi.py)
    distributed = torchrun_env
    if args.cpu_selftest:
        from mquant_amd import shard
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if distributed:
            dist.init_process_group(backend="gloo")
        mine = shard.shard_indices(world, rank, world)
        local = torch.stack([torch.arange(64, dtype=torch.float32) + 1000.0 * i for i in mine])
        full = shard.gather_logits(local, world) if distributed else local
        ok = bool(torch.equal(full, torch.stack([torch.arange(64, dtype=torch.float32) + 1000.0 * i for i in range(world)])))
        if rank == 0:
            print(json.dumps({"selftest": "launcher + batch shard + gather_logits over gloo", "n_gpus": world,
                              "gathered_ok": ok}), flush=True)
        if distributed:
            dist.destroy_process_group()
        sys.exit(0 if ok else 1)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    torch.set_grad_enabled(False)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=dev)

    from mquant_amd import ops, workload

    headline = args.workload == "qwen2vl_7b" and not args.tiny and args.w_groupsize <= 0 and args.visual_w_bits in (None, 4)
    build_specs, workload_desc = workload.WORKLOADS[args.workload]
    specs = workload.tiny_specs() if args.tiny else build_specs(args.batch)
    via_wrappers = not args.direct_engines and not args.tiny      # every workload is built through the drop-in API (round 4: the secondary lines too)
    pf, via_error = None, None
    if via_wrappers:
        try:
            pf = workload.WrapperPrefill(specs, device=dev, dtype=torch.float16, fuse_siblings=not args.no_fuse, w_groupsize=args.w_groupsize,
                                         vis_w_bits=args.visual_w_bits)
        except Exception as exc:          # never lose the bench line: fall back to the directly assembled engines, and say so
            via_error, via_wrappers = repr(exc), False
            torch.cuda.empty_cache()
    if pf is None:
        pf = workload.Prefill(specs, device=dev, dtype=torch.float16, share_groups=not args.no_fuse, vis_w_bits=args.visual_w_bits)
    if args.had_fast:
        pf.set_had_fast(True)            # NON-DEFAULT, labelled secondary line: per-layer flag MQ_HAD_FAST (include/mquant_hip.h)
    tokens_per_step = workload.M_LLM * args.batch if not args.tiny else specs[-1].M
    hidden = specs[-1].n
    vocab = VOCABS.get(args.workload, VOCAB) if not args.tiny else 1024
    B_local = args.batch if not args.tiny else 1      # samples per rank and step: each ends in its own last-position logits

    # Per-step logits: the rank's sample ends in logits = lm_head(rms_norm(last position)) -- fp16, lm_head is not
    # wrapped (reference quant_utils.py:560-564) -- computed from the step's final Linear output INSIDE the step
    # (same hipGraph, same stream).  Under torch.distributed the ranks' logits then go through one RCCL all_gather
    # per step on a SIDE stream, overlapping the next sample's hot path (buffers alternate by step parity).  The
    # real-logits parity check (whole prefill, rank vs single GPU) stays outside the timing.
    with_logits = not args.no_logits
    side = torch.cuda.Stream(device=dev)
    lm_head, logits_step, logits_send, logits_all = None, None, None, None
    if with_logits:
        g = torch.Generator(device=dev).manual_seed(7)
        lm_head = (torch.randn((vocab, hidden), generator=g, device=dev) * 0.02).to(torch.float16)
        logits_step = torch.zeros((B_local, vocab), dtype=torch.float16, device=dev)
        if distributed:
            logits_send = [torch.zeros((B_local, vocab), dtype=torch.float16, device=dev) for _ in range(2)]
            logits_all = [torch.zeros((world * B_local, vocab), dtype=torch.float16, device=dev) for _ in range(2)]

    # N > 1: sample i runs on rank i; static scales are replicated constants (every rank calibrates on
    # sample 0 with the same seeds).  The whole-prefill logits of this rank's sample, for the parity check:
    fp_logits, logits_local = None, None
    if args.full and distributed and headline and args.batch == 1 and not args.no_fuse:
        from mquant_amd.full_prefill import FullPrefill
        fp_logits = FullPrefill(pf, fused_glue=True)
        fp_logits.calibrate()
        fp_logits.set_sample(rank)
        logits_local = fp_logits.step().to(torch.float16).clone()
        fp_logits.restore_hot_path_scales()      # the timed step runs on the hot path's own calibration
        torch.cuda.synchronize(dev)

    def capture(fn, keep=None):
        """Launch-bound inner loop -> one hipGraph (the kernels themselves are unchanged).  ``keep`` receives
        the function's return value (the output tensor of the step's last Linear)."""
        keep = keep if keep is not None else [None]
        if args.no_graph:
            def eager():
                keep[0] = fn()
            eager()
            return eager
        fn()                      # first-call allocations / attribute setup happen outside capture
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        # thread_local: the default (global) capture mode makes EVERY thread's event queries fail while this thread captures,
        # and the RCCL watchdog thread polls its collectives' events at any time -- one bench in ~15 aborted with
        # hipErrorStreamCaptureUnsupported in ProcessGroupNCCL's watchdog under torchrun (tools/debug/torchrun_loop.sh)
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            keep[0] = fn()
        return g.replay

    # the samples of a step are stacked along the rows: sample b ends at row (b + 1) * M / B_local - 1
    last_rows = None
    if with_logits and B_local > 1:
        per = specs[-1].M // B_local
        last_rows = torch.arange(1, B_local + 1, device=dev) * per - 1

    def lm_logits(h):
        # the unquantized lm_head on the last position(s): mq_gemv_f16 streams the weights once (6.8 TB/s where hipBLASLt's kernel for
        # the shape reaches 5.0); more than 8 rows per rank go to torch.matmul
        if h.shape[0] <= 8 and h.shape[0] * hidden * 2 <= 65536:
            ops.gemv_f16(h, lm_head, out=logits_step)
        else:
            torch.matmul(h, lm_head.t(), out=logits_step)

    def hot_path_and_logits():
        y = pf.step()                    # [M, hidden]: output of the last Linear of the step (down_proj)
        if with_logits:
            h = torch.nn.functional.rms_norm(y[-1:] if last_rows is None else y.index_select(0, last_rows), (hidden,), eps=1e-6)
            lm_logits(h)
        return y

    step_out = [None]                    # the last Linear's output of the latest step (the graph's own buffer when captured)
    run_step = capture(hot_path_and_logits, step_out)
    counter = [0]
    side_done = [None, None]

    def step():
        run_step()
        if not (with_logits and distributed):
            return
        par = counter[0] & 1
        counter[0] += 1
        main = torch.cuda.current_stream(dev)
        if side_done[par] is not None:
            main.wait_event(side_done[par])          # the side stream has finished with this parity's buffers
        logits_send[par].copy_(logits_step)
        ev = torch.cuda.Event()
        ev.record(main)
        with torch.cuda.stream(side):
            side.wait_event(ev)
            dist.all_gather_into_tensor(logits_all[par], logits_send[par])
            side_done[par] = torch.cuda.Event()
            side_done[par].record(side)

    def fence():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize(dev)

    # settle clocks / caches before the contract's W warm-up steps: ~0.3 s of untimed replays of the captured step (the
    # sustained run of profiles/r3_soak.txt is ~0.8 % faster once warm; a fresh box's first process has been seen slower)
    settle_replays = 0 if args.tiny else 30
    for _ in range(settle_replays):
        run_step()
    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    if distributed:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    ms_per_step = elapsed / args.steps * 1e3
    value = world * tokens_per_step * args.steps / elapsed

    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its last step, before anything else runs on the model
        import numpy as np
        outputs = {"last_linear_out": step_out[0]}
        if with_logits:
            outputs["logits"] = logits_step
            if distributed:
                outputs["logits_all_ranks"] = logits_all[(counter[0] - 1) & 1]
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, t in outputs.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), t.float().cpu().numpy())

    logits_check = None
    if args.full and distributed and with_logits:
        # what the timed steps exchanged: row r of the gathered tensor is rank r's logits of that step
        par = (counter[0] - 1) & 1
        mine = logits_all[par][rank * B_local:(rank + 1) * B_local]
        logits_check = {"step_exchange": {"all_gather_bytes": int(world * B_local * vocab * 2), "samples_per_rank": B_local,
                                          "own_row_intact": bool(torch.equal(mine, logits_step)),
                                          "finite": bool(torch.isfinite(logits_all[par].float()).all().item())}}
        if B_local > 1:
            # the B_local > 1 path of shard.gather_logits (sample i lives on rank i % world): this rank's rows come back at
            # the positions of its samples, in sample order
            from mquant_amd import shard
            n_samples = world * B_local
            ordered = shard.gather_logits(logits_step.clone(), n_samples)
            mine_idx = shard.shard_indices(n_samples, rank, world)
            logits_check["gather_logits"] = {"samples": n_samples, "shape": list(ordered.shape),
                                             "own_samples_in_place": bool(torch.equal(ordered[torch.tensor(mine_idx, device=dev)], logits_step))}
    if fp_logits is not None:
        from mquant_amd import shard
        gathered = shard.gather_logits(logits_local, world)
        torch.cuda.synchronize(dev)
        if rank == 0:
            # rank r's result for sample r must equal the single-GPU result for the same sample
            fp_logits.apply_full_prefill_scales()
            same = []
            for i in range(world):
                fp_logits.set_sample(i)
                ref = fp_logits.step().to(torch.float16)
                same.append(bool(torch.equal(ref[0], gathered[i])))
            fp_logits.restore_hot_path_scales()
            logits_check = dict(logits_check or {}, samples=world, equal_to_single_gpu=all(same), per_sample=same)

    if args.full:
        # ---- kernel attribution: the GEMM launches of a step alone, HIP events on the launch stream
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = max(3, min(args.steps, 10))

        def timed(run, batches=5):
            """average duration of one replay: median over ``batches`` batches of ``reps`` back-to-back replays (a single
            batch right after the host-side checks above was seen 13 % slow on a fresh box: clocks / power state)"""
            for _ in range(2):
                run()
            torch.cuda.synchronize(dev)
            got = []
            for _ in range(batches):
                e0.record()
                for _ in range(reps):
                    run()
                e1.record()
                torch.cuda.synchronize(dev)
                got.append(e0.elapsed_time(e1) / reps)
            got.sort()
            return got[len(got) // 2]

        hot_ms = timed(capture(pf.step))                 # the hot path alone (no logits, no exchange), stream-timed
        gemm_ms = timed(capture(pf.step_gemm_only))
        quant_ms = timed(capture(pf.step_quant_only))
        lm_ms = None
        if with_logits:
            last_row = torch.zeros((B_local, hidden), dtype=torch.float16, device=dev)

            def lm_only():
                h = torch.nn.functional.rms_norm(last_row, (hidden,), eps=1e-6)
                lm_logits(h)
            lm_ms = timed(lm_only)
        launches = pf.gemm_launches()
        traffic, traffic_note, traffic_source, traffic_stale = None, "no PMC traffic file for this workload", None, None
        tpath = next((pth for pth in (os.path.join(ROOT, "profiles", nm) for nm in ("r6_traffic.json", "r5_traffic.json", "r4_traffic.json", "r3_traffic.json", "r2_traffic.json"))
                      if os.path.exists(pth)), None)
        if tpath and headline and args.batch == 1 and not args.no_fuse:
            # HBM bytes per GEMM launch from the PMC passes (tools/pmc_traffic.py); counters cannot be
            # read inside the timed run, so this is the committed measurement of the same command -- with
            # the commit and command it was taken at, so that a stale file is detectable
            with open(tpath) as fh:
                tj = json.load(fh)
            traffic = tj["kernels"].get("gemm", {}).get("hbm_bytes_per_launch")
            traffic_note = tj["corrections"]
            # stale = any kernel source changed since the counters were taken (digest over mquant_amd/csrc/*.hip, *.h recorded by
            # tools/pmc_traffic.py; files measured before round 4 carry none and count as stale)
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            try:
                from pmc_traffic import csrc_digest
                digest_now = csrc_digest()
            except Exception:
                digest_now = None
            traffic_stale = not (digest_now is not None and tj.get("csrc_sha16") == digest_now)
            traffic_source = {"file": os.path.relpath(tpath, ROOT), "measured_at_commit": tj.get("commit"),
                              "command": tj.get("command"), "csrc_sha16": tj.get("csrc_sha16"), "csrc_sha16_now": digest_now}
        achieved = pf.gemm_ops() / (gemm_ms * 1e-3) / 1e12
        step_tops = pf.gemm_ops() / (ms_per_step * 1e-3) / 1e12
        roofline = {"bound": "mfma", "kernel": "gemm_ws_kernel / gemm_w4a8_pp_kernel 256x256 (both V_MFMA_I32_16X16X64_I8)",
                    "achieved": round(achieved, 2), "peak": PEAK_INT8_TOPS, "unit": "TOP/s",
                    "frac": round(achieved / PEAK_INT8_TOPS, 4),
                    "step_frac": round(step_tops / PEAK_INT8_TOPS, 4),
                    "step_frac_note": "GEMM ops / ms_per_step / peak: the whole timed step (quantize and Hadamard launches included), "
                                      "where frac covers the GEMM launches alone",
                    "traffic": traffic,
                    "traffic_unit": "HBM bytes per launch (PMC FETCH_SIZE x2 + WRITE_SIZE)", "traffic_note": traffic_note,
                    "traffic_source": traffic_source, "traffic_stale": traffic_stale,
                    "algorithmic_bytes_per_launch": round(pf.gemm_bytes() / launches),
                    "launches_per_step": launches,
                    "avg_launch_us": round(gemm_ms * 1e3 / launches, 3),
                    "algorithmic_ops_per_launch": round(pf.gemm_ops() / launches),
                    "gemm_ms_per_step": round(gemm_ms, 4),
                    "quant_hadamard_ms_per_step": round(quant_ms, 4),
                    "quant_hadamard_GBps": round(pf.quant_bytes() / (quant_ms * 1e-3) / 1e9, 1),
                    "hot_path_ms_per_step_stream_timed": round(hot_ms, 4)}

        if not args.tiny:
            try:
                sus = sustained_int8_peak(pf, dev)
                top = max(sus["mfma_i32_16x16x64_i8"], sus["mfma_i32_32x32x32_i8"])
                roofline["peak_sustained_measured"] = {
                    "value": top, "unit": "TOP/s", "by_instruction": sus,
                    "how": "mq_bench_mfma_burn: register-only int8 MFMA chains, 2 waves per SIMD on every CU, no memory traffic, operand bytes "
                           "taken from this workload's int8 activations and unpacked int4 weights; ~60 ms per reading, measured live on this box",
                    "frac_of_sustained": round(achieved / top, 4), "step_frac_of_sustained": round(step_tops / top, 4),
                    "note": "the package power limit (~1.3-1.4 kW) sets the clock: the nominal peak (2.4 GHz) is reached on all-zero operands only; "
                            "frac keeps the nominal peak as its denominator (profiles/r5_clock_reconciliation.txt)"}
            except Exception as exc:  # a report, never a reason to lose the line
                roofline["peak_sustained_measured"] = {"value": None, "how": f"failed: {exc!r}"}

        if not args.tiny and not args.no_floor_model:
            # per-shape launch times (each shape's GEMMs back to back from their own hipGraph, distinct weight images as in the step) and the
            # floor model beside them: mquant_amd/floor_model.py
            try:
                from mquant_amd import floor_model
                from mquant_amd.engine import WORKSPACE
                groups = floor_model.shape_groups(pf.layers)
                per_shape_us = {}
                for gi, grp in enumerate(groups):
                    def run_group(grp=grp):
                        for L in grp["layers"]:
                            a = WORKSPACE.act(dev, L.spec.M, L.lin.K_pad)
                            x0 = WORKSPACE.x0(dev, L.spec.M) if L.lin.split else None
                            L.lin.gemm(a, x0, torch.float16, L.row_sel, L.out)
                    per_shape_us[gi] = timed(capture(run_group), batches=3) * 1e3 / len(grp["layers"])
                sus_top = (roofline.get("peak_sustained_measured") or {}).get("value") or 0.0
                fm = floor_model.summarize(groups, per_shape_us, sus_top, cus=torch.cuda.get_device_properties(dev).multi_processor_count)
                roofline["frac_floor_model"] = fm["frac_floor_model"]
                roofline["floor_model"] = fm
            except Exception as exc:  # a report, never a reason to lose the line
                roofline["floor_model"] = {"error": repr(exc)}

    n_lin = sum(sp.count for sp in specs)
    desc = workload_desc + f", M_llm={workload.M_LLM}"
    if args.batch != 1:
        desc += f", x{args.batch} samples per step" + (" (scaling study, not the benchmark configuration)" if headline else "")
    if not args.no_fuse:
        desc += " (Linears fed the same tensor -- q/k/v, gate/up -- share one quantization and one GEMM)"
    if not headline and not args.tiny:
        desc = "SECONDARY LINE, not the benchmark configuration: " + desc
    if args.w_groupsize > 0:
        desc = (f"NON-DEFAULT group-wise weight scales (--w_groupsize {args.w_groupsize}; every Linear whose input width is a multiple of it -- "
                "all but the vision tower's split fc2): ") + desc
    if args.visual_w_bits == 8:
        desc = ("W8A8 vision tower + merger (--visual_w_bits 8) with the W4A8 LLM -- the reference's first canonical command, "
                "docs/qwen2vl.md:19; NOT the benchmark configuration (W4A8 + W4A8): ") + desc
    if args.had_fast:
        desc = "NON-DEFAULT fast Hadamard mode (fp16 matrix-core K x K stage, not bit-identical to the reference): " + desc
    line = {"metric": "W4A8 prefill tokens/sec (hot path: Hadamard + static quant + W4A8 Linear), "
                      + {"qwen2vl_7b": "Qwen2-VL-7B 448px+512tok", "qwenvl_7b": "Qwen-VL-7B 448px+512tok",
                         "internvl2_8b": "InternVL2-8B 448px+512tok", "qwen2vl_72b": "Qwen2-VL-72B 448px+512tok"}[args.workload],
            "value": round(value, 1), "unit": "tokens/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "int8",
            "data": f"synthetic (random weights with the real shapes, all {n_lin} weight images distinct = "
                    f"{pf.weight_bytes() / 1e9:.2f} GB streamed per step; random activations with outlier channels; layers of equal "
                    "(M, k_in) read the SAME synthetic input tensor, which flatters the caches slightly on the activation side)",
            "config": {"workload": desc if not args.tiny else "tiny debug shapes",
                       "path": ("fake_quant drop-in API: add_actquant -> RTN -> calibration protocol -> model_quant -> "
                                "ActQuantWrapper.forward" if via_wrappers else "integer engines assembled directly (workload.Prefill)")
                               + (f"; the wrapper build FAILED and was replaced: {via_error}" if via_error else ""),
                       "step": "every wrapped Linear of one image+prompt prefill (quantize / Hadamard+quantize launch + GEMM launch each), one hipGraph"
                               + ("; then the sample's logits (fp16 lm_head on the last position, same graph)"
                                  + ("; the RCCL all_gather of the ranks' logits runs on a side stream and overlaps the next sample's hot path" if distributed else "")
                                  if with_logits else ""),
                       "tokens_per_step_per_gpu": tokens_per_step, "parallelism": f"batch-shard x{world}",
                       "gemm_TOP_per_step": round(pf.gemm_ops() / 1e12, 3),
                       "hip_graph": not args.no_graph, "settle_replays": settle_replays,
                       "settle_replays_note": "untimed replays of the captured step before the contract's warm-up steps",
                       "weights_GB": round(pf.weight_bytes() / 1e9, 3)}}
    if args.full:
        line["config"].update(ttft_hot_path_ms=round(hot_ms, 4), lm_head_ms=None if lm_ms is None else round(lm_ms, 4))
        line["roofline"] = roofline
    if args.full and headline and not (args.no_full_prefill or args.no_fuse or args.batch != 1):
        line["full_prefill"] = full_prefill_report(pf, dev, args)
    if args.ttft_kv_fp8 and not args.tiny and args.workload in ("qwen2vl_7b", "qwen2vl_72b") and not args.no_fuse and args.batch == 1:
        from mquant_amd import full_prefill as fpm
        line["full_prefill_kv_fp8"] = full_prefill_report(pf, dev, args, geometry=fpm.QWEN2VL_72B if args.workload == "qwen2vl_72b" else fpm.QWEN2VL_7B,
                                                          kv_fp8=True, attn_fp8=True, variants=False)
    if stray_world:
        line["config"]["launcher_note"] = ("WORLD_SIZE was set without RANK / LOCAL_RANK / MASTER_PORT (not a torch.distributed.run "
                                           "rank): ran as a single process")
    if logits_check is not None:
        line["logits_check"] = logits_check
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and headline:
        try:
            line["cpu_baseline"] = cpu_baseline_reference()
        except Exception as exc:  # the baseline is a report, never a reason to lose the line
            line["cpu_baseline"] = {"value": None, "unit": "tokens/s", "cores": 0, "kind": "reference",
                                    "sample": f"failed: {exc!r}"}
        try:                      # second, labelled number: the C port of the integer path (oracle/mq_oracle.c)
            line["cpu_baseline_port"] = cpu_baseline(float(pf.gemm_ops()))
        except Exception as exc:
            line["cpu_baseline_port"] = {"value": None, "kind": "port", "sample": f"failed: {exc!r}"}
    if args.full and rank == 0 and world == 1 and headline and not args.no_secondary and not args.no_fuse and args.batch == 1 and not args.had_fast:
        # the headline is complete; the other configurations follow as bounded child processes (this process keeps its line)
        try:
            pf = None
            torch.cuda.empty_cache()
            line["secondary"] = run_secondary(args.secondary_budget, t_process)
        except Exception as exc:
            line["secondary"] = {"error": repr(exc)}
    if rank == 0:
        print(json.dumps(line), flush=True)
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
