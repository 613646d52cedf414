"""Generation end to end against the float64 model of tests/generation_reference.py: ``GreedyLoop`` and ``GreedyLoopBatch`` over
both cache storages, held to a model of the whole token sequence that has no cache, no kernel and no position arithmetic in
common with them.  Every other greedy-loop file compares the loop with paths that share ``cache.step``; a mistake all of them
share (a decode position, the newest key, the order of the scale halves, the GQA map, a neighbour's ``rope_delta``) shows here.

The body is the greedy-loop tests' body plus the weight-less RMS norm in front of q|k|v.  Prompts enter the cache two ways:
  (a) ``cache.advance(R); cache.step(...)`` with R <= 8 rows per call and ``rope_delta`` 0, the delta set afterwards.  The batch
      (prompts of 5, 8 and 2 tokens) takes rows [0, 2), [2, 5), [5, 8) in three calls; a sequence whose prompt has ended is fed
      token 0, and ``start`` then sets its length back: generation overwrites those rows before it reads them;
  (b) K rotated by ``ops.rope_inplace`` at positions 0 .. P - 1 and written with ``cache.fill``, the prefill hand-off.
The first token is picked on the device from the prompt's last row, so the prompt's attention is under the id demand too.

Assertions, per sequence (a batch's sequences each against their own single-sequence reference), for eager steps:
  16-bit  the 16 embedded ids and ``token`` equal float64 greedy decoding; the relative hidden error at every generated position
          is <= c * E_plain; every cache row is within c * plain's error of the same row, K and V apart.
  e4m3    the reference runs over the device's ids and attends the device's dequantised cache bytes: the same hidden demand; per
          layer, for K and V apart, the share of bytes that differ from the reference's own codes <= 2 * plain's share and the
          relative error of the dequantised rows <= 2 * plain's; the device's id equals the reference's argmax wherever its margin
          exceeds 2 * c * plain's logit error, and at most a quarter of the positions fall under it.
  both    rows beyond the last position keep the NaN pattern they started with.
c and every yardstick (E_plain, plain's shares and row errors) come from the CPU alone: tests/test_generation_reference_cpu.py.
The first fp16 case also runs ``capture()`` + ``generate()`` (the same ids and cache bytes as the eager run) and, for the batch,
a second run with two deltas exchanged, which must change exactly those two sequences.

Geometry (4, 4, 64) cannot generate on the device: the decode attention kernels are built for head_dim 128 and refuse it.  Its full
model is pinned on the CPU only; here ``check_append_at_head_dim_64`` holds layer 0's cache rows -- the append's positions, deltas and
RoPE group count at head_dim 64 -- to the float64 model.  (4, 4, 128) runs end to end in its place."""
import json
import time

import pytest
import torch
import torch.nn.functional as F

import generation_reference as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
CAP, STEPS = 32, G.STEPS
POISON = {torch.float8_e4m3fn: 0x7F, torch.float16: 0x7E00, torch.bfloat16: 0x7FC0}       # a NaN of the storage
VARIANTS = "h4kv2d128-fp16"
RUNS = [(c.name, storage, kind) for c in G.CASES.values() if c.name not in G.CPU_ONLY for storage in G.STORAGES
        for kind in ("single", "batch")]


class _Model:
    """One case on the device: the weights, a fresh cache of either kind, the body over it (it records its outputs on request)."""

    def __init__(self, name, storage, batch, deltas):
        from mquant_amd import Fp8KVCache, Fp8KVCacheBatch, KVCache16, KVCache16Batch
        c, w = G.CASES[name], G.case_weights(name)
        self.case, self.storage, self.batch, self.w = c, storage, batch, w
        self.H, self.HKV, self.D = c.geometry
        self.table, self.lm_head = w.table.to(DEV), w.lm_head.to(DEV)
        self.layers = [(a.to(DEV), b.to(DEV)) for a, b in w.layers]
        cos, sin = G.rope_tables(CAP + 8, self.D, w.dtype)
        self.cos, self.sin = cos.to(DEV), sin.to(DEV)
        self.scales = [s.to(DEV) for s in G.make_kv_scales(c.geometry)]
        lead = (batch,) if batch else ()
        zero = [0] * batch if batch else 0                            # the offset tensor exists from the start; (a) sets it later
        if storage == "e4m3":
            cls = Fp8KVCacheBatch if batch else Fp8KVCache
            self.cache = cls(*lead, G.LAYERS, CAP, self.HKV, self.D, self.scales, self.cos, self.sin, DEV, w.dtype, rope_delta=zero)
        else:
            cls = KVCache16Batch if batch else KVCache16
            self.cache = cls(*lead, G.LAYERS, CAP, self.HKV, self.D, self.cos, self.sin, DEV, w.dtype, rope_delta=zero)
        self.deltas = deltas
        for buf in self.cache.caches:                                 # nothing at or beyond n_keys may matter
            self._raw(buf)[:] = POISON[buf.dtype]
        self.record = None

    @staticmethod
    def _raw(buf):
        return buf.view(torch.uint8 if buf.dtype == torch.float8_e4m3fn else torch.int16)

    def body(self, h):
        for i, (wqkv, wo) in enumerate(self.layers):
            o = self.cache.step(i, F.linear(F.rms_norm(h, (G.DIM,), eps=G.EPS), wqkv), self.H)
            h = h + F.linear(o, wo)
        if self.record is not None:
            self.record.append(h.clone())
        return h

    def pick(self, h):
        from mquant_amd import ops
        return ops.gemv_f16_argmax(F.rms_norm(h, (G.DIM,), eps=G.EPS), self.lm_head).cpu().tolist()

    # ---- the two ways a prompt enters the cache: -> the first token(s), picked on the device ----
    def prompt_by_steps(self, prompts):
        """(a): multi-row steps at rope_delta 0"""
        B = len(prompts)
        bounds, first = sorted(set(len(p) for p in prompts)), [None] * B
        lo = 0
        for hi in bounds:
            assert hi - lo <= 8
            toks = [(p[lo:hi] if hi <= len(p) else [0] * (hi - lo)) for p in prompts]
            self.cache.advance(hi - lo)
            h = self.body(self.table[torch.tensor(sum(toks, []), device=DEV)]).view(B, hi - lo, G.DIM)
            for b, p in enumerate(prompts):
                if len(p) == hi:
                    first[b] = self.pick(h[b, -1:])[0]
            lo = hi
        return first

    def prompt_by_fill(self, prompts):
        """(b): a prefill of every sequence on its own -- rope_inplace, cache.fill, the prefill attention"""
        from mquant_amd import ops
        H, HKV, D = self.H, self.HKV, self.D
        first = []
        for b, p in enumerate(prompts):
            P = len(p)
            h = self.table[torch.tensor(p, device=DEV)]
            for i, (wqkv, wo) in enumerate(self.layers):
                qkv = F.linear(F.rms_norm(h, (G.DIM,), eps=G.EPS), wqkv)
                ops.rope_inplace(qkv, H + HKV, D, self.cos[:P].contiguous(), self.sin[:P].contiguous())
                q, kv = qkv[:, :H * D].view(P, H, D), qkv[:, H * D:].view(P, 2 * HKV, D)
                rows = self.cache.fill(i, b, kv) if self.batch else self.cache.fill(i, kv)
                if self.storage == "e4m3":
                    o = ops.attn_prefill_fp8kv(q, rows, self.scales[i])
                else:
                    o = ops.attn_prefill(q, kv[:, :HKV], kv[:, HKV:])
                h = h + F.linear(o, wo)
            first.append(self.pick(h[-1:])[0])
        return first

    def loop(self, prompts, path):
        """the prompt through `path`, the deltas set, a started loop"""
        from mquant_amd import GreedyLoop, GreedyLoopBatch
        first = (self.prompt_by_steps if path == "a" else self.prompt_by_fill)(prompts)
        if self.batch:
            self.cache.set_rope_delta(self.deltas)
            loop = GreedyLoopBatch(self.cache, self.table, self.lm_head, self.body, eps=G.EPS)
            loop.start([len(p) for p in prompts], first)
        else:
            self.cache.set_rope_delta(self.deltas[0])
            loop = GreedyLoop(self.cache, self.table, self.lm_head, self.body, eps=G.EPS)
            loop.start(len(prompts[0]), first[0])
        return loop

    def state(self, loop, b, P):
        """what one sequence left behind: (ids embedded at P .. P + STEPS - 1, token, per layer the raw cache [CAP, 2 HKV, D])"""
        ids, token = loop.ids.cpu(), loop.token.cpu().tolist()
        ids = ids[b] if self.batch else ids
        assert ids[:P].tolist() == [0] * P and ids[P + STEPS:].tolist() == [0] * (CAP - P - STEPS)     # nothing else is logged
        raws = [self._raw(buf[b] if self.batch else buf).cpu() for buf in self.cache.caches]
        return ids[P:P + STEPS].tolist(), token[b if self.batch else 0], raws


def _eager(name, storage, kind, path, deltas=None):
    """-> (model, per sequence (embedded ids, token, hidden [STEPS, dim] float64, raw cache per layer), the case's sequence numbers)"""
    c = G.CASES[name]
    seqs = [1, 2, 3] if kind == "batch" else [0]
    deltas = deltas or [c.sequences[s].rope_delta for s in seqs]
    prompts = [G.make_prompt(c.sequences[s].prompt_seed, c.sequences[s].prompt_len) for s in seqs]
    m = _Model(name, storage, len(seqs) if kind == "batch" else 0, deltas)
    loop = m.loop(prompts, path)
    m.record = []
    for _ in range(STEPS):
        loop.step()
    hidden, m.record = torch.stack(m.record).cpu().to(torch.float64), None             # [STEPS, B or 1, dim]
    assert m.cache.n_keys.cpu().tolist() == [len(p) + STEPS for p in prompts]
    return m, loop, [m.state(loop, b, len(p)) + (hidden[:, b],) for b, p in enumerate(prompts)], seqs


def _untouched(m, raws, P, who):
    for raw in raws:
        assert bool((raw[P + STEPS:] == POISON[m.cache.caches[0].dtype]).all()), f"{who}: a row beyond the last position was written"


def _check_16bit(m, seq, got, who, figures):
    ids, token, raws, hidden = got
    c, y = m.case, G.yardstick(m.case.name, "16bit", seq)
    P, cc, HKV = c.sequences[seq].prompt_len, G.C[c.dtype], m.HKV
    print(f"{who}: ids {ids} then {token}")

    def cache_rows(a, b, what):
        for i, raw in enumerate(raws):
            rows = raw[:P + STEPS].view(m.w.dtype).to(torch.float64)
            for half, (e, e_plain) in enumerate(zip(G.rel_rows_kv(rows, y["ref"]["kv"][i], HKV), y["kv_row_err"][i])):
                ratio = float((e[a:b] / e_plain[a:b]).max())
                figures["kv_row_ratio"] = max(figures.get("kv_row_ratio", 0.0), ratio)
                assert ratio <= cc, f"{who}: layer {i} {'KV'[half]} {what} rows {e[a:b].tolist()} above {cc} * plain's {e_plain[a:b].tolist()}"

    cache_rows(0, P, "prompt")                                        # these do not depend on any picked id: before the id demand
    assert ids == y["ids"][P:P + STEPS], f"{who}: the embedded ids are not float64 greedy decoding's {y['ids'][P:P + STEPS]}"
    assert token == y["ids"][P + STEPS], f"{who}: token {token}, float64 picks {y['ids'][P + STEPS]}"
    err = G.rel_rows(hidden, y["ref"]["hidden"][P:])
    figures["r"] = max(figures.get("r", 0.0), float(err.max()) / y["e_plain"])
    print(f"{who}: hidden error {float(err.max()):.2e}, E_plain {y['e_plain']:.2e}, r = {float(err.max()) / y['e_plain']:.2f}")
    assert float(err.max()) <= cc * y["e_plain"], f"{who}: hidden error {err.tolist()} above {cc} * E_plain = {cc * y['e_plain']:.2e}"
    cache_rows(P, P + STEPS, "generated")
    _untouched(m, raws, P, who)


def _check_e4m3(m, seq, got, who, figures):
    ids, token, raws, hidden = got
    c, y = m.case, G.yardstick(m.case.name, "e4m3", seq)
    s, cc, HKV = c.sequences[seq], G.C[c.dtype], m.HKV
    P = s.prompt_len
    print(f"{who}: ids {ids} then {token}")
    scales = G.make_kv_scales(c.geometry)
    codes = [raw[:P + STEPS] for raw in raws]
    forced = [G.e4m3_values(code, sc) for code, sc in zip(codes, scales)]
    ref = G.reference(m.w, y["prompt"] + ids, P, s.rope_delta, storage="e4m3", kv_scales=scales, forced_cache=forced)
    err = G.rel_rows(hidden, ref["hidden"][P:])
    figures["r"] = max(figures.get("r", 0.0), float(err.max()) / y["e_plain"])
    print(f"{who}: hidden error {float(err.max()):.2e}, E_plain {y['e_plain']:.2e}, r = {float(err.max()) / y['e_plain']:.2f}")
    assert float(err.max()) <= cc * y["e_plain"], f"{who}: hidden error {err.tolist()} above {cc} * E_plain = {cc * y['e_plain']:.2e}"
    for i in range(G.LAYERS):
        for half, sl in enumerate((slice(0, HKV), slice(HKV, 2 * HKV))):
            share, deq = G.share_differing(codes[i][:, sl], ref["codes"][i][:, sl]), G.rel_all(forced[i][:, sl], ref["kv"][i][:, sl])
            figures["share"] = max(figures.get("share", 0.0), share)
            figures["share_over_plain"] = max(figures.get("share_over_plain", 0.0), share / max(y["share"][i][half], 1e-9))
            figures["deq_over_plain"] = max(figures.get("deq_over_plain", 0.0), deq / max(y["deq_err"][i][half], 1e-30))
            assert share <= 2 * y["share"][i][half], \
                f"{who}: layer {i} {'KV'[half]}: {share:.4f} of the cache bytes differ from the reference's codes, plain's share is {y['share'][i][half]:.4f}"
            assert deq <= 2 * y["deq_err"][i][half], \
                f"{who}: layer {i} {'KV'[half]}: dequantised rows {deq:.2e} from the reference's, plain's are {y['deq_err'][i][half]:.2e}"
    want, margin = G.margins(ref["logits"][P - 1:])
    low = margin <= 2 * cc * y["logit_err"]
    figures["low_margins"] = max(figures.get("low_margins", 0), int(low.sum()))
    assert int(low.sum()) <= STEPS // 4, f"{who}: {int(low.sum())} margins under 2 * {cc} * {y['logit_err']:.4f}"
    for j, (a, b) in enumerate(zip(want, ids + [token])):
        assert low[j] or a == b, f"{who}: pick {j} is {b}, the reference's argmax {a} has a margin of {float(margin[j]):.4f}"
    _untouched(m, raws, P, who)


def _same_bytes(a, b):
    return a[0] == b[0] and a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def check_run(name, storage, kind):
    """one configuration: both prompt paths, and on the first case the captured step and the exchanged deltas"""
    check = _check_16bit if storage == "16bit" else _check_e4m3
    figures, t0 = {}, time.perf_counter()
    for path in "ab":
        m, loop, got, seqs = _eager(name, storage, kind, path)
        for b, seq in enumerate(seqs):
            check(m, seq, got[b], f"{name} {storage} {kind} prompt ({path}) sequence {b}", figures)
        if name != VARIANTS or path != "a":
            continue
        # capture() + generate(): the same ids and the same cache bytes as the eager run just checked
        who = f"{name} {storage} {kind} captured"
        c = G.CASES[name]
        prompts = [G.make_prompt(c.sequences[s].prompt_seed, c.sequences[s].prompt_len) for s in seqs]
        m2 = _Model(name, storage, m.batch, m.deltas)
        loop2 = m2.loop(prompts, "a")
        loop2.capture()
        ids = loop2.generate(STEPS)
        ids = ids.tolist() if kind == "batch" else [ids.tolist()]
        for b, p in enumerate(prompts):
            state = m2.state(loop2, b, len(p))
            assert ids[b] == state[0] == got[b][0], f"{who} sequence {b}: ids {ids[b]}, eager {got[b][0]}"
            assert _same_bytes(state, got[b]), f"{who} sequence {b}: token or cache bytes differ from the eager run's"
        if kind != "batch":
            continue
        # two deltas exchanged: exactly those two sequences change
        who = f"{name} {storage} batch, deltas of sequences 0 and 1 exchanged"
        deltas = [m.deltas[1], m.deltas[0], m.deltas[2]]
        _, _, other, _ = _eager(name, storage, kind, "a", deltas=deltas)
        for b in (0, 1):
            assert not torch.equal(other[b][3][0], got[b][3][0]), f"{who}: sequence {b}'s first generated hidden state did not move"
        assert _same_bytes(other[2], got[2]) and torch.equal(other[2][3], got[2][3]), f"{who}: sequence 2 changed"
    figures["seconds"] = round(time.perf_counter() - t0, 2)
    print("FIGURES " + json.dumps({"run": f"{name}-{storage}-{kind}", **{k: round(v, 4) for k, v in figures.items()}}))


def check_append_at_head_dim_64(storage, kind):
    """The (4, 4, 64) geometry of the CPU file cannot generate here (the decode attention is built for head_dim 128 and refuses 64:
    tests/test_attn_decode_refusals_cpu.py), but the append serves it, with the other RoPE group count.  Layer 0's K|V depend on the
    ids and the positions only, so the cache's own append is held to the float64 model there: the prompt in multi-row appends at
    delta 0 as in (a), then the yardstick's ids one row at a time at the sequence's delta; the bounds of the full runs."""
    name = "h4kv4d64-fp16"
    c = G.CASES[name]
    seqs = [1, 2, 3] if kind == "batch" else [0]
    ys = [G.yardstick(name, storage, s) for s in seqs]
    prompts = [y["prompt"] for y in ys]
    m = _Model(name, storage, len(seqs) if kind == "batch" else 0, [c.sequences[s].rope_delta for s in seqs])
    wqkv = m.layers[0][0]

    def push(toks):
        m.cache.advance(len(toks[0]))
        h = m.table[torch.tensor(sum(toks, []), device=DEV)]
        m.cache._append(0, F.linear(F.rms_norm(h, (G.DIM,), eps=G.EPS), wqkv), m.H)

    lo = 0
    for hi in sorted(set(len(p) for p in prompts)):
        push([(p[lo:hi] if hi <= len(p) else [0] * (hi - lo)) for p in prompts])
        lo = hi
    m.cache.set_length([len(p) for p in prompts] if m.batch else len(prompts[0]))
    m.cache.set_rope_delta(m.deltas if m.batch else m.deltas[0])
    for j in range(STEPS):
        push([[y["ids"][len(p) + j]] for y, p in zip(ys, prompts)])
    HKV, cc = m.HKV, G.C[c.dtype]
    for b, (y, p) in enumerate(zip(ys, prompts)):
        who, P = f"append at head_dim 64, {storage} {kind} sequence {b}", len(p)
        raw = m._raw(m.cache.caches[0][b] if m.batch else m.cache.caches[0]).cpu()
        want = y["ref"]["kv"][0]
        if storage == "16bit":
            rows = raw[:P + STEPS].view(m.w.dtype).to(torch.float64)
            for half, (e, e_plain) in enumerate(zip(G.rel_rows_kv(rows, want, HKV), y["kv_row_err"][0])):
                assert float((e / e_plain).max()) <= cc, f"{who}: {'KV'[half]} rows {e.tolist()} above {cc} * plain's {e_plain.tolist()}"
        else:
            codes = raw[:P + STEPS]
            deq = G.e4m3_values(codes, G.make_kv_scales(c.geometry)[0])
            for half, sl in enumerate((slice(0, HKV), slice(HKV, 2 * HKV))):
                share, err = G.share_differing(codes[:, sl], y["ref"]["codes"][0][:, sl]), G.rel_all(deq[:, sl], want[:, sl])
                assert share <= 2 * y["share"][0][half], f"{who}: {'KV'[half]}: {share:.4f} of the bytes differ, plain's share is {y['share'][0][half]:.4f}"
                assert err <= 2 * y["deq_err"][0][half], f"{who}: {'KV'[half]}: dequantised rows {err:.2e}, plain's {y['deq_err'][0][half]:.2e}"
        _untouched(m, [raw], P, who)


def test_generation_equals_the_float64_model():
    """every configuration of this file in one test, as the other greedy-loop files do (they share the yardsticks and the suite
    keeps its test count); every configuration runs whatever the ones before it did, and a failure names each one that failed"""
    failed = []
    for run in RUNS:
        try:
            check_run(*run)
        except AssertionError as e:
            failed.append(f"{'-'.join(run)}: {e}")
    d64 = [(storage, kind) for storage in G.STORAGES for kind in ("single", "batch")]
    for run in d64:
        try:
            check_append_at_head_dim_64(*run)
        except AssertionError as e:
            failed.append(f"head_dim 64 {'-'.join(run)}: {e}")
    assert not failed, f"{len(failed)} of {len(RUNS) + len(d64)} configurations failed:\n" + "\n".join(failed)
