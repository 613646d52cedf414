"""A float64 model of greedy generation, written from the formulas: no cache object, no kernel, no ``mquant_amd`` import.

The toy decoder of the greedy-loop tests with a weight-less RMS norm in front of q|k|v: an embedding table, per layer
``wqkv`` and ``wo``, a final weight-less RMS norm and ``lm_head``.  Per layer and position t

    x = rms_norm(h_t);  q|k|v = x @ wqkv.T;  q, k rotated (HF rotate-half) at position pos(t)
    o = softmax(q . K[0..t] / sqrt(head_dim)) V[0..t]   (query head h reads KV head h // (heads // kv_heads))
    h_t += o @ wo.T

with pos(t) = t for a prompt token (t < prompt_len) and t + rope_delta after it.  The cos / sin tables are the 16-bit tables
the device reads, cast to float64: the reference rotates by the same angles.  ``storage="e4m3"`` stores K (after rotation)
and V as clamp(x / s, +-448) -> e4m3fn -> * s with one scale per KV head, K scales first, then V scales.

``reference``  the whole sequence at once under a causal mask;  ``reference_incremental``  the same numbers position by
position with a Python list as the cache (tests/test_generation_reference_cpu.py holds the two together);  ``greedy``  float64
greedy decoding with the top-1 / top-2 margins;  ``plain``  the same model in 16-bit arithmetic on the CPU, one rounding per
op -- the yardstick of every tolerance;  ``MUTATIONS``  the reference with one mistake each.

``CASES`` is the table tests/test_gpu_generation_reference.py runs; its seeds were picked on the CPU by the conditions
tests/test_generation_reference_cpu.py asserts."""
import functools
import math
from collections import namedtuple

import torch

EPS = 1e-6
E4M3_MAX = 448.0
DIM, VOCAB, LAYERS, STEPS = 512, 1001, 2, 16
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}

#: the reference with one mistake each; the name says which
MUTATIONS = ("decode_position_plus_1", "rope_delta_ignored", "newest_key_masked", "gqa_modulo", "kv_scale_halves_swapped",
             "v_one_head_early", "no_softmax_scale")

Geometry = namedtuple("Geometry", "heads kv_heads head_dim")
Weights = namedtuple("Weights", "table lm_head layers geometry dtype")      # layers: [(wqkv, wo)], all in ``dtype`` on the CPU


def rope_tables(rows, head_dim, dtype, base=10000.0):
    """(cos, sin) [rows, head_dim] in ``dtype``: fp32 angles, one rounding -- the formula of ``full_prefill._rope_tables``."""
    inv = 1.0 / (base ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    ang = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None, :]
    ang = torch.cat([ang, ang], dim=-1)
    return ang.cos().to(dtype).contiguous(), ang.sin().to(dtype).contiguous()


def make_weights(seed, geometry, dtype, dim=DIM, vocab=VOCAB, layers=LAYERS):
    """The seeded toy model.  The V rows of ``wqkv`` are a quarter of the K rows' size (and ``wo`` four times its usual size, so the
    attention weighs as much in the residual): K and V then need different e4m3 scales, and a mistake that swaps the two halves
    of ``kv_scales`` clamps K."""
    H, HKV, D = geometry
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape, s=1.0: torch.randn(shape, generator=g) * s
    table, lm_head = rnd(vocab, dim).to(dtype), rnd(vocab, dim, s=0.05).to(dtype)
    ls = []
    for _ in range(layers):
        wqkv = rnd((H + 2 * HKV) * D, dim, s=dim ** -0.5)
        wqkv[(H + HKV) * D:] *= 0.25
        ls.append((wqkv.to(dtype), rnd(dim, H * D, s=4.0 * (H * D) ** -0.5).to(dtype)))
    return Weights(table, lm_head, ls, Geometry(*geometry), dtype)


def make_kv_scales(geometry, layers=LAYERS):
    """Per layer float32 [2 * kv_heads]: K scales (absmax 6 of unit-variance keys) then V scales (a quarter), each head its own."""
    HKV = geometry[1]
    head = 1.0 + 0.125 * torch.arange(HKV, dtype=torch.float32)
    return [torch.cat([6.0 * head, 1.5 * head]) * (1.0 + 0.25 * i) / E4M3_MAX for i in range(layers)]


def make_prompt(seed, length, vocab=VOCAB):
    return torch.randint(0, vocab, (length,), generator=torch.Generator().manual_seed(seed)).tolist()


def positions(T, prompt_len, rope_delta, mutation=None):
    """pos(t) for t < T"""
    delta = 0 if mutation == "rope_delta_ignored" else rope_delta
    extra = 1 if mutation == "decode_position_plus_1" else 0
    return [t if t < prompt_len else t + delta + extra for t in range(T)]


# ---- the float64 pieces ----
def _rms(x):
    return x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + EPS)


def _rotate(x, cos, sin):
    """x [T, heads, D], cos / sin [T, D]: HF rotate-half"""
    half = x.shape[-1] // 2
    rot = torch.cat([-x[..., half:], x[..., :half]], dim=-1)
    return x * cos[:, None, :] + rot * sin[:, None, :]


def e4m3_codes(kv, scales):
    """kv [T, 2 * kv_heads, D], scales [2 * kv_heads] -> the e4m3fn bytes of clamp(kv / s, +-448), uint8"""
    t = (kv.to(torch.float32) / scales.to(torch.float32)[None, :, None]).clamp(-E4M3_MAX, E4M3_MAX)
    return t.to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_values(codes, scales):
    """the float64 values e4m3 bytes [T, 2 * kv_heads, D] stand for"""
    return codes.view(torch.float8_e4m3fn).to(torch.float64) * scales.to(torch.float64)[None, :, None]


def _kv_head(h, geometry, mutation):
    H, HKV, _ = geometry
    return h % HKV if mutation == "gqa_modulo" else h // (H // HKV)


def _v_head(kvh, geometry, mutation):
    return (kvh - 1) % geometry.kv_heads if mutation == "v_one_head_early" else kvh


def _scales_for(kv_scales, layer, geometry, mutation):
    s = kv_scales[layer].to(torch.float64).cpu()
    if mutation == "kv_scale_halves_swapped":
        s = torch.cat([s[geometry.kv_heads:], s[:geometry.kv_heads]])
    return s


def _project(w, layer, h, pos, cos, sin):
    """h [T, dim] float64, pos a list of T positions -> (q [T, H, D] rotated, K|V [T, 2 HKV, D] with K rotated)"""
    H, HKV, D = w.geometry
    T = h.shape[0]
    qkv = (_rms(h) @ w.layers[layer][0].to(torch.float64).t()).view(T, H + 2 * HKV, D)
    c, s = cos[pos].to(torch.float64), sin[pos].to(torch.float64)
    qk = _rotate(qkv[:, :H + HKV], c, s)
    return qk[:, :H], torch.cat([qk[:, H:], qkv[:, H + HKV:]], dim=1)


def _store(kv, storage, scales):
    """what the cache holds of kv: -> (values float64, codes uint8 or None)"""
    if storage == "16bit":
        return kv, None
    codes = e4m3_codes(kv, scales)
    return e4m3_values(codes, scales), codes


def reference(w, ids, prompt_len, rope_delta, *, storage="16bit", kv_scales=None, forced_cache=None, mutation=None):
    """The float64 model over the whole sequence ``ids`` at once, full causal attention.  forced_cache: per layer a float64
    [T, 2 * kv_heads, D] tensor (the dequantised rows of a device's cache) that replaces K|V in the attention.
    -> dict: hidden [T, dim] (pre-norm, after the last layer), logits [T, vocab], kv (per layer [T, 2 HKV, D], the reference's OWN
    K|V as the cache would hold them), codes (per layer uint8, e4m3 only)."""
    assert storage in ("16bit", "e4m3") and (storage == "16bit") == (kv_scales is None) and mutation in (None,) + MUTATIONS
    H, HKV, D = w.geometry
    T = len(ids)
    pos = positions(T, prompt_len, rope_delta, mutation)
    cos, sin = rope_tables(max(pos) + 1, D, w.dtype)
    h = w.table.to(torch.float64)[ids]
    t = torch.arange(T)
    allowed = t[None, :] <= t[:, None]
    if mutation == "newest_key_masked":
        allowed = allowed & ~((t[None, :] == t[:, None]) & (t[:, None] >= prompt_len))
    scale = 1.0 if mutation == "no_softmax_scale" else D ** -0.5
    kvs, codes = [], []
    for i in range(len(w.layers)):
        q, kv = _project(w, i, h, pos, cos, sin)
        kv, c = _store(kv, storage, None if storage == "16bit" else _scales_for(kv_scales, i, w.geometry, mutation))
        kvs.append(kv)
        codes.append(c)
        use = kv if forced_cache is None else forced_cache[i].to(torch.float64)
        o = torch.empty(T, H, D, dtype=torch.float64)
        for hd in range(H):
            kvh = _kv_head(hd, w.geometry, mutation)
            s = (q[:, hd] @ use[:, kvh].t()) * scale
            p = torch.softmax(s.masked_fill(~allowed, -math.inf), dim=-1)
            o[:, hd] = p @ use[:, HKV + _v_head(kvh, w.geometry, mutation)]
        h = h + o.reshape(T, H * D) @ w.layers[i][1].to(torch.float64).t()
    return {"hidden": h, "logits": _rms(h) @ w.lm_head.to(torch.float64).t(), "kv": kvs, "codes": codes}


def reference_incremental(w, ids, prompt_len, rope_delta, *, storage="16bit", kv_scales=None):
    """``reference`` one position at a time, a Python list of rows per layer as the cache -> (hidden [T, dim], logits [T, vocab])"""
    H, HKV, D = w.geometry
    cache = [[] for _ in w.layers]
    hidden = []
    for t, tok in enumerate(ids):
        p = t if t < prompt_len else t + rope_delta
        cos, sin = rope_tables(p + 1, D, w.dtype)
        h = w.table[tok].to(torch.float64)[None]
        for i in range(len(w.layers)):
            q, kv = _project(w, i, h, [p], cos, sin)
            cache[i].append(_store(kv, storage, None if storage == "16bit" else kv_scales[i].to(torch.float64).cpu())[0][0])
            rows = torch.stack(cache[i])                             # [t + 1, 2 HKV, D]
            o = []
            for hd in range(H):
                kvh = hd // (H // HKV)
                prob = torch.softmax((rows[:, kvh] @ q[0, hd]) * D ** -0.5, dim=0)
                o.append(prob @ rows[:, HKV + kvh])
            h = h + torch.cat(o)[None] @ w.layers[i][1].to(torch.float64).t()
        hidden.append(h[0])
    hidden = torch.stack(hidden)
    return hidden, _rms(hidden) @ w.lm_head.to(torch.float64).t()


def margins(logits):
    """logits [T, vocab] -> (argmax [T] as a list, top-1 minus top-2 [T])"""
    top = torch.topk(logits, 2, dim=-1)
    return top.indices[:, 0].tolist(), top.values[:, 0] - top.values[:, 1]


def greedy(w, prompt, rope_delta, steps, **kw):
    """Float64 greedy decoding: -> (ids: the prompt and ``steps`` + 1 picked tokens, margin [steps + 1]: top-1 minus top-2 of every
    pick).  ids[len(prompt) + j] is the token embedded by generation step j; the last one is picked and never embedded."""
    ids, margin = list(prompt), []
    for _ in range(steps + 1):
        logits = reference(w, ids, len(prompt), rope_delta, **kw)["logits"][-1:]
        tok, m = margins(logits)
        ids.append(tok[0])
        margin.append(m[0])
    return ids, torch.stack(margin)


# ---- the same model in honest 16-bit arithmetic: every op reads 16-bit values, computes in fp32 and rounds once ----
def plain(w, ids, prompt_len, rope_delta, *, storage="16bit", kv_scales=None):
    """-> dict like ``reference``'s: hidden, logits and kv in float64 (the 16-bit values), codes for e4m3."""
    H, HKV, D = w.geometry
    dt, f32 = w.dtype, torch.float32
    rnd = lambda x: x.to(dt).to(f32)
    T = len(ids)
    pos = positions(T, prompt_len, rope_delta)
    cos, sin = rope_tables(max(pos) + 1, D, dt)
    cos, sin = cos[pos].to(f32), sin[pos].to(f32)
    causal = torch.ones(T, T, dtype=torch.bool).tril()
    h = w.table[ids].to(f32)
    kvs, codes = [], []
    for i, (wqkv, wo) in enumerate(w.layers):
        x = rnd(h * torch.rsqrt((h * h).mean(dim=-1, keepdim=True) + EPS))
        qkv = rnd(x @ wqkv.to(f32).t()).view(T, H + 2 * HKV, D)
        qk = rnd(_rotate(qkv[:, :H + HKV], cos, sin))
        q, kv = qk[:, :H], torch.cat([qk[:, H:], qkv[:, H + HKV:]], dim=1)
        if storage == "e4m3":
            c = e4m3_codes(kv, kv_scales[i].cpu())
            codes.append(c)
            kv = rnd(c.view(torch.float8_e4m3fn).to(f32) * kv_scales[i].cpu().to(f32)[None, :, None])     # dequantised to 16 bit
            kvs.append(e4m3_values(c, kv_scales[i].cpu()))
        else:
            codes.append(None)
            kvs.append(kv.to(torch.float64))
        o = torch.empty(T, H, D, dtype=f32)
        for hd in range(H):
            kvh = hd // (H // HKV)
            s = (q[:, hd] @ kv[:, kvh].t()) * D ** -0.5
            p = rnd(torch.softmax(s.masked_fill(~causal, -math.inf), dim=-1))
            o[:, hd] = rnd(p @ kv[:, HKV + kvh])
        h = rnd(h + rnd(o.reshape(T, H * D) @ wo.to(f32).t()))
    x = rnd(h * torch.rsqrt((h * h).mean(dim=-1, keepdim=True) + EPS))
    logits = rnd(x @ w.lm_head.to(f32).t())
    return {"hidden": h.to(torch.float64), "logits": logits.to(torch.float64), "kv": kvs, "codes": codes}


def plain_greedy(w, prompt, rope_delta, steps, **kw):
    """``plain`` decoding greedily on its own logits -> (ids like ``greedy``'s, the last ``plain`` result, over ids[:-1])"""
    ids = list(prompt)
    for _ in range(steps + 1):
        out = plain(w, ids, len(prompt), rope_delta, **kw)
        ids.append(int(torch.argmax(out["logits"][-1])))
    return ids, out


# ---- error measures ----
def rel_rows(got, want):
    """row by row ||got - want|| / ||want|| over everything but the first dimension"""
    got, want = got.to(torch.float64).flatten(1), want.to(torch.float64).flatten(1)
    return (got - want).norm(dim=1) / want.norm(dim=1)


def rel_all(got, want):
    got, want = got.to(torch.float64), want.to(torch.float64)
    return float((got - want).norm() / want.norm())


def share_differing(a, b):
    return float((a != b).double().mean())


# ---- the configurations the GPU file runs ----
#: c of "device error <= c * plain's error", per dtype: bounded from the CPU side alone by c * E_plain <= E_mut / 5.  bf16's
#: rounding is 8 times fp16's while the mistakes stay where they are, so its gap leaves room for 1.5 only
C = {"fp16": 3.0, "bf16": 1.5}
Sequence = namedtuple("Sequence", "prompt_seed prompt_len rope_delta")
#: one model (weights seed) per geometry and dtype; four sequences over it: [0] the single-sequence run, [1:] the batch of three.
#: no_gap names the (storage, sequence) pairs that are exempt from the CPU file's mutation gap, and from nothing else: bf16's E_plain
#: is 8 times fp16's, and for the batch's two-token prompt at delta -2 no prompt seed leaves c * E_plain <= E_mut / 5 at c = 1.5 (the
#: nearest mistake, a decode position one too far, moves a query that has three keys very little).  The CPU file asserts that each
#: exemption is needed; the GPU file keeps every assertion there, the hidden bound c * E_plain included -- it still bounds the
#: device by honest arithmetic, it only does not separate that one mistake by the factor 5
Case = namedtuple("Case", "name geometry dtype weights_seed sequences no_gap")
SHAPES = [(5, 3), (5, 0), (8, 3), (2, -2)]          # (prompt length, rope_delta): GreedyLoop's, then GreedyLoopBatch's three


def _case(name, geometry, dtype, weights_seed, prompt_seeds, no_gap=()):
    assert len(prompt_seeds) == len(SHAPES)
    return Case(name, Geometry(*geometry), dtype, weights_seed, [Sequence(s, *shape) for s, shape in zip(prompt_seeds, SHAPES)], tuple(no_gap))


CASES = {c.name: c for c in [
    _case("h4kv2d128-fp16", (4, 2, 128), "fp16", 0, [0, 2, 0, 0]),
    _case("h4kv2d128-bf16", (4, 2, 128), "bf16", 0, [104, 674, 37, 69], no_gap=[("16bit", 3), ("e4m3", 3)]),
    _case("h4kv4d128-fp16", (4, 4, 128), "fp16", 0, [0, 2, 1, 8]),
    _case("h4kv4d128-bf16", (4, 4, 128), "bf16", 0, [209, 35, 37, 106], no_gap=[("16bit", 3)]),
    _case("h4kv4d64-fp16", (4, 4, 64), "fp16", 0, [0, 2, 4, 3]),
]}
#: the decode attention kernels are built for head_dim 128: this geometry's full model is pinned on the CPU; the GPU file holds its
#: layer-0 appends to it
CPU_ONLY = ("h4kv4d64-fp16",)
STORAGES = ("16bit", "e4m3")


@functools.lru_cache(maxsize=None)
def case_weights(name):
    c = CASES[name]
    return make_weights(c.weights_seed, c.geometry, DTYPES[c.dtype])


@functools.lru_cache(maxsize=None)
def yardstick(name, storage, seq):
    """Everything the CPU side knows about one sequence of one case, computed once:
    16bit: ids = float64 greedy decoding, ref = the free-running reference over them, plain teacher-forced on the same ids.
    e4m3:  ids = plain's own greedy decoding, ref = the reference forced on plain's cache."""
    c, w = CASES[name], case_weights(name)
    s = c.sequences[seq]
    prompt = make_prompt(s.prompt_seed, s.prompt_len)
    kw = {"storage": storage, "kv_scales": make_kv_scales(c.geometry) if storage == "e4m3" else None}
    P = s.prompt_len
    if storage == "16bit":
        ids, margin = greedy(w, prompt, s.rope_delta, STEPS, **kw)
        pl = plain(w, ids[:-1], P, s.rope_delta, **kw)
        forced = None
    else:
        ids, pl = plain_greedy(w, prompt, s.rope_delta, STEPS, **kw)
        forced = pl["kv"]
    ref = reference(w, ids[:-1], P, s.rope_delta, forced_cache=forced, **kw)
    if storage == "e4m3":
        margin = margins(ref["logits"][P - 1:])[1]
    gen = slice(P, P + STEPS)
    y = {"prompt": prompt, "ids": ids, "margin": margin, "ref": ref, "plain": pl, "kw": kw, "forced": forced,
         "e_plain": float(rel_rows(pl["hidden"], ref["hidden"])[gen].max()),
         "logit_err": float((pl["logits"] - ref["logits"])[P - 1:].abs().max()),
         "kv_row_err": [rel_rows_kv(a, b, c.geometry.kv_heads) for a, b in zip(pl["kv"], ref["kv"])]}
    if storage == "e4m3":
        HKV = c.geometry.kv_heads
        y["share"] = [(share_differing(a[:, :HKV], b[:, :HKV]), share_differing(a[:, HKV:], b[:, HKV:]))
                      for a, b in zip(pl["codes"], ref["codes"])]
        y["deq_err"] = [(rel_all(a[:, :HKV], b[:, :HKV]), rel_all(a[:, HKV:], b[:, HKV:])) for a, b in zip(pl["kv"], ref["kv"])]
    return y


def rel_rows_kv(got, want, kv_heads):
    """[T, 2 HKV, D] twice -> (K row errors [T], V row errors [T])"""
    return rel_rows(got[:, :kv_heads], want[:, :kv_heads]), rel_rows(got[:, kv_heads:], want[:, kv_heads:])


def mutation_errors(name, storage, seq):
    """{mutation: min over the positions after the prompt of its relative hidden distance from the reference}: over the ids and (e4m3)
    the forced cache of ``yardstick``.  A mutation this sequence cannot see comes out as 0."""
    c, w, y = CASES[name], case_weights(name), yardstick(name, storage, seq)
    s = c.sequences[seq]
    out = {}
    for m in MUTATIONS:
        if m == "kv_scale_halves_swapped" and storage == "16bit":
            out[m] = 0.0
            continue
        mut = reference(w, y["ids"][:-1], s.prompt_len, s.rope_delta, forced_cache=y["forced"], mutation=m, **y["kw"])
        out[m] = float(rel_rows(mut["hidden"], y["ref"]["hidden"])[s.prompt_len:].min())
    return out
