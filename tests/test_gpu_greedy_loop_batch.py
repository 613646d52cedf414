"""``GreedyLoopBatch`` (mquant_amd/generate.py) on the GPU, over both batched cache classes: the toy decoder of
tests/test_gpu_greedy_loop.py (dim 512, 4 heads, 2 kv heads, head_dim 128, vocab 1001, caches of 64 rows, two layers) for B = 3
sequences whose prompts hold 5, 17 and 33 rows, six steps.

The reference is a host loop over THREE SINGLE-SEQUENCE caches in which everything else is batched exactly as in the loop under
test -- the same ``F.linear`` on [3, dim], the same ``F.rms_norm``, ``ops.gemv_f16`` on [3, dim], the CPU ``argmax`` -- so only the
cache step differs.  At 64 rows both plans are one key range, so everything compared is integers or bytes: the ids, the id log,
the key counts, the cache rows."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DIM, H, HKV, D, VOCAB, CAP, LAYERS = 512, 4, 2, 128, 1001, 64, 2
B, PROMPTS, FIRST, STEPS, EPS = 3, [5, 17, 33], [123, 7, 900], 6, 1e-6
DELTAS = [0, 4, -2]
STORAGES = ["e4m3", "16bit"]


@functools.lru_cache(maxsize=None)
def _weights():
    """(embedding table, lm_head, per layer (wqkv, wo), per layer kv scales, cos, sin, per layer and sequence the prefill K|V rows)"""
    from mquant_amd.full_prefill import _rope_tables
    g = torch.Generator(device=DEV).manual_seed(2025)
    rnd = lambda *shape, s=1.0: (torch.randn(shape, generator=g, device=DEV) * s).half()
    table, lm_head = rnd(VOCAB, DIM), rnd(VOCAB, DIM, s=0.05)
    layers = [(rnd((H + 2 * HKV) * D, DIM, s=DIM ** -0.5), rnd(DIM, H * D, s=(H * D) ** -0.5)) for _ in range(LAYERS)]
    scales = [torch.full((2 * HKV,), 4.0 / 448.0, device=DEV) * (1.0 + 0.25 * i) for i in range(LAYERS)]
    cos, sin = _rope_tables(CAP + 8, D, DEV, torch.float16)
    prefill = [[rnd(n, 2 * HKV, D) for n in PROMPTS] for _ in range(LAYERS)]
    return table, lm_head, layers, scales, cos[:, 0].contiguous(), sin[:, 0].contiguous(), prefill


def _plans_are_one_range():
    from mquant_amd import ops
    assert ops.attn_decode_plan(1, CAP, H, HKV)["splits"] == 1 == ops.attn_decode_batch_plan(B, 1, CAP, H, HKV)["splits"]


def _batched_model(storage):
    """(a fresh prefilled batched cache, the body over it)"""
    from mquant_amd import Fp8KVCacheBatch, KVCache16Batch
    _, _, layers, scales, cos, sin, prefill = _weights()
    if storage == "e4m3":
        cache = Fp8KVCacheBatch(B, LAYERS, CAP, HKV, D, scales, cos, sin, DEV, torch.float16, rope_delta=DELTAS)
    else:
        cache = KVCache16Batch(B, LAYERS, CAP, HKV, D, cos, sin, DEV, torch.float16, rope_delta=DELTAS)
    for i in range(LAYERS):
        for b in range(B):
            cache.fill(i, b, prefill[i][b])

    def body(h):
        for i, (wqkv, wo) in enumerate(layers):
            o = cache.step(i, F.linear(h, wqkv), H)
            h = h + F.linear(o, wo)
        return h
    return cache, body


@functools.lru_cache(maxsize=None)
def _host_loop(storage, steps=STEPS + 2):
    """the reference: -> (ids embedded per sequence [B][steps], the ids picked last [B], per layer and sequence the cache bytes)"""
    from mquant_amd import Fp8KVCache, KVCache16, ops
    table, lm_head, layers, scales, cos, sin, prefill = _weights()
    caches = []
    for b in range(B):
        if storage == "e4m3":
            c = Fp8KVCache(LAYERS, CAP, HKV, D, scales, cos, sin, DEV, torch.float16, rope_delta=DELTAS[b])
        else:
            c = KVCache16(LAYERS, CAP, HKV, D, cos, sin, DEV, torch.float16, rope_delta=DELTAS[b])
        for i in range(LAYERS):
            c.fill(i, prefill[i][b])
        c.set_length(PROMPTS[b])
        caches.append(c)
    tokens, embedded = list(FIRST), [[] for _ in range(B)]
    for _ in range(steps):
        for b in range(B):
            embedded[b].append(tokens[b])
            caches[b].advance(1)
        h = table[tokens].clone()
        for i, (wqkv, wo) in enumerate(layers):
            qkv = F.linear(h, wqkv)
            o = torch.cat([caches[b].step(i, qkv[b:b + 1], H) for b in range(B)])
            h = h + F.linear(o, wo)
        logits = ops.gemv_f16(F.rms_norm(h, (DIM,), eps=EPS), lm_head)
        tokens = torch.argmax(logits.cpu(), dim=1).tolist()
    rows = [[caches[b].caches[i].view(torch.uint8).clone() for b in range(B)] for i in range(LAYERS)]
    return embedded, tokens, rows


def _loop(storage):
    from mquant_amd import GreedyLoopBatch
    table, lm_head = _weights()[:2]
    cache, body = _batched_model(storage)
    return GreedyLoopBatch(cache, table, lm_head, body, eps=EPS), cache


def _check_state(loop, cache, storage, steps):
    """after `steps` steps from the start: log, key counts, the tokens left and the cache rows, against the reference at that point"""
    embedded, _, _ = _host_loop(storage)
    ids = loop.ids.cpu()
    for b, n in enumerate(PROMPTS):
        want = [0] * n + embedded[b][:steps] + [0] * (CAP - n - steps)
        assert ids[b].tolist() == want, b                             # nothing else is logged
    assert cache.n_keys.cpu().tolist() == [n + steps for n in PROMPTS]
    if steps < len(embedded[0]):
        assert loop.token.cpu().tolist() == [embedded[b][steps] for b in range(B)]
    # cache rows [0, n + steps): those of the reference, which only ever APPENDS -- its later rows are not compared
    rows = _host_loop(storage)[2]
    for i in range(LAYERS):
        for b, n in enumerate(PROMPTS):
            assert torch.equal(cache.caches[i].view(torch.uint8)[b, :n + steps], rows[i][b][:n + steps]), (i, b)


def check_eager_steps_equal_the_host_loop_over_single_caches(storage):
    _plans_are_one_range()
    embedded, _, _ = _host_loop(storage)
    print("host loop ids", embedded)
    assert [e[0] for e in embedded] == FIRST and all(0 <= t < VOCAB for e in embedded for t in e)
    loop, cache = _loop(storage)
    loop.start(PROMPTS, FIRST)
    for _ in range(STEPS):
        loop.step()
    _check_state(loop, cache, storage, STEPS)


def check_graph_replays_equal_the_host_loop_and_continue(capture_first, storage):
    embedded, _, _ = _host_loop(storage)
    loop, cache = _loop(storage)
    if capture_first:
        loop.capture()
        loop.start(PROMPTS, FIRST)
    else:
        loop.start(PROMPTS, FIRST)
        before = [c.view(torch.uint8).clone() for c in cache.caches]
        loop.capture()
        assert cache.n_keys.cpu().tolist() == PROMPTS and loop.token.cpu().tolist() == FIRST      # capture() restored both ...
        assert all(torch.equal(c.view(torch.uint8), b) for c, b in zip(cache.caches, before))    # ... and every cache row
        assert int(loop.ids.abs().sum()) == 0                                                      # ... and the log
    got = loop.generate(STEPS)
    assert got.dtype == torch.int32 and got.device.type == "cpu" and got.shape == (B, STEPS)
    assert got.tolist() == [e[:STEPS] for e in embedded]
    _check_state(loop, cache, storage, STEPS)
    more = loop.generate(2)                                           # on from where it stands
    assert more.tolist() == [e[STEPS:STEPS + 2] for e in embedded]
    _check_state(loop, cache, storage, STEPS + 2)
    # the same graph from the same start once more
    loop.start(PROMPTS, FIRST)
    assert loop.generate(STEPS).tolist() == [e[:STEPS] for e in embedded]


def check_generate_refuses_to_leave_the_shortest_remaining_capacity(storage):
    loop, _ = _loop(storage)
    loop.start([5, CAP - 2, 33], FIRST)
    with pytest.raises(AssertionError, match="exceed the cache"):
        loop.generate(3)
    assert loop.generate(0).shape == (B, 0)
    with pytest.raises(AssertionError, match="3 sequences need 3"):
        loop.start([5, 17], FIRST)


def _sweep(check, **axes):
    """check(**case) for every combination of the axes; a failure names its case"""
    for values in itertools.product(*axes.values()):
        case = dict(zip(axes, values))
        try:
            check(**case)
        except AssertionError as e:
            raise AssertionError(f"{check.__name__} {case}: {e}") from e


def test_the_batched_greedy_loop_over_both_cache_classes():
    """every case of this file in one test (they share the host loop's reference); a failure names the check and its case"""
    _sweep(check_eager_steps_equal_the_host_loop_over_single_caches, storage=STORAGES)
    _sweep(check_graph_replays_equal_the_host_loop_and_continue, capture_first=[True, False], storage=STORAGES)
    _sweep(check_generate_refuses_to_leave_the_shortest_remaining_capacity, storage=STORAGES)
