"""``GreedyLoop`` (mquant_amd/generate.py) over a ``KVCache16`` on the GPU: the loop is written against the cache's interface, not
against its storage, and this file shows it for the 16-bit cache with the toy model of tests/test_gpu_greedy_loop.py, restated here:
a two-layer body on fixed random fp16 weights (dim 512, 4 heads, 2 kv heads, head_dim 128, vocab 1001, a cache of 64 rows whose
rows [0, 5) are prefilled): per layer a torch ``F.linear`` to q|k|v, ``cache.step``, a ``F.linear`` back plus the residual.  From the
same start six tokens are generated three ways --

  (i)   a host loop: ``gemv_f16``, the CPU ``argmax``, ``table[token]``, ``cache.advance`` and the body by hand;
  (ii)  ``GreedyLoop.step()`` six times, eager;
  (iii) ``capture()`` + ``generate(6)``: six replays of one graph, one copy at the end, in both capture orders

-- and everything compared is integers or bytes: the id sequences, the id log, the key count, the cache rows."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DIM, H, HKV, D, VOCAB, CAP, LAYERS = 512, 4, 2, 128, 1001, 64, 2
PROMPT, FIRST, STEPS, EPS = 5, 123, 6, 1e-6
POISON = 0x7E00             # an fp16 NaN, as int16


@functools.lru_cache(maxsize=None)
def _weights():
    """(embedding table, lm_head, per layer (wqkv, wo), cos, sin, prefill K|V rows per layer): never written to"""
    from mquant_amd.full_prefill import _rope_tables
    g = torch.Generator(device=DEV).manual_seed(2024)
    rnd = lambda *shape, s=1.0: (torch.randn(shape, generator=g, device=DEV) * s).half()
    table, lm_head = rnd(VOCAB, DIM), rnd(VOCAB, DIM, s=0.05)
    layers = [(rnd((H + 2 * HKV) * D, DIM, s=DIM ** -0.5), rnd(DIM, H * D, s=(H * D) ** -0.5)) for _ in range(LAYERS)]
    cos, sin = _rope_tables(CAP, D, DEV, torch.float16)
    prefill = [rnd(PROMPT, 2 * HKV, D) for _ in range(LAYERS)]
    return table, lm_head, layers, cos[:, 0].contiguous(), sin[:, 0].contiguous(), prefill


def _model():
    """(a fresh prefilled cache whose other rows hold NaN patterns, the body over it)"""
    from mquant_amd import KVCache16
    table, lm_head, layers, cos, sin, prefill = _weights()
    cache = KVCache16(LAYERS, CAP, HKV, D, cos, sin, DEV, torch.float16)
    for i in range(LAYERS):
        cache.caches[i].view(torch.int16)[:] = POISON                 # nothing at or beyond n_keys may matter
        cache.fill(i, prefill[i])

    def body(h):
        for i, (wqkv, wo) in enumerate(layers):
            o = cache.step(i, F.linear(h, wqkv), H)
            h = h + F.linear(o, wo)
        return h
    return cache, body


def _rows(cache, a, b):
    return [c.view(torch.int16)[a:b].clone() for c in cache.caches]


@functools.lru_cache(maxsize=None)
def _host_loop():
    """(i): (the ids embedded at positions 5 .. 10, the id picked last, cache rows [0, 11) per layer) -- a host round trip per token"""
    from mquant_amd import ops
    table, lm_head = _weights()[:2]
    cache, body = _model()
    cache.set_length(PROMPT)
    token, embedded = FIRST, []
    for _ in range(STEPS):
        embedded.append(token)
        cache.advance(1)
        h = body(table[token][None].clone())
        logits = ops.gemv_f16(F.rms_norm(h, (DIM,), eps=EPS), lm_head)
        token = int(torch.argmax(logits.cpu(), dim=1))
    assert int(cache.n_keys.item()) == PROMPT + STEPS
    return embedded, token, _rows(cache, 0, PROMPT + STEPS)


def _loop():
    from mquant_amd import GreedyLoop
    table, lm_head = _weights()[:2]
    cache, body = _model()
    return GreedyLoop(cache, table, lm_head, body, eps=EPS), cache


def test_eager_steps_equal_the_host_loop():
    _loop_wants_the_cache_in_the_models_dtype()
    embedded, last, host_rows = _host_loop()
    print("host loop ids", embedded, "then", last)
    assert embedded[0] == FIRST and all(0 <= t < VOCAB for t in embedded + [last]) and len(set(embedded + [last])) > 2
    loop, cache = _loop()
    loop.start(PROMPT, FIRST)
    for _ in range(STEPS):
        loop.step()
    ids = loop.ids.cpu().tolist()
    assert ids[PROMPT:PROMPT + STEPS] == embedded and int(loop.token.item()) == last
    assert ids[:PROMPT] == [0] * PROMPT and ids[PROMPT + STEPS:] == [0] * (CAP - PROMPT - STEPS)       # nothing else is logged
    assert int(cache.n_keys.item()) == PROMPT + STEPS
    for a, b in zip(_rows(cache, 0, PROMPT + STEPS), host_rows):
        assert torch.equal(a, b)
    for c in cache.caches:                                            # nothing beyond the last position was written
        assert bool((c.view(torch.int16)[PROMPT + STEPS:] == POISON).all())


@pytest.mark.parametrize("capture_first", [True, False], ids=["capture-then-start", "start-then-capture"])
def test_graph_replays_equal_eager_steps_and_the_host_loop(capture_first):
    embedded, last, host_rows = _host_loop()
    eager, eager_cache = _loop()
    eager.start(PROMPT, FIRST)
    assert eager.generate(STEPS).tolist() == embedded                 # not captured: generate() steps eagerly

    loop, cache = _loop()
    before = _rows(cache, 0, CAP)
    if capture_first:
        loop.capture()
        assert int(cache.n_keys.item()) == 0
        loop.start(PROMPT, FIRST)
    else:
        loop.start(PROMPT, FIRST)
        loop.capture()
        assert int(cache.n_keys.item()) == PROMPT and int(loop.token.item()) == FIRST      # capture() restored both
    for a, b in zip(_rows(cache, 0, CAP), before):                    # ... and the cache row of the warm-up's position, bit for bit
        assert torch.equal(a, b)
    assert loop.ids.cpu().tolist() == [0] * CAP
    got = loop.generate(STEPS)
    assert got.dtype == torch.int32 and got.device.type == "cpu"
    assert got.tolist() == embedded and int(loop.token.item()) == last
    assert loop.ids[PROMPT:PROMPT + STEPS].cpu().tolist() == [FIRST] + embedded[1:]
    assert int(cache.n_keys.item()) == PROMPT + STEPS == int(eager_cache.n_keys.item())
    for a, b, c in zip(_rows(cache, 0, PROMPT + STEPS), _rows(eager_cache, 0, PROMPT + STEPS), host_rows):
        assert torch.equal(a, b) and torch.equal(a, c)
    # the same graph from the same start once more, then on from where it stands
    loop.start(PROMPT, FIRST)
    assert loop.generate(STEPS).tolist() == embedded and int(loop.token.item()) == last
    more = loop.generate(2)
    assert more[0].item() == last and int(cache.n_keys.item()) == PROMPT + STEPS + 2
    assert loop.ids[PROMPT + STEPS:PROMPT + STEPS + 2].cpu().tolist() == more.tolist()


def _loop_wants_the_cache_in_the_models_dtype():
    from mquant_amd import GreedyLoop, KVCache16
    table, lm_head, _, cos, sin, _ = _weights()
    cache = KVCache16(1, CAP, HKV, D, cos, sin, DEV, torch.bfloat16)
    with pytest.raises(AssertionError):
        GreedyLoop(cache, table, lm_head, lambda h: h)
