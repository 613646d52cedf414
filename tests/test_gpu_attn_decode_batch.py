"""Decode attention over a BATCH of caches (mq_attn_decode_fp8kv_batch, mq_attn_decode_batch and their fused-quantizer forms;
csrc/attn_decode.hip) on the GPU.  Six sequences of capacity 320 with lengths 1, 31, 32, 33, 97 and 320 on the device: under every
forced plan sequence b has the BITS of the single-sequence entry point on cache[b] with its own length, under the heuristic plan
every element is within the bound of tests/attn_decode_reference.py, and what lies at or beyond a sequence's length, in the
workspace before the call, around the output or in ANOTHER sequence cannot change a bit of it."""
import contextlib
import itertools
import functools

import pytest
import torch

import attn_decode_cases as cases
from attn_decode_reference import decode_reference, dequant_cache
from attn_reference import assert_within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DTYPES = [torch.float16, torch.bfloat16]
GEOMETRIES = [(28, 4), (4, 2)]
STORAGES = ["e4m3", "16bit"]
T, B, D = 320, 6, 128
LENGTHS = {1: [1, 31, 32, 33, 97, 320], 3: [3, 31, 32, 33, 97, 320]}       # by R: a sequence holds at least its R rows
PLANS = [(1, 0), (0, 32), (0, 128)]


@contextlib.contextmanager
def forced(plan):
    from mquant_amd import ops
    ops.attn_decode_debug_force(*plan)
    try:
        yield
    finally:
        ops.attn_decode_debug_force(0, 0)


@functools.lru_cache(maxsize=None)
def _inputs(dtype, H, HKV, storage):
    """(q of every position [B, T, H, 128], caches [B, T, 2 HKV, 128] in the storage, scale or None): made once, never written to"""
    qkv, q, cache8, scale = cases.make_case(B * T + H, B * T, H, HKV, dtype, DEV)
    if storage == "e4m3":
        return q.reshape(B, T, H, D), cache8.view(B, T, 2 * HKV, D), scale
    return q.reshape(B, T, H, D), qkv[:, H * D:].reshape(B, T, 2 * HKV, D).contiguous(), None


def _queries(q_all, lengths, R):
    """[B, R, H, 128]: of every sequence the rows of its last R positions"""
    return torch.stack([q_all[b, n - R:n] for b, n in enumerate(lengths)])


def _counts(lengths):
    return torch.tensor(lengths, dtype=torch.int32, device=DEV)


def batched(q, cache, scale, n_keys, **kw):
    from mquant_amd import ops
    if scale is not None:
        return ops.attn_decode_fp8kv_batch(q, cache, scale, n_keys=n_keys, **kw)
    return ops.attn_decode_batch(q, cache, n_keys=n_keys, **kw)


def single(q, cache, scale, n_keys, **kw):
    from mquant_amd import ops
    if scale is not None:
        return ops.attn_decode_fp8kv(q, cache, scale, n_keys=n_keys, **kw)
    return ops.attn_decode(q, cache, n_keys=n_keys, **kw)


def bits(t):
    return t.contiguous().view(torch.int16)


def check_ragged_lengths_give_the_bits_of_the_single_sequence_call(plan, R, geometry, storage, dtype):
    H, HKV = geometry
    from mquant_amd import ops
    q_all, cache, scale = _inputs(dtype, H, HKV, storage)
    lengths = LENGTHS[R]
    q, n_keys = _queries(q_all, lengths, R), _counts(lengths)
    with forced(plan):
        p = ops.attn_decode_batch_plan(B, R, T, H, HKV)
        assert plan[0] in (0, p["splits"]) and plan[1] in (0, p["keys_per_split"]) and p["grid"] == B * HKV * p["splits"]
        got = batched(q, cache, scale, n_keys)
        want = [single(q[b], cache[b], scale, n_keys[b:b + 1]) for b in range(B)]         # the same capacity: the same plan
    assert got.shape == (B * R, H * D) and bool(torch.isfinite(got).all())
    for b in range(B):
        assert torch.equal(bits(got[b * R:(b + 1) * R]), bits(want[b])), (b, lengths[b])
    assert not torch.equal(bits(got[:R]), bits(got[R:2 * R]))


def check_the_heuristic_plan_is_within_the_bound(R, geometry, storage, dtype):
    H, HKV = geometry
    from mquant_amd import ops
    q_all, cache, scale = _inputs(dtype, H, HKV, storage)
    lengths = LENGTHS[R]
    q = _queries(q_all, lengths, R)
    assert ops.attn_decode_batch_plan(B, R, T, H, HKV)["splits"] > 1          # short sequences leave ranges empty that the long one uses
    got = batched(q, cache, scale, _counts(lengths))
    for b, n in enumerate(lengths):
        if scale is not None:
            k, v = dequant_cache(cache[b, :n], scale)
        else:
            k, v = cache[b, :n, :HKV], cache[b, :n, HKV:]
        o, bound = decode_reference(q[b], k, v, True)
        assert_within(got[b * R:(b + 1) * R], o, bound, f"sequence {b} of {n} keys")


def check_nothing_beyond_a_length_in_the_workspace_or_in_another_sequence_matters(plan, storage):
    from mquant_amd import ops
    H, HKV, R, dtype = 28, 4, 1, torch.float16
    q_all, cache, scale = _inputs(dtype, H, HKV, storage)
    lengths = LENGTHS[R]
    q, n_keys = _queries(q_all, lengths, R), _counts(lengths)
    with forced(plan):
        clean = batched(q, cache, scale, n_keys)
        need = ops.attn_decode_batch_workspace_bytes(B, R, T, H, HKV)
        assert (need > 0) == (plan != (1, 0))

        # rows at or beyond each length hold NaNs, the workspace holds NaNs, the output lies between canaries
        dirty = cache.clone()
        for b, n in enumerate(lengths):
            if storage == "e4m3":
                dirty.view(torch.uint8)[b, n:] = 0x7F
            else:
                dirty[b, n:] = float("nan")
        ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=DEV)
        ws[need:] = 0xA5
        wide = torch.full((B * R + 2, H * D + 64), 7.0, dtype=dtype, device=DEV)
        batched(q, dirty, scale, n_keys, out=wide[1:B * R + 1, :H * D], workspace=ws[:need] if need else None)
        assert torch.equal(bits(wide[1:B * R + 1, :H * D]), bits(clean))
        assert bool((wide[0] == 7.0).all()) and bool((wide[B * R + 1] == 7.0).all()) and bool((wide[:, H * D:] == 7.0).all())
        assert bool((ws[need:] == 0xA5).all())
        if need:
            with pytest.raises(Exception, match=f"workspace of {need} bytes"):
                batched(q, dirty, scale, n_keys, workspace=ws[:need - 16])

        # sequences 1 and 4 change places -- q rows, cache, length: so do their outputs, and no other bit moves
        perm = [0, 4, 2, 3, 1, 5]
        swapped = batched(q[perm].contiguous(), dirty.view(torch.uint8)[perm].view(dirty.dtype), scale, n_keys[perm].contiguous())
    assert torch.equal(bits(swapped.view(B, R, -1)), bits(clean.view(B, R, -1)[perm]))
    assert not torch.equal(bits(clean[R:2 * R]), bits(clean[4 * R:5 * R]))


def check_the_fused_quantizer_equals_batched_decode_then_quantize(plan, tiled, storage, dtype):
    """B R = 18 rows: the tiled layout's second 16-row tile is reached, by global row; a scale per row through row_sel"""
    from mquant_amd import ops
    H, HKV, R = 28, 4, 3
    q_all, cache, scale = _inputs(dtype, H, HKV, storage)
    lengths = LENGTHS[R]
    q, n_keys = _queries(q_all, lengths, R), _counts(lengths)
    sel = (torch.arange(B * R, device=DEV) * 7 % 3 == 0).to(torch.uint8)
    with forced(plan):
        o = batched(q, cache, scale, n_keys)
        s0 = float(o.float().abs().max()) / 127.0 * 0.8               # some values saturate
        s1 = 0.37 * s0
        got = ops.attn_decode_quant_i8_batch(q, cache, scale, s0, s1, n_keys=n_keys, row_sel=sel, tiled=tiled)
    want, _ = ops.quantize_act_i8(o, s0, s1, row_sel=sel, tiled=tiled)
    a = got.to_rows() if tiled else got
    b = want.to_rows() if tiled else want
    assert a.shape == b.shape == (B * R, H * D)
    assert torch.equal(a, b)
    assert int(a.abs().max()) >= 127 and 0 < int(sel.sum()) < B * R


def check_the_device_clamps_hold_per_sequence(plan, storage):
    """n_keys[b] = 0 counts as R and T + 5 as T -- for that sequence only"""
    H, HKV, R, dtype = 4, 2, 3, torch.float16
    q_all, cache, scale = _inputs(dtype, H, HKV, storage)
    asked, meant = [0, 97, T + 5, 33, -7, 2], [R, 97, T, 33, R, R]
    q = _queries(q_all, meant, R)
    with forced(plan):
        got = batched(q, cache, scale, _counts(asked))
        want = batched(q, cache, scale, _counts(meant))
        alone = single(q[2], cache[2], scale, T)
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(got[2 * R:3 * R]), bits(alone))
    # and no key count at all: every sequence holds T keys
    with forced(plan):
        full = batched(_queries(q_all, [T] * B, R), cache, scale, None)
    assert torch.equal(bits(full[2 * R:3 * R]), bits(alone))


def check_one_captured_graph_advances_appends_and_attends_over_four_positions(storage):
    """advance -> batched append -> batched attention as one graph, replayed at four positions, against the same steps run eagerly"""
    from mquant_amd import Fp8KVCacheBatch, KVCache16Batch
    from mquant_amd.full_prefill import _rope_tables
    H, HKV, dtype, steps, Bc = 4, 2, torch.float16, 4, 3
    starts = [5, 31, 120]
    qkv_all, _, _, scale = cases.make_case(99, Bc * (T + steps), H, HKV, dtype, DEV)
    qkv_all = qkv_all.view(Bc, T + steps, -1)
    cos, sin = _rope_tables(T, D, torch.device(DEV), dtype)
    cos, sin = cos[:, 0].contiguous(), sin[:, 0].contiguous()

    def make():
        if storage == "e4m3":
            c = Fp8KVCacheBatch(Bc, 1, T, HKV, D, [scale], cos, sin, DEV, dtype, rope_delta=[0, 3, -2])
        else:
            c = KVCache16Batch(Bc, 1, T, HKV, D, cos, sin, DEV, dtype, rope_delta=[0, 3, -2])
        for b, n in enumerate(starts):
            c.fill(0, b, qkv_all[b, :n, H * D:].reshape(n, 2 * HKV, D))
        c.set_length(starts)
        return c

    def new_rows(i):
        return torch.stack([qkv_all[b, starts[b] + i] for b in range(Bc)])

    eager, outs = make(), []
    for i in range(steps):
        eager.advance(1)
        outs.append(eager.step(0, new_rows(i).clone(), H))

    cache = make()
    qkv = new_rows(0).clone()
    out = torch.zeros((Bc, H * D), dtype=dtype, device=DEV)
    cache.advance(1)
    cache.step(0, qkv, H, out=out)                                    # warm-up: workspace and one-time checks
    cache.set_length(starts)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.advance(1)
        cache.step(0, qkv, H, out=out)
    for i in range(steps):
        qkv.copy_(new_rows(i))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(outs[i])), i
    assert cache.n_keys.cpu().tolist() == [n + steps for n in starts] == eager.n_keys.cpu().tolist()
    assert torch.equal(cache.caches[0].view(torch.uint8), eager.caches[0].view(torch.uint8))


def _sweep(check, **axes):
    """check(**case) for every combination of the axes; a failure names its case"""
    for values in itertools.product(*axes.values()):
        case = dict(zip(axes, values))
        try:
            check(**case)
        except AssertionError as e:
            raise AssertionError(f"{check.__name__} {case}: {e}") from e


def test_decode_attention_over_a_batch_of_caches():
    """every case of this file in one test: the cases are milliseconds each, and a failure names the check and its case"""
    both = dict(storage=STORAGES, dtype=DTYPES)
    _sweep(check_ragged_lengths_give_the_bits_of_the_single_sequence_call, plan=PLANS, R=[1, 3], geometry=GEOMETRIES, **both)
    _sweep(check_the_heuristic_plan_is_within_the_bound, R=[1, 3], geometry=GEOMETRIES, **both)
    _sweep(check_nothing_beyond_a_length_in_the_workspace_or_in_another_sequence_matters, plan=[(1, 0), (0, 32), (0, 0)], storage=STORAGES)
    _sweep(check_the_fused_quantizer_equals_batched_decode_then_quantize, plan=[(1, 0), (0, 32)], tiled=[True, False], **both)
    _sweep(check_the_device_clamps_hold_per_sequence, plan=[(1, 0), (0, 32)], storage=STORAGES)
    _sweep(check_one_captured_graph_advances_appends_and_attends_over_four_positions, storage=STORAGES)
