"""A batch whose second sequence lies more than 2^32 bytes behind the first: the batched append and the batched decode attention
reach sequence b through ``kv_cache + b * seq_stride`` in 64-bit arithmetic, while the offsets inside a sequence stay 32-bit.  As in
tests/test_gpu_wide_strides.py one uninitialised buffer of 4 GiB + 16 MiB is viewed with the stride under test, small operands are
written into the view, and everything is compared BIT FOR BIT with the single-sequence calls on compact tensors holding the same
values.  Only bytes the test wrote are ever read."""
import contextlib
import itertools

import pytest
import torch

import attn_decode_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
BIG_BYTES = (4 << 30) + (16 << 20)
SEQ_BYTES = (1 << 32) + (1 << 20)              # from sequence 0's cache to sequence 1's
H, HKV, D = 8, 2, 128
B, T, R = 2, 72, 3
LENGTHS = [37, 72]


@pytest.fixture(scope="module")
def big():
    buf = torch.empty((BIG_BYTES,), dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    yield buf
    del buf
    torch.cuda.empty_cache()


@contextlib.contextmanager
def forced(plan):
    from mquant_amd import ops
    ops.attn_decode_debug_force(*plan)
    try:
        yield
    finally:
        ops.attn_decode_debug_force(0, 0)


def check_the_second_sequence_lies_beyond_4_gib(big, storage):
    from mquant_amd import ops
    from mquant_amd.full_prefill import _rope_tables
    dtype = torch.float16
    el, size = (torch.float8_e4m3fn, 1) if storage == "e4m3" else (dtype, 2)
    qkv_all, _, cache8, scale = cases.make_case(B * T + H, B * T, H, HKV, dtype, DEV)
    if storage == "e4m3":
        compact = cache8.view(B, T, 2 * HKV, D).clone()
    else:
        compact, scale = qkv_all[:, H * D:].reshape(B, T, 2 * HKV, D).contiguous(), None
    cos, sin = _rope_tables(T + 8, D, torch.device(DEV), dtype)
    cos, sin = cos[:, 0].contiguous(), sin[:, 0].contiguous()

    wide = torch.as_strided(big.view(el), (B, T, 2 * HKV, D), (SEQ_BYTES // size, 2 * HKV * D, D, 1))
    assert wide.data_ptr() == big.data_ptr() and wide[1].data_ptr() - big.data_ptr() == SEQ_BYTES > 1 << 32
    assert SEQ_BYTES + T * 2 * HKV * D * size <= BIG_BYTES
    wide.view(torch.uint8).copy_(compact.view(torch.uint8))
    assert torch.equal(wide.view(torch.uint8), compact.view(torch.uint8))

    n_keys = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    delta = torch.tensor([2, -1], dtype=torch.int32, device=DEV)
    rows = torch.cat([qkv_all[b * T + n - R:b * T + n] for b, n in enumerate(LENGTHS)])          # [B R, ...]: each sequence's newest rows

    def append(batch, qkv, caches, n, d):
        if storage == "e4m3":
            return (ops.kv_append_rope_fp8_batch if batch else ops.kv_append_rope_fp8)(qkv, H, caches, scale, cos, sin, n_keys=n, rope_delta=d)
        return (ops.kv_append_rope_batch if batch else ops.kv_append_rope)(qkv, H, caches, cos, sin, n_keys=n, rope_delta=d)

    def attend(batch, q, caches, n):
        if storage == "e4m3":
            return (ops.attn_decode_fp8kv_batch if batch else ops.attn_decode_fp8kv)(q, caches, scale, n_keys=n)
        return (ops.attn_decode_batch if batch else ops.attn_decode)(q, caches, n_keys=n)

    got = rows.clone()
    append(True, got, wide, n_keys, delta)
    want = rows.clone()
    for b in range(B):
        append(False, want[b * R:(b + 1) * R], compact[b], n_keys[b:b + 1], delta[b:b + 1])
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and not torch.equal(got.view(torch.int16), rows.view(torch.int16))
    assert torch.equal(wide.view(torch.uint8), compact.view(torch.uint8))

    q = got[:, :H * D].view(B, R, H, D)
    for plan in [(1, 0), (0, 32), (0, 0)]:
        with forced(plan):
            o = attend(True, q, wide, n_keys)
            for b in range(B):
                alone = attend(False, q[b], compact[b], n_keys[b:b + 1])
                assert torch.equal(o[b * R:(b + 1) * R].view(torch.int16), alone.view(torch.int16)), (plan, b)
                there = attend(False, q[b], wide[b], n_keys[b:b + 1])
                assert torch.equal(there.view(torch.int16), alone.view(torch.int16)), (plan, b)
    assert not torch.equal(o[:R], o[R:])


def _sweep(check, **axes):
    """check(**case) for every combination of the axes; a failure names its case"""
    for values in itertools.product(*axes.values()):
        case = dict(zip(axes, values))
        try:
            check(**case)
        except AssertionError as e:
            raise AssertionError(f"{check.__name__} {case}: {e}") from e


def test_the_second_sequence_lies_beyond_4_gib(big):
    _sweep(check_the_second_sequence_lies_beyond_4_gib, big=[big], storage=["e4m3", "16bit"])
