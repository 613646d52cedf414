"""The batched append (mq_kv_append_rope_fp8_batch, mq_kv_append_rope_batch; csrc/kv_append.hip) on the GPU: three sequences at
distinct positions with distinct RoPE offsets in ONE launch.  The qkv bits and the cache bytes of sequence b are those of the
single-sequence entry point on a copy, and every other byte of the whole cache buffer -- the padding behind a row, the gap between
two sequences' caches, the rows of other positions -- keeps its canary."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DTYPES = [torch.float16, torch.bfloat16]
STORAGES = ["e4m3", "16bit"]
H, HKV, D = 4, 2, 128
B, T, TABLE_ROWS = 3, 40, 48
LD_PAD, GAP = 64, 3              # elements of padding behind a cache row, rows of gap between two sequences' caches
CANARY = 0x5A


def _tables(dtype):
    from mquant_amd.full_prefill import _rope_tables
    cos, sin = _rope_tables(TABLE_ROWS, D, torch.device(DEV), dtype)
    return cos[:, 0].contiguous(), sin[:, 0].contiguous()


def _buffers(storage, dtype, padded):
    """(the whole buffer as bytes, its caches [B, T, 2 HKV, D] -- a view with a padded row stride and a gap between the sequences)"""
    el = torch.float8_e4m3fn if storage == "e4m3" else dtype
    size = 1 if storage == "e4m3" else 2
    ld = 2 * HKV * D + (LD_PAD if padded else 0)
    seq = (T + (GAP if padded else 0)) * ld
    raw = torch.full((B * seq * size + 64,), CANARY, dtype=torch.uint8, device=DEV)
    caches = raw[:B * seq * size].view(el).view(B, seq)[:, :T * ld].unflatten(1, (T, ld))[:, :, :2 * HKV * D].unflatten(2, (2 * HKV, D))
    assert caches.stride() == (seq, ld, D, 1) and caches.data_ptr() == raw.data_ptr()
    return raw, caches


def _append(storage, batch, qkv, caches, scale, cos, sin, n_keys, rope_delta):
    from mquant_amd import ops
    if storage == "e4m3":
        fn = ops.kv_append_rope_fp8_batch if batch else ops.kv_append_rope_fp8
        return fn(qkv, H, caches, scale, cos, sin, n_keys=n_keys, rope_delta=rope_delta)
    fn = ops.kv_append_rope_batch if batch else ops.kv_append_rope
    return fn(qkv, H, caches, cos, sin, n_keys=n_keys, rope_delta=rope_delta)


def _ints(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _check(storage, dtype, R, padded, rotate, counts, deltas, meant=None):
    """one batched call against B single-sequence calls on copies; returns the batched buffer"""
    g = torch.Generator(device=DEV).manual_seed(R * 100 + len(storage))
    qkv = (torch.randn((B * R, (H + 2 * HKV) * D + 16), generator=g, device=DEV) * 0.7).to(dtype)      # 16 columns behind every row
    scale = torch.tensor([0.004, 0.02, 0.01, 0.05], device=DEV) if storage == "e4m3" else None
    cos, sin = _tables(dtype) if rotate else (None, None)
    raw, caches = _buffers(storage, dtype, padded)
    raw1, caches1 = _buffers(storage, dtype, padded)
    n_keys = _ints(counts)
    delta = _ints(deltas) if (deltas is not None and rotate) else None

    got = qkv.clone()
    _append(storage, True, got[:, :-16], caches, scale, cos, sin, n_keys, delta)
    want = qkv.clone()
    for b in range(B):
        _append(storage, False, want[b * R:(b + 1) * R, :-16], caches1[b], scale, cos, sin, n_keys[b:b + 1],
                None if delta is None else delta[b:b + 1])
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(got[:, (H + HKV) * D:].view(torch.int16), qkv[:, (H + HKV) * D:].view(torch.int16))       # V and the tail: untouched
    assert rotate != torch.equal(got[:, :H * D].view(torch.int16), qkv[:, :H * D].view(torch.int16))
    assert torch.equal(raw, raw1)                                     # every byte of the buffer, gaps and padding included

    # and the bytes that changed are exactly the R rows of every sequence, at its own position
    touched = torch.zeros_like(caches.view(torch.uint8), dtype=torch.bool)
    for b, n in enumerate(meant or counts):
        touched[b, n - R:n] = True
    mask = torch.zeros_like(raw, dtype=torch.bool)
    _mask_like(mask, storage, padded)[touched] = True
    assert bool((raw[~mask] == CANARY).all())
    rows = caches.view(torch.uint8)[touched]
    assert rows.numel() == B * R * 2 * HKV * D * (1 if storage == "e4m3" else 2)
    assert float((rows == CANARY).float().mean()) < 0.1               # the rows were written
    return raw


def _mask_like(mask, storage, padded):
    """the caches' view of a boolean buffer with one entry per byte: [B, T, 2 HKV, D x bytes per element]"""
    size = 1 if storage == "e4m3" else 2
    ld = (2 * HKV * D + (LD_PAD if padded else 0)) * size
    seq = (T + (GAP if padded else 0)) * ld
    return mask[:B * seq].view(B, seq)[:, :T * ld].unflatten(1, (T, ld))[:, :, :2 * HKV * D * size].unflatten(2, (2 * HKV, D * size))


def check_three_sequences_at_their_own_positions_and_offsets(padded, R, storage, dtype):
    _check(storage, dtype, R, padded, True, [7, 40, 19], [0, 5, -3])


def check_append_only_mode(R, storage):
    _check(storage, torch.float16, R, True, False, [7, 40, 19], None)


def check_no_offsets_at_all_and_the_offsets_matter(R, storage):
    a = _check(storage, torch.float16, R, True, True, [7, 40, 19], None)
    b = _check(storage, torch.float16, R, True, True, [7, 40, 19], [0, 5, -3])
    assert not torch.equal(a, b)


def check_both_clamps_hold_per_sequence(R, storage):
    """counts 0 and T + 9 are R and T for their sequence only; offsets that leave the tables clamp to its first and last row"""
    _check(storage, torch.float16, R, True, True, [0, T + 9, 19], [-1000, 1000, 2], meant=[R, T, 19])
    same = _check(storage, torch.float16, R, True, True, [R, T, 19], [-1000, 1000, 2])
    clamped = _check(storage, torch.float16, R, True, True, [0, T + 9, 19], [-1000, 1000, 2], meant=[R, T, 19])
    assert torch.equal(same, clamped)


def _sweep(check, **axes):
    """check(**case) for every combination of the axes; a failure names its case"""
    for values in itertools.product(*axes.values()):
        case = dict(zip(axes, values))
        try:
            check(**case)
        except AssertionError as e:
            raise AssertionError(f"{check.__name__} {case}: {e}") from e


def test_the_append_over_a_batch_of_caches():
    """every case of this file in one test: the cases are milliseconds each, and a failure names the check and its case"""
    _sweep(check_three_sequences_at_their_own_positions_and_offsets, padded=[False, True], R=[1, 3], storage=STORAGES, dtype=DTYPES)
    for check in (check_append_only_mode, check_no_offsets_at_all_and_the_offsets_matter, check_both_clamps_hold_per_sequence):
        _sweep(check, R=[1, 3], storage=STORAGES)
