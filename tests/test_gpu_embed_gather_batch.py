"""The batched embedding gather (mq_embed_gather_batch; csrc/embed.hip) on the GPU: B sequences of one new row each -- the rows
are the table rows, sequence b's id is logged in its own log at its own position and nowhere else, ids and positions are clamped."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
VOCAB, LOG_ROWS = 37, 12


def bits(t):
    return t.contiguous().view(torch.int16)


def _ints(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def check_rows_and_log_entries_of_a_batch(B, dim, dtype):
    from mquant_amd import ops
    g = torch.Generator(device=DEV).manual_seed(dim + B)
    table = torch.randn((VOCAB, dim), generator=g, device=DEV).to(dtype)
    ids = [36, 0, 17, 5, 30, 1, 22, 9][:B]
    counts = [1, 12, 5, 7, 2, 11, 3, 8][:B]
    wide = torch.full((B + 2, dim + 8), 7.0, dtype=dtype, device=DEV)
    logs = torch.full((B, LOG_ROWS + 4), -77, dtype=torch.int32, device=DEV)          # four entries of padding behind every log
    out = ops.embed_gather_batch(table, _ints(ids), out=wide[1:B + 1, :dim], id_log=logs[:, :LOG_ROWS], n_keys=_ints(counts))
    assert torch.equal(bits(out), bits(table[ids]))
    assert bool((wide[0] == 7.0).all()) and bool((wide[B + 1] == 7.0).all()) and bool((wide[:, dim:] == 7.0).all())
    want = torch.full((B, LOG_ROWS + 4), -77, dtype=torch.int32)
    for b in range(B):
        want[b, counts[b] - 1] = ids[b]
    assert torch.equal(logs.cpu(), want)
    # without a log, and with a fresh output
    assert torch.equal(bits(ops.embed_gather_batch(table, _ints(ids))), bits(table[ids]))


def check_ids_and_positions_are_clamped_per_sequence():
    from mquant_amd import ops
    dim, B = 512, 4
    table = torch.randn((VOCAB, dim), device=DEV).half()
    ids, rows = [-5, VOCAB, 2 ** 31 - 1, 7], [0, VOCAB - 1, VOCAB - 1, 7]
    counts, at = [0, LOG_ROWS + 9, -3, 4], [0, LOG_ROWS - 1, 0, 3]
    logs = torch.full((B, LOG_ROWS), -77, dtype=torch.int32, device=DEV)
    out = ops.embed_gather_batch(table, _ints(ids), id_log=logs, n_keys=_ints(counts))
    assert torch.equal(bits(out), bits(table[rows]))
    want = torch.full((B, LOG_ROWS), -77, dtype=torch.int32)
    for b in range(B):
        want[b, at[b]] = rows[b]
    assert torch.equal(logs.cpu(), want)
    # no key counts: every sequence logs at its last entry
    logs.fill_(-77)
    ops.embed_gather_batch(table, _ints(ids), id_log=logs)
    want.fill_(-77)
    want[:, LOG_ROWS - 1] = torch.tensor(rows, dtype=torch.int32)
    assert torch.equal(logs.cpu(), want)


def check_one_sequence_is_the_single_sequence_call():
    from mquant_amd import ops
    dim = 512
    table = torch.randn((VOCAB, dim), device=DEV).half()
    a_log = torch.full((1, LOG_ROWS), -77, dtype=torch.int32, device=DEV)
    b_log = torch.full((LOG_ROWS,), -77, dtype=torch.int32, device=DEV)
    a = ops.embed_gather_batch(table, _ints([19]), id_log=a_log, n_keys=_ints([6]))
    b = ops.embed_gather(table, _ints([19]), id_log=b_log, n_keys=_ints([6]))
    assert torch.equal(bits(a), bits(b)) and torch.equal(a_log[0], b_log) and b_log.cpu().tolist().count(-77) == LOG_ROWS - 1


def _sweep(check, **axes):
    """check(**case) for every combination of the axes; a failure names its case"""
    for values in itertools.product(*axes.values()):
        case = dict(zip(axes, values))
        try:
            check(**case)
        except AssertionError as e:
            raise AssertionError(f"{check.__name__} {case}: {e}") from e


def test_the_embedding_gather_for_a_batch_of_sequences():
    """every case of this file in one test: the cases are milliseconds each, and a failure names the check and its case"""
    # dim 512: 64 chunks, part of one workgroup; 8200: 1025 chunks, five workgroups, the last one ragged
    _sweep(check_rows_and_log_entries_of_a_batch, B=[1, 3, 8], dim=[512, 8200], dtype=[torch.float16, torch.bfloat16])
    check_ids_and_positions_are_clamped_per_sequence()
    check_one_sequence_is_the_single_sequence_call()
