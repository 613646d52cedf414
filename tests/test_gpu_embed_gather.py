"""``mq_embed_gather`` (csrc/embed.hip; ops.embed_gather) on the GPU: rows of a 16-bit embedding table at ids read on the device, and
the id log a captured generation loop leaves for the host.  Bit copies and integers: every comparison is exact and looks at WHOLE
buffers -- the poison behind ``dim`` in a strided ``out`` and every log entry the call must not write included."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
TABLES = [(1001, 1288), (37, 8)]            # (vocab, dim): 161 chunks of 16 bytes (one workgroup, partly idle) and a single chunk
# rows wider than one workgroup's 256 chunks (dim > 2048): 2056 = 257 chunks, the second workgroup has ONE live lane; 3584 (the 7B
# model dim) = 448, the second is partly idle; 4096 = exactly two full workgroups; 8200 = 1025, five workgroups, the last with one lane
WIDE_DIMS = [2056, 3584, 4096, 8200]
LOG_ROWS = 40
POISON_ID = -77


@functools.lru_cache(maxsize=None)
def _table(dtype, vocab, dim):
    """a table in a wider buffer (row stride dim + 8), distinct rows; never written to"""
    g = torch.Generator(device=DEV).manual_seed(vocab + dim)
    wide = torch.randn((vocab, dim + 8), generator=g, device=DEV).to(dtype)
    return wide[:, :dim]


def bits(t):
    return t.contiguous().view(torch.int16)


def gather(table, ids, n_keys="none", log=True):
    """one call into a poisoned, strided out and a poisoned log -> (out buffer [R, dim + 8], log or None)"""
    from mquant_amd import ops
    R, dim = len(ids), table.shape[1]
    ids_dev = torch.tensor(ids, dtype=torch.int32, device=DEV)
    wide = torch.full((R, dim + 8), 7.0, dtype=table.dtype, device=DEV)
    id_log = torch.full((LOG_ROWS,), POISON_ID, dtype=torch.int32, device=DEV) if log else None
    nk = None if n_keys == "none" else torch.tensor([n_keys], dtype=torch.int32, device=DEV)
    out = ops.embed_gather(table, ids_dev, out=wide[:, :dim], id_log=id_log, n_keys=nk)
    assert out.data_ptr() == wide.data_ptr()
    assert ids_dev.cpu().tolist() == list(ids) and (nk is None or int(nk.item()) == n_keys)     # read, never written
    return wide, id_log


def check(table, ids, wide, id_log, n):
    """rows are bit copies of the clamped ids' rows, the poison behind dim is intact, the log holds the clamped ids at [n - R, n)"""
    vocab, dim = table.shape
    R = len(ids)
    clamped = [min(max(i, 0), vocab - 1) for i in ids]
    assert torch.equal(bits(wide[:, :dim]), bits(table[clamped]))
    assert bool((wide[:, dim:] == 7.0).all())
    if id_log is not None:
        want = [POISON_ID] * LOG_ROWS
        want[n - R:n] = clamped
        assert id_log.cpu().tolist() == want


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("vocab,dim", TABLES)
@pytest.mark.parametrize("R", [1, 3, 8])
def test_rows_are_bit_copies(dtype, vocab, dim, R):
    table = _table(dtype, vocab, dim)
    ids = [(vocab - 1) * r // max(R - 1, 1) for r in range(R)] if R > 1 else [vocab // 3]       # first and last row included
    ids = ids[::-1]
    wide, id_log = gather(table, ids, n_keys=20)
    check(table, ids, wide, id_log, 20)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("dim", WIDE_DIMS)
def test_rows_wider_than_one_workgroup(dtype, dim):
    """blockIdx.x >= 1, for R = 1, 3 and 8: every chunk of the row arrives, the poison behind dim survives, and the log still
    gets ONE entry per row"""
    vocab = 37
    table = _table(dtype, vocab, dim)
    for R in (1, 3, 8):
        ids = [(vocab - 1) * r // max(R - 1, 1) for r in range(R)] if R > 1 else [vocab // 3]
        ids = ids[::-1]
        wide, id_log = gather(table, ids, n_keys=20)
        check(table, ids, wide, id_log, 20)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("vocab,dim", TABLES)
def test_ids_outside_the_table_are_clamped(dtype, vocab, dim):
    table = _table(dtype, vocab, dim)
    ids = [-5, vocab + 9, 3, -(1 << 31), (1 << 31) - 1]
    wide, id_log = gather(table, ids, n_keys=11)
    check(table, ids, wide, id_log, 11)
    assert id_log[6:11].cpu().tolist() == [0, vocab - 1, 3, 0, vocab - 1]


@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("n_dev,acts_as", [(20, 20), (LOG_ROWS, LOG_ROWS), ("R", "R"), (0, "R"), (-7, "R"), (1000, LOG_ROWS),
                                           ((1 << 31) - 1, LOG_ROWS)])
def test_log_position_from_the_device_count(R, n_dev, acts_as):
    """n = clamp(*n_keys, R, log_rows): inside the range, at both ends, below R and above log_rows"""
    table = _table(torch.float16, 1001, 1288)
    n_dev, n = (R if n_dev == "R" else n_dev), (R if acts_as == "R" else acts_as)
    ids = [100 + 7 * r for r in range(R)]
    wide, id_log = gather(table, ids, n_keys=n_dev)
    check(table, ids, wide, id_log, n)


@pytest.mark.parametrize("R", [1, 3, 8])
def test_without_a_count_the_log_ends_at_log_rows(R):
    table = _table(torch.bfloat16, 37, 8)
    ids = [36 - r for r in range(R)]
    wide, id_log = gather(table, ids)
    check(table, ids, wide, id_log, LOG_ROWS)


def test_without_a_log_nothing_is_logged():
    table = _table(torch.float16, 1001, 1288)
    bystander = torch.full((LOG_ROWS,), POISON_ID, dtype=torch.int32, device=DEV)
    wide, id_log = gather(table, [5, 900, 17], n_keys=20, log=False)
    check(table, [5, 900, 17], wide, None, 20)
    assert id_log is None and bool((bystander == POISON_ID).all())


def test_default_out_and_bad_arguments():
    from mquant_amd import ops
    from mquant_amd._lib import MQuantHipError
    table = _table(torch.float16, 1001, 1288)
    ids = torch.tensor([1000, 0], dtype=torch.int32, device=DEV)
    out = ops.embed_gather(table, ids)
    assert out.shape == (2, 1288) and torch.equal(bits(out), bits(table[[1000, 0]]))
    with pytest.raises(MQuantHipError, match="R = 9 rows"):
        ops.embed_gather(table, torch.zeros((9,), dtype=torch.int32, device=DEV))
    with pytest.raises(MQuantHipError, match="log_rows = 1 entries for R = 2 rows"):
        ops.embed_gather(table, ids, id_log=torch.zeros((1,), dtype=torch.int32, device=DEV))
