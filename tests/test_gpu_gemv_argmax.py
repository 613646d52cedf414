"""``mq_gemv_f16_argmax`` (csrc/gemv_f16.hip; ops.gemv_f16_argmax) on the GPU: the lm_head product with the greedy token picked on
the device.  Two exact contracts, so every comparison is exact:

  * logits, when asked for, are the bits ``ops.gemv_f16`` writes for the same arguments;
  * token[m] is the argmax of THOSE 16-bit values as the CPU ``torch.argmax`` defines it (lowest index among equals, -0 == +0, a
    NaN is maximal and the first NaN wins): ``torch.argmax(ops.gemv_f16(x, w).cpu(), dim=1)`` is the checker of every test but
    one -- the integer-valued operands of tests/gemv_exact_cases.py have a checker that never calls the kernel (the int64 product
    of the CPU, rounded once), since a fault shared by the two instantiations of the one template is invisible to the first.

Rows of W go to waves four at a time, wave by wave, workgroup = four waves (rows [16 b, 16 b + 16) of pass 0 belong to workgroup b);
a matrix with more rows than the grid's waves x 4 takes further passes (70001 rows: three on a 256-CU chip).  The planted cases
put the winner where that hand-out can go wrong: the re-read last row, the ends of a group of four, another workgroup, another pass."""
import functools

import pytest
import torch

import gemv_exact_cases as exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.set_grad_enabled(False)
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]
SHAPES = [(1, 1, 8), (1, 3, 8), (3, 1001, 1288), (8, 4099, 4096), (2, 5, 3584), (1, 70001, 64)]      # (M, N, K)
MULTI_PASS = (1, 70001, 64)


@functools.lru_cache(maxsize=None)
def _case(dtype, M, N, K):
    """(x [M, K], w [N, K], gemv_f16's logits [M, N], the checker's tokens [M] on the CPU): made once per shape, never written to"""
    from mquant_amd import ops
    g = torch.Generator(device=DEV).manual_seed(7 * M + N + K)
    x = torch.randn((M, K), generator=g, device=DEV).to(dtype)
    w = (torch.randn((N, K), generator=g, device=DEV) * 0.02).to(dtype)
    ref = ops.gemv_f16(x, w)
    return x, w, ref, checker(ref)


def checker(logits):
    return torch.argmax(logits.cpu(), dim=1)


def check_tokens(x, w, **kw):
    """tokens of one call == the checker's on gemv_f16 of the same operands; returns them (CPU, int64)"""
    from mquant_amd import ops
    tok = ops.gemv_f16_argmax(x, w, **kw)
    assert tok.dtype == torch.int32 and tok.shape == (x.shape[0],)
    got, want = tok.cpu().long(), checker(ops.gemv_f16(x, w))
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    return got


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def rows_per_pass(N):
    """rows of W one pass of the grid hands out: workgroups x 4 waves x 4 rows (at M = 2 the workspace is 16 bytes per workgroup)"""
    from mquant_amd import ops
    return ops.gemv_argmax_workspace_bytes(2, N)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_random_data(dtype, M, N, K):
    from mquant_amd import ops
    x, w, ref, want = _case(dtype, M, N, K)
    poison = torch.full((M, N), 7.0, dtype=dtype, device=DEV)
    tok = ops.gemv_f16_argmax(x, w)                                   # logits=None: no logits reach memory
    assert tok.dtype == torch.int32 and tok.shape == (M,)
    print("tokens", tok.cpu().tolist(), "checker", want.tolist())
    assert torch.equal(tok.cpu().long(), want)
    assert bool((poison == 7.0).all())
    logits = torch.full((M, N), 7.0, dtype=dtype, device=DEV)
    tok2 = ops.gemv_f16_argmax(x, w, logits=logits)
    assert same_bits(logits, ref) and torch.equal(tok2.cpu().long(), want)
    assert bool((poison == 7.0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M", exact.EVERY_M, ids=lambda M: f"M{M}")
def test_integer_operands_against_a_checker_that_is_not_the_kernel(dtype, M):
    """Every M of the launch's switch, each at every shape tests/gemv_exact_cases.py lists for it (the mirrored ones, where every
    maximum is a tie, included), with operands whose fp32 sums are exact in any order: the logits are the int64 product of the CPU
    rounded once, the tokens ``torch.argmax`` of THOSE values -- ``gemv_f16`` is one of the three calls under test here, not the
    checker."""
    from mquant_amd import ops
    shapes = exact.cases_of(M)
    assert len(shapes) >= 3
    for _, N, K, mirrored in shapes:
        what = (N, K, mirrored)
        x, w, want, want_tok = exact.case(dtype, M, N, K, mirrored)
        x, w = x.to(DEV), w.to(DEV)
        ref = ops.gemv_f16(x, w, out=torch.full((M, N), float("nan"), dtype=dtype, device=DEV))
        assert exact.same_bits(ref, want), what
        tok = torch.full((M,), -77, dtype=torch.int32, device=DEV)          # a row the launch forgets stays -77
        ops.gemv_f16_argmax(x, w, token_out=tok)                            # logits=None
        print(what, "tokens", tok.cpu().tolist(), "checker", want_tok.tolist())
        assert torch.equal(tok.cpu().long(), want_tok), what
        tok2 = torch.full((M,), -77, dtype=torch.int32, device=DEV)
        logits = torch.full((M, N), float("nan"), dtype=dtype, device=DEV)
        ops.gemv_f16_argmax(x, w, logits=logits, token_out=tok2)
        assert same_bits(logits, ref) and exact.same_bits(logits, want), what
        assert torch.equal(tok2.cpu().long(), want_tok), what


def test_the_last_shape_takes_more_than_one_pass():
    assert rows_per_pass(MULTI_PASS[1]) < MULTI_PASS[1] // 2, "70001 rows were meant to take three passes of the grid"


def _planted(dtype, M, N_full, K, N, rows):
    """the first N rows of the cached W with x[0] written over `rows`: logit |x[0]|^2 ~ K at m = 0, far above the random ones"""
    x, w, _, _ = _case(dtype, M, N_full, K)
    w = w[:N].clone()
    for n in rows:
        w[n] = x[0]
    return x, w


PLANTS = [  # (M, N of the cached case, K, N used, planted row)
    (3, 1001, 1288, 1001, 0),
    (3, 1001, 1288, 1001, 1000),           # N - 1 with N % 4 = 1: the last group re-reads it three times
    (3, 1001, 1288, 998, 997),             # N % 4 = 2
    (3, 1001, 1288, 999, 998),             # N % 4 = 3
    (3, 1001, 1288, 999, 996),             # the first row of that last, partial group
    (8, 4099, 4096, 4099, 4098),
    (2, 5, 3584, 5, 4),
    (1, 3, 8, 3, 2),
    (3, 1001, 1288, 1001, 500),            # first and last row of a wave's group of four
    (3, 1001, 1288, 1001, 503),
    (1, 70001, 64, 70001, 40000),          # a row of the second pass
    (1, 70001, 64, 70001, 69998),          # ... of the third
    (1, 70001, 64, 70001, 70000),          # ... and its re-read last row
]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,NF,K,N,row", PLANTS, ids=[f"{p[3]}x{p[2]}-row{p[4]}" for p in PLANTS])
def test_planted_maximum(dtype, M, NF, K, N, row):
    x, w = _planted(dtype, M, NF, K, N, [row])
    got = check_tokens(x, w)
    assert int(got[0]) == row and bool((got < N).all())


TIES = [  # (M, N, K, the two planted rows): the lower index wins
    (3, 1001, 1288, (500, 502)),           # the same group of four
    (3, 1001, 1288, (501, 503)),
    (3, 1001, 1288, (17, 900)),            # different workgroups
    (3, 1001, 1288, (998, 1000)),          # ... the higher one being the re-read last row
    (1, 70001, 64, (100, 100 + 32768)),    # different passes (the same wave on a 256-CU chip)
    (1, 70001, 64, (33000, 69000)),
    (1, 70001, 64, (40001, 5)),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,N,K,rows", TIES, ids=[f"{t[1]}-rows{t[3][0]}-{t[3][1]}" for t in TIES])
def test_ties_go_to_the_lowest_index(dtype, M, N, K, rows):
    from mquant_amd import ops
    x, w = _planted(dtype, M, N, K, N, rows)
    ref = ops.gemv_f16(x, w)
    assert same_bits(ref[:, rows[0]], ref[:, rows[1]])                # bit-identical rows of W: bit-identical logits
    got = check_tokens(x, w)
    assert int(got[0]) == min(rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,N,K", [(3, 1001, 1288), (1, 70001, 64), (1, 3, 8)])
def test_all_logits_zero_give_token_zero(dtype, M, N, K):
    x, w, _, _ = _case(dtype, M, N, K)
    got = check_tokens(torch.zeros_like(x), w)
    assert got.tolist() == [0] * M


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,N,K,nans,inf", [(3, 1001, 1288, (700, 333), 20), (3, 1001, 1288, (334, 1000), 999),
                                             (1, 70001, 64, (69999, 40000), 39999), (1, 70001, 64, (6, 50000), 3)])
def test_the_first_nan_wins_and_beats_infinity(dtype, M, N, K, nans, inf):
    from mquant_amd import ops
    x, w, _, _ = _case(dtype, M, N, K)
    x, w = x.clone(), w.clone()
    x[:, 0] = 1.0
    w[inf, 0] = float("inf")
    for n in nans:
        w[n, 0] = float("nan")
    ref = ops.gemv_f16(x, w)
    assert bool(torch.isnan(ref[:, list(nans)]).all()) and bool((ref[:, inf] == float("inf")).all())
    got = check_tokens(x, w)
    assert got.tolist() == [min(nans)] * M


# ---- exact properties
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,N,K", [(3, 1001, 1288), (8, 4099, 4096), (1, 70001, 64)])
def test_workspace_contents_do_not_matter_and_its_tail_is_untouched(dtype, M, N, K):
    from mquant_amd import ops
    x, w, _, want = _case(dtype, M, N, K)
    need = ops.gemv_argmax_workspace_bytes(M, N)
    assert need > 0 and need % 16 == 0
    for fill in (0xFF, 0x00):
        ws = torch.full((need + 256,), fill, dtype=torch.uint8, device=DEV)
        tok = ops.gemv_f16_argmax(x, w, workspace=ws)
        assert torch.equal(tok.cpu().long(), want), fill
        assert bool((ws[need:] == fill).all())
    with pytest.raises(Exception, match="the workspace needs"):
        ops.gemv_f16_argmax(x, w, workspace=ws[:need - 16])


@pytest.mark.parametrize("M,N,K", [(3, 1001, 1288), (8, 4099, 4096), (1, 1, 8)])
def test_token_out_inside_a_larger_buffer(M, N, K):
    from mquant_amd import ops
    x, w, _, want = _case(torch.float16, M, N, K)
    buf = torch.full((M + 2,), -77, dtype=torch.int32, device=DEV)
    tok = ops.gemv_f16_argmax(x, w, token_out=buf[1:M + 1])
    assert tok.data_ptr() == buf[1:].data_ptr()
    assert buf.cpu().tolist() == [-77] + want.tolist() + [-77]


def test_strided_operands_and_logits_buffer():
    """the operands of test_gpu_gemv.py::test_strided_operands_and_out_buffer"""
    from mquant_amd import ops
    g = torch.Generator(device=DEV).manual_seed(1)
    xw = torch.randn((2, 2 * 512), generator=g, device=DEV).half()
    ww = (torch.randn((300, 3 * 512), generator=g, device=DEV) * 0.05).half()
    x, w = xw[:, :512], ww[:, 512:1024]                         # row strides larger than K
    ref = torch.full((2, 1024), 7.0, dtype=torch.float16, device=DEV)
    ops.gemv_f16(x, w, out=ref[:, 100:400])
    out = torch.full((2, 1024), 7.0, dtype=torch.float16, device=DEV)
    tok = ops.gemv_f16_argmax(x, w, logits=out[:, 100:400])
    assert same_bits(out, ref)                                   # the logits and the 7.0 around them
    assert torch.equal(tok.cpu().long(), checker(ref[:, 100:400]))
    assert torch.equal(ops.gemv_f16_argmax(x, w).cpu(), tok.cpu())


def test_a_captured_graph_follows_x():
    from mquant_amd import ops
    M, N, K = 3, 1001, 1288
    x, w, _, want = _case(torch.float16, M, N, K)
    xb = x.clone()
    tok = torch.zeros((M,), dtype=torch.int32, device=DEV)
    ops.gemv_f16_argmax(xb, w, token_out=tok)                         # warm-up: the wrapper's workspace
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gemv_f16_argmax(xb, w, token_out=tok)
    seen = []
    for rows in ((123, 777, 1000), (5, 0, 640)):
        x_new = (w[list(rows)].float() * 50.0).half()                 # row m points along W[rows[m]]
        xb.copy_(x_new)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(tok.cpu().long(), checker(ops.gemv_f16(x_new, w)))
        seen.append(tok.cpu().tolist())
    assert seen[0] != seen[1] and seen[0] != want.tolist()
    xb.copy_(x)
    graph.replay()
    assert torch.equal(tok.cpu().long(), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_the_same_call_twice_gives_the_same_bits(dtype):
    from mquant_amd import ops
    M, N, K = 8, 4099, 4096
    x, w, ref, _ = _case(dtype, M, N, K)
    outs = []
    for _ in range(2):
        logits = torch.empty((M, N), dtype=dtype, device=DEV)
        outs.append((ops.gemv_f16_argmax(x, w, logits=logits).cpu(), logits))
    assert torch.equal(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]) and same_bits(outs[0][1], ref)


def test_no_rows_and_no_columns():
    from mquant_amd import ops
    from mquant_amd._lib import MQuantHipError
    x = torch.zeros((2, 64), dtype=torch.float16, device=DEV)
    w = torch.zeros((16, 64), dtype=torch.float16, device=DEV)
    assert ops.gemv_f16_argmax(x[:0], w).shape == (0,)
    with pytest.raises(MQuantHipError, match="an argmax over nothing"):
        ops.gemv_f16_argmax(x, w[:0])
