"""The exactness argument of tests/gemv_exact_cases.py, checked on any machine for every shape the GPU tests launch: the operands
are integers inside their ranges and exact in the 16-bit dtype, the 2^24 precondition holds, and the expected logits from the int64
product equal a float64 product rounded to the dtype.  The list of shapes itself is checked too: it is what closes the gaps."""
import pytest
import torch

import gemv_exact_cases as exact

DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["fp16", "bf16"]


def test_the_shapes_reach_every_instantiation_and_both_lds_sizes():
    for N, K in [(1001, 1288), (9, 8), (9, 16)]:
        assert [M for (M, n, k) in exact.SHAPES if (n, k) == (N, K)] == list(range(1, 9))
    assert (5, 70001, 64) in exact.SHAPES
    assert {M * K * 2 for (M, N, K) in exact.SHAPES if K >= 4096} == {64 * 1024}           # x fills the 64 KiB the entry points allow
    assert all(K % 8 == 0 and 1 <= M <= 8 and M * K * 2 <= 64 * 1024 for (M, N, K) in exact.SHAPES)
    assert len(set(exact.SHAPES)) == len(exact.SHAPES)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", exact.SHAPES, ids=exact.shape_id)
def test_the_int64_product_is_the_float64_product_rounded_once(dtype, shape):
    M, N, K = shape
    xi, wi = exact.draw(M, N, K)
    assert int(xi.abs().max()) <= exact.X_MAX and int(wi.abs().max()) <= exact.W_MAX
    assert exact.X_MAX * exact.W_MAX * K < 2 ** 24
    x, w, logits, tokens = exact.case(dtype, M, N, K)
    assert x.dtype == dtype and w.dtype == dtype and logits.dtype == dtype and logits.shape == (M, N)
    assert torch.equal(x.long(), xi) and torch.equal(w.long(), wi)                          # the dtype holds the integers exactly
    want = (x.double() @ w.double().t()).to(dtype)
    assert exact.same_bits(logits, want)
    assert bool(torch.isfinite(logits.float()).all())
    # the tokens are the first maximum of the rounded values
    top = logits.float().max(dim=1, keepdim=True).values
    first = (logits.float() == top).int().argmax(dim=1)
    assert torch.equal(tokens, first)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", exact.MIRRORED, ids=exact.shape_id)
def test_in_the_mirrored_cases_every_maximum_is_a_tie(dtype, shape):
    M, N, K = shape
    x, w, logits, tokens = exact.case(dtype, M, N, K, mirrored=True)
    assert torch.equal(w[N // 2:2 * (N // 2)], w[:N // 2])
    assert exact.same_bits(logits, (x.double() @ w.double().t()).to(dtype))
    v = logits.float()
    assert bool(((v == v.max(dim=1, keepdim=True).values).sum(dim=1) >= 2).all())
    assert bool((tokens < N // 2).all())                                                    # the lower of the two indices
