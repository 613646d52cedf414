"""Integer-valued operands for ``gemv_f16`` / ``gemv_f16_argmax``, as plain data and CPU arithmetic: the cases of
tests/test_gpu_gemv.py, tests/test_gpu_gemv_argmax.py and tests/test_gpu_wide_strides.py that compare BITS with a checker which is
not the kernel, and tests/test_gemv_exact_cases_cpu.py, which shows on any machine that the argument below holds for every shape.

x holds integers in [-2, 2], W integers in [-3, 3]: exact in fp16 and bf16.  With max|x| * max|w| * K < 2^24 every product and
every partial sum is an integer of magnitude below 2^24, which fp32 holds exactly -- the kernel's fp32 accumulator is then exact in
ANY summation order (lanes, butterfly, fdot2 or fma), and the one rounding left is the store to the 16-bit dtype.  The expected
logits are therefore the int64 product, converted to float32 (exact) and then to the dtype (round to nearest even); the expected
tokens are ``torch.argmax`` of those 16-bit values on the CPU: a checker that never calls the kernel.  Integer data repeats its
logits, and where the largest one is repeated the lowest-index rule decides the token (MIRRORED makes that every row)."""
import functools

import torch

X_MAX, W_MAX = 2, 3
EVERY_M = range(1, 9)               # the eight instantiations behind gemv_launch's switch
SHAPES = (
    # N % 4 = 1: the last row is re-read; 161 chunks of 16 bytes: lanes 0 .. 32 take a third step
    [(M, 1001, 1288) for M in EVERY_M]
    # K = 8: x (16 M bytes) is smaller than the argmax's key slots (32 M bytes), the launch raises the LDS to them; K = 16: the
    # two sizes are equal.  Nine rows: three of the workgroup's four waves own rows
    + [(M, 9, K) for K in (8, 16) for M in EVERY_M]
    + [(8, 9, 4096), (1, 9, 32768)]     # x is exactly 64 KiB
    + [(5, 70001, 64)]                  # several passes of the grid
)
# Ties at the maximum are rarer than ties in general (the winning value sits in the sparse tail), so two more cases make every
# maximum a tie: rows [N // 2, 2 (N // 2)) of W repeat rows [0, N // 2), each logit occurs at n and at n + N // 2 -- in another
# workgroup, for 70001 rows in another pass of the grid -- and the lower index must win.
MIRRORED = [(4, 1001, 1288), (6, 70001, 64)]


def cases_of(M, mirrored=True):
    """the (M, N, K, mirrored) cases of one instantiation, in one list: a GPU test per M and dtype runs them all"""
    return [s + (False,) for s in SHAPES if s[0] == M] + ([s + (True,) for s in MIRRORED if s[0] == M] if mirrored else [])


def shape_id(s):
    return "M%d-N%d-K%d" % s


def draw(M, N, K, seed=None):
    """(x [M, K], w [N, K]) int64 on the CPU from a seeded generator"""
    g = torch.Generator().manual_seed(M + 10 * N + 1000 * K if seed is None else seed)
    x = torch.randint(-X_MAX, X_MAX + 1, (M, K), generator=g, dtype=torch.int64)
    w = torch.randint(-W_MAX, W_MAX + 1, (N, K), generator=g, dtype=torch.int64)
    return x, w


def expected(x, w, dtype):
    """(logits [M, N] of `dtype`, tokens [M] int64) for integer x, w (int64, CPU); asserts the precondition of the argument above"""
    assert x.dtype == torch.int64 and w.dtype == torch.int64 and not x.is_cuda and not w.is_cuda
    K = x.shape[1]
    assert int(x.abs().max()) * int(w.abs().max()) * K < 2 ** 24, (int(x.abs().max()), int(w.abs().max()), K)
    exact = x @ w.t()
    assert int(exact.abs().max()) < 2 ** 24
    logits = exact.to(torch.float32).to(dtype)
    return logits, torch.argmax(logits, dim=1)


@functools.lru_cache(maxsize=None)
def case(dtype, M, N, K, mirrored=False):
    """(x, w of `dtype`, expected logits, expected tokens), all on the CPU; made once per shape, never written to"""
    x, w = draw(M, N, K)
    if mirrored:
        w[N // 2:2 * (N // 2)] = w[:N // 2].clone()
    logits, tokens = expected(x, w, dtype)
    return x.to(dtype), w.to(dtype), logits, tokens


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))
