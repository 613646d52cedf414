"""The case list of the Hadamard sweep (hadamard_cases.py) against the launch plan (csrc/hadamard.hip make_had_plan, queried through
mq_hadamard_debug_plan: host arithmetic, no device -- the CU count falls back to 256): the cases reach exactly the path keys the
plan can return over the accepted domain, the refusals come back through the query with the launch's codes and messages, the
oracle is fit to judge the shape classes no test held before, and the tie inputs of the GPU sweep are what they claim."""
import ctypes as C

import numpy as np
import pytest

import hadamard_cases as hc
import oracle

MQ_EINVAL, MQ_EUNSUPPORTED = -1, -2


def last_error():
    from mquant_amd import _lib
    L = _lib.load()
    L.mq_last_error.restype = C.c_char_p
    return L.mq_last_error().decode()


@pytest.fixture(scope="module")
def domain():
    """Path keys over a grid of the API's accepted domain, enumerated here (not taken from the case list's own walk): K of the
    table and 1, m = 2^0 .. 2^15, the M ladder, dtypes, fp32_had, plain / quantizing, both activations, words / descriptor, both
    layouts, aligned / unaligned x / a row stride of 2 mod 4, the thread hook."""
    L = hc.lib()
    keep = [hc.PLAN_FIELDS.index(f) for f in hc.KEY_FIELDS]
    buf = (C.c_int * len(hc.PLAN_FIELDS))()
    keys, refused = set(), 0
    Ms = hc.m_ladder(hc.cu_count())
    try:
        for hook in (0, 256, 512):
            L.mq_hadamard_debug_threads(hook)
            for K in (1,) + hc.TABLE_K:
                for p in range(16):
                    n = K << p
                    for dt in (0, 1, 2):
                        for fl in (0, 1, 2, 3):
                            for quant, act, tiled in ((0, 0, 0), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (1, 2, 0), (1, 2, 1)):
                                for aligned in (7, 6, 3):
                                    for M in Ms:
                                        if L.mq_hadamard_debug_plan(M, n, n, K, dt, fl, quant, act, tiled, aligned, buf) == 0:
                                            keys.add(tuple(buf[i] for i in keep))
                                        else:
                                            refused += 1
    finally:
        L.mq_hadamard_debug_threads(0)
    assert refused > 0
    return keys


@pytest.fixture(scope="module")
def case_keys():
    out = {}
    for c in hc.cases():
        out.setdefault(hc.key(c), []).append(c.name)
    return out


def test_the_cases_reach_every_path_the_plan_can_return(domain, case_keys):
    assert set(case_keys) == domain, (sorted(domain - set(case_keys))[:5], sorted(set(case_keys) - domain)[:5])
    names = dict(zip(hc.KEY_FIELDS, zip(*domain)))
    assert set(names["butterfly"]) == {0, 1, 2, 3} and set(names["kxk"]) == {0, 1, 2, 3, 4, 5}
    assert set(names["threads"]) == {256, 512} and set(names["unit"]) == {0, 3, 5} and set(names["parts_log2"]) == {0, 1, 2, 3}
    assert set(names["fast_first"]) == {0}           # the fast dispatcher (hadamard_fast.hip) is not part of this sweep


def test_dropping_the_cases_of_one_path_is_noticed(domain, case_keys):
    """The check above is not vacuous: without the cases the plan sends down one path the set is incomplete."""
    for target in domain:
        kept = {k for k in case_keys if k != target}
        assert kept != domain, target
    assert all(case_keys[k] for k in domain)


def test_the_hand_placed_sections_cover_the_switches_by_themselves():
    """Both sides of every switch are placed by hand (the fill only adds combinations of them): every butterfly class x {K = 1,
    K > 1} that fits the LDS, every K x K class at 256 and 512 threads, each parts_log2 value, the row map, each staging width."""
    sec = [hc.plan(c) for c in hc.sections(hc.cu_count())]
    bf = {(p["butterfly"], c.K > 1) for p, c in zip(sec, hc.sections(hc.cu_count()))}
    assert bf == {(0, False), (0, True), (1, False), (1, True), (2, False), (2, True), (3, False)}
    assert {(p["kxk"], p["threads"]) for p in sec} >= {(k, t) for k in (0, 2, 4, 5) for t in (256, 512)} | {(1, 256), (3, 512)}
    assert {p["parts_log2"] for p in sec} == {0, 1, 2, 3} and {p["remap"] for p in sec} == {0, 1}
    assert {(p["unit"], p["act"]) for p in sec} == {(u, a) for u in (0, 3, 5) for a in (0, 1)}
    assert {(p["x_vec"], p["q_vec"]) for p in sec if p["unit"]} >= {(1, 1), (0, 1), (1, 0)}
    shapes = {(c.n, c.K) for c in hc.sections(hc.cu_count())}
    assert {(1664, 52), (27648, 108), (1024, 1), (2048, 1), (4096, 1), (8192, 1), (12288, 12), (24576, 12)} <= shapes
    # register pass: R = 2, 4, 8, 16
    assert {c.n // c.K >> 9 for c in hc.sections(hc.cu_count()) if 512 < c.n // c.K <= 8192} == {2, 4, 8, 16}


def test_rows_on_both_sides_of_every_short_batch_step():
    """parts_log2 steps where M << (parts + 1) crosses the CU count; the ladder has the row count on either side."""
    cus = hc.cu_count()
    for n_in, n, K in hc.UNITS:
        for j in (1, 2, 3):
            a, b = (hc.query(M, n_in, n, K, "f16", hc.HAD_PREPARED, True, 0, False, 7)[1]["parts_log2"] for M in (cus >> j, (cus >> j) + 1))
            assert a >= b and {cus >> j, (cus >> j) + 1} <= set(hc.m_ladder(cus))
    p = [hc.query(M, 18944, 19968, 156, "f16", hc.HAD_PREPARED, True, 0, False, 7)[1]["parts_log2"] for M in hc.m_ladder(cus)]
    assert set(p) == {0, 1, 2, 3}
    assert [hc.query(M, 5120, 5120, 40, "f16", hc.HAD_PREPARED, True, 0, True, 7)[1]["remap"] for M in (127, 128)] == [0, 1]


REFUSALS = [
    # (M, n_in, n, K, dtype, flags, quant, act, tiled, aligned), code, message part
    ((3, 100, 100, 12, "f16", 0, False, 0, False, 7), MQ_EINVAL, "K=12 does not divide n=100"),
    ((3, 240, 240, 20, "f16", 0, False, 0, False, 7), MQ_EINVAL, "n/K=12 is not a power of two"),
    ((3, 96, 96, 6, "f16", 0, False, 0, False, 7), MQ_EINVAL, "K=6 needs 4-byte aligned had_words and K % 4 == 0"),
    ((3, 40960, 40960, 40, "f32", 0, False, 0, False, 7), MQ_EUNSUPPORTED, "n=40960 needs 164160 B of LDS (> 160 KiB)"),
    ((3, 65536, 65536, 1, "f16", 0, True, 0, True, 7), MQ_EUNSUPPORTED, "needs 262144 B of LDS"),
    ((3, 49152, 49152, 12, "f16", 1, True, 0, False, 7), MQ_EUNSUPPORTED, "(> 160 KiB)"),
    ((3, 0, 64, 1, "f16", 0, False, 0, False, 7), MQ_EINVAL, "bad shape (n_in=0, n=64)"),
    ((3, 65, 64, 1, "f16", 0, False, 0, False, 7), MQ_EINVAL, "bad shape"),
    ((3, 80, 80, 20, "f16", 0, True, 1, False, 7), MQ_EINVAL, "mq_act_hadamard_quant_i8: n/K must be >= 8"),
    # the mask-driven units store two levels at a time: an odd row stride of a row-major destination is refused ...
    ((3, 5120, 5120, 40, "f16", hc.HAD_PREPARED, True, 0, False, 1), MQ_EINVAL, "3 x 2 units need an even row stride"),
    ((3, 18944, 19968, 156, "f16", hc.HAD_PREPARED, True, 0, False, 0), MQ_EINVAL, "5 x 2 units need an even row stride"),
]


@pytest.mark.parametrize("args,code,part", REFUSALS, ids=[r[2] for r in REFUSALS])
def test_refusals_come_back_through_the_query(args, code, part):
    rc, _ = hc.query(*args)
    assert rc == code and part in last_error(), (rc, last_error())


def test_what_the_odd_stride_refusal_leaves_alone():
    """... while the same destination is accepted with plain sign words (classic path, byte stores), in the tiled layout, at a
    forced thread count that leaves the units, and for the plain transform; a stride of 2 mod 4 keeps the units."""
    sh = (3, 5120, 5120, 40, "f16")
    assert hc.query(*sh, 0, True, 0, False, 1)[1]["q_vec"] == 0
    assert hc.query(*sh, hc.HAD_PREPARED, True, 0, True, 1)[0] == 0
    assert hc.query(*sh, hc.HAD_PREPARED, True, 0, False, 1, threads=512)[1]["unit"] == 0
    assert hc.query(*sh, hc.HAD_PREPARED, False, 0, False, 1)[1]["unit"] == 3
    rc, p = hc.query(*sh, hc.HAD_PREPARED, True, 0, False, 3)
    assert rc == 0 and p["unit"] == 3 and p["q_vec"] == 0


def test_an_empty_batch_plans_nothing():
    rc, p = hc.query(0, 100, 100, 7, "f16", 0, False, 0, False, 7)
    assert rc == 0 and not any(p.values())


def test_the_hook_is_the_calling_threads_and_is_reset():
    assert hc.query(3, 18944, 19968, 156, "f16", hc.HAD_PREPARED, True, 0, False, 7, threads=256)[1]["unit"] == 0
    assert hc.query(3, 18944, 19968, 156, "f16", hc.HAD_PREPARED, True, 0, False, 7)[1]["unit"] == 5


# ------------------------------------------------------------------------------------------------ the oracle on the new classes
def sylvester(m):
    h = np.ones((1, 1))
    while h.shape[0] < m:
        h = np.block([[h, h], [h, -h]])
    return h


def dense_f64(x, n, K, hk):
    """(H_K (x) H_m) [x; 0] / sqrt(n) in float64, H_m = H_a (x) H_b applied as dense factors."""
    m = n // K
    a = 1 << (m.bit_length() - 1) // 2
    b = m // a
    v = np.zeros(n)
    v[: x.size] = x
    v = v.reshape(K, a, b)
    v = np.einsum("pa,kab->kpb", sylvester(a), v)
    v = np.einsum("qb,kpb->kpq", sylvester(b), v)
    if K > 1:
        v = np.einsum("jk,kpq->jpq", hk.astype(np.float64), v)
    return v.reshape(n) / np.sqrt(np.float64(n))


@pytest.mark.parametrize("n_in,n,K", [(20, 20, 20), (40, 40, 20), (70, 80, 20), (96, 96, 12), (160, 160, 20), (448, 448, 28),
                                      (640, 640, 20), (1, 1, 1), (2, 2, 1), (4, 4, 1), (1024, 1024, 1), (2048, 2048, 1),
                                      (12288, 12288, 12), (20000, 20480, 20), (16384, 16384, 1), (32768, 32768, 1),
                                      (28672, 28672, 28), (36864, 36864, 36)])
def test_the_oracle_is_fit_to_judge_the_new_shape_classes(had_table, n_in, n, K):
    """oracle.hadamard in plain fp32 against the float64 dense product.  The bound is derived: every output is a chain of
    log2(m) + K + 1 fp32 operations (butterflies, scale, K signed additions) on terms whose magnitudes sum to at most sum_k |x_k|,
    so its error is at most (log2 m + K + 1) * 2^-24 * sum_k |x_k| / sqrt(n)."""
    from golden_inputs import make_x
    x = make_x(n + K, (2, n_in))
    hk = had_table["mats"].get(K)
    got = oracle.hadamard(x, n, K, hk, mid_round=0, out_round=0)
    m = n // K
    for r in range(2):
        want = dense_f64(x[r].astype(np.float64), n, K, hk)
        bound = (np.log2(m) + K + 1) * 2.0 ** -24 * np.abs(x[r].astype(np.float64)).sum() / np.sqrt(n)
        err = np.abs(got[r].astype(np.float64) - want).max()
        print(f"n={n} K={K}: max error {err:.3e}, bound {bound:.3e}, largest output {np.abs(want).max():.3e}")
        assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------ the tie inputs
TIES = [(sh, dtype, s) for sh in hc.TIE_SHAPES
        for dtype, ss in (("f32", hc.TIE_SCALES_F32), ("f16", hc.TIE_SCALES_16), ("bf16", hc.TIE_SCALES_16)) for s in ss]


@pytest.mark.parametrize("shape,dtype,s", TIES, ids=[f"{sh[1]}x{sh[2]}|{dt}|s{s:g}" for sh, dt, s in TIES])
def test_the_tie_inputs_are_what_they_claim(had_table, shape, dtype, s):
    """With the oracle alone: every element of a one-hot row rotates to the same magnitude; at least half of the probed elements
    are exact ties; for fp32 inputs (scales that are no powers of two) at least a tenth are quotient / reciprocal disagreements
    and both clamps are met.  (With a power-of-two scale the reciprocal is exact: the 16-bit sets hold ties only.)"""
    n_in, n, K, _ = shape
    x, n_ties = hc.tie_rows(n_in, n, K, dtype, s, step=2 if n > 8192 else 1)
    rot = hc.rotate(x, n, K, had_table["mats"].get(K), dtype, 0)
    assert (np.abs(rot) == np.abs(rot[:, :1])).all()
    ties, flips = hc.tie_shares(rot, s)
    print(f"{n}x{K} {dtype} s={s}: {x.shape[0]} rows, {ties:.0%} exact ties, {flips:.0%} disagreements")
    assert ties >= 0.5 and n_ties >= 8
    q = rot / np.float32(s)
    if dtype == "f32":
        assert flips >= 0.1
        assert q.min() <= -128.5 and q.max() >= 127.5
    else:
        assert q.min() <= -120 and q.max() >= 120
