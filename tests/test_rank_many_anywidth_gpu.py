"""ts_rank_many on the matrix pass at every served width (rank_plan.h: every multiple of 64 from 128 up to a 4,096-byte
row): the bf16 widths with d % 128 == 64, whose last group of k-steps has two steps instead of four, the bf16 rows past
2,048 bytes on the 32-row tile, the fp32 widths between the four earlier ones.  Against the fp64 truth of the oracle, bit
for bit against the exact lattice corpora of tests/exact_common.py, and by the launches the profile brackets count."""
import functools

import numpy as np
import pytest

from oracle import oracle
from rank_common import ExactData, _check_lists, _targets, exact_many_targets

pytestmark = pytest.mark.gpu

WIDTHS = [("bf16", d) for d in (128, 192, 320, 1088, 1536, 1984, 2048)] + [("f32", d) for d in (128, 192, 640, 960)]


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


@pytest.mark.parametrize("nq", [19, 300])
@pytest.mark.parametrize("dtype,d", WIDTHS)
def test_rank_many_matches_the_truth_at_every_served_width(ts, dtype, d, nq):
    n = 1999
    q, c = oracle.inputs(n, nq, d, 100 + d + nq, "cos")
    qp, cp = oracle.prepared_inputs(q, c, "cos", dtype)
    truth = oracle.scores_fp64(qp, cp)
    targets = _targets(truth, nq, n)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="cos") as ix:
        ranks, scores = ix.rank_many(q, targets)
    _check_lists(truth, targets, ranks, scores, n)
    assert ranks[0][0] == 0 and ranks[0][1] == n - 1 and ranks[0][2] == 7


@functools.lru_cache(maxsize=4)
def _exact(metric, d):
    return ExactData(metric, 20_001, d, 64, 2000 + d + (metric == "cos"))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [192, 320, 960])
@pytest.mark.parametrize("metric", ["ip", "cos"])
def test_exact_corpora_rank_canonically_with_exact_scores(ts, metric, d, dtype):
    """Scores that are exact in any summation order: the canonical rank and the truth's score bits for whole piles, piles
    split by a pass of 16, the zero pile, repeats and a row past n.  A k-step multiplied past the row end (the next LDS
    row's first bytes) would move scores off the lattice values."""
    D = _exact(metric, d)
    n, nq = D.c.shape[0], D.q.shape[0]
    rng = np.random.default_rng(d)
    targets = [exact_many_targets(D, i, rng) for i in range(nq)]
    with ts.TheoremIndex.from_embeddings(D.c, dtype=dtype, metric=metric) as ix:
        ranks, scores = ix.rank_many(D.q, targets)
    for i, t in enumerate(targets):
        t = np.array(t)
        ok = t < n
        want = np.where(ok, D.rank[i, np.minimum(t, n - 1)], -1)
        assert np.array_equal(ranks[i], want), (i, np.flatnonzero(ranks[i] != want)[:5])
        assert np.array_equal(scores[i][ok].view(np.uint32), D.t[i, t[ok]].view(np.uint32)), i      # the same bits (+0 for a zero)
        assert np.isnan(scores[i][~ok]).all(), i


@pytest.mark.parametrize("dtype,d", [("bf16", 1088), ("bf16", 1984), ("f32", 960)])
def test_duplicate_row_ranks_right_behind_its_twin(ts, dtype, d):
    """A row stored at two ids scores the same at both and ranks r, r + 1: the gather launch's score of a target is the
    counting pass's score of that row, bit for bit, also through the two-step tail group and on the 32-row tile."""
    n, nq = 3001, 40
    q, c = oracle.inputs(n, nq, d, 7, "cos")
    c[901] = c[17]
    c[2999] = c[5]
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="cos") as ix:
        ranks, scores = ix.rank_many(q, [[17, 901, 2999, 5]] * nq)
    for i in range(nq):
        r, s = ranks[i], scores[i]
        assert s[0].tobytes() == s[1].tobytes() and r[1] == r[0] + 1, (i, r, s)
        assert s[2].tobytes() == s[3].tobytes() and r[2] == r[3] + 1, (i, r, s)


@pytest.mark.parametrize("n", [10, 31, 33, 63, 65, 129])
@pytest.mark.parametrize("dtype,d", [("bf16", 192), ("bf16", 1984), ("f32", 640)])
@pytest.mark.parametrize("metric", ["cos", "ip"])
def test_small_corpora_and_last_partial_tile(ts, metric, dtype, d, n):
    nq = 19
    q, c = oracle.inputs(n, nq, d, n + d, metric)
    qp, cp = oracle.prepared_inputs(q, c, metric, dtype)
    truth = oracle.scores_fp64(qp, cp)
    targets = [[n - 1, 0, n // 2, n - 1 - (i % n)] for i in range(nq)]
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric=metric) as ix:
        ranks, scores = ix.rank_many(q, targets)
    _check_lists(truth, targets, ranks, scores, n)


def test_nan_rows_never_count_and_rank_nowhere(ts):
    n, d, nq = 700, 320, 6
    q, c = oracle.inputs(n, nq, d, 3, "ip")
    c[5, 3] = np.nan
    c[650, d - 1] = np.nan                    # in the two-step tail group
    qp, cp = oracle.prepared_inputs(q, c, "ip", "bf16")
    truth = oracle.scores_fp64(qp, cp)
    order = np.argsort(-np.nan_to_num(truth, nan=-np.inf), axis=1, kind="stable")
    targets = [[5, int(order[i, 0]), int(order[i, 400]), 650, 699] for i in range(nq)]
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        ranks, scores = ix.rank_many(q, targets)
    for i in range(nq):
        assert ranks[i][0] == -1 and np.isnan(scores[i][0]) and ranks[i][3] == -1 and np.isnan(scores[i][3])
        assert ranks[i][1] == 0
    _check_lists(truth, targets, ranks, scores, n)


def test_one_launch_per_256_queries_and_16_targets(ts):
    """The profile brackets the counting launches: ONE over all n rows for 40 queries with three targets each at bf16
    d = 640, four for 300 queries (two blocks) with 17 targets (two passes).  d = 200 is not served: one streaming pass per
    target column, as before, and still the right ranks."""
    n = 20_000
    for d, served in ((640, True), (200, False)):
        q, c = oracle.inputs(n, 300, d, 11 + d, "cos")
        rng = np.random.default_rng(d)
        t3 = [[int(x) for x in rng.integers(0, n, 3)] for _ in range(40)]
        t17 = [[int(x) for x in rng.integers(0, n, 17)] for _ in range(300)]
        with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="cos") as ix:
            ix.profile_enable(True)
            ix.profile_read()
            r3, s3 = ix.rank_many(q[:40], t3)
            p3 = ix.profile_read()
            r17, s17 = ix.rank_many(q, t17)
            p17 = ix.profile_read()
            ix.profile_enable(False)
        print("d", d, "launches", p3, p17)
        if served:
            assert p3["launches"] == 1 and p3["rows_per_launch"] == n, p3
            assert p17["launches"] == 4 and p17["rows_per_launch"] == n, p17
        else:
            assert p3["launches"] == 3 and p17["launches"] == 2 * 17, (p3, p17)      # 17 columns x two blocks of queries
        qp, cp = oracle.prepared_inputs(q[:40], c, "cos", "bf16")
        _check_lists(oracle.scores_fp64(qp, cp), t3, r3, s3, n)
