"""ts_rank_many / TheoremIndex.rank_many: ranks of many target rows per query from one matrix pass (kernels_rank_mfma.h),
against the fp64 truth of the oracle, and the graded metrics past the top-k depth on an IndexRanking."""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

GAP = 1e-6        # fp64 gap below which two ranks count as tied
SCORE_TOL = 1e-5


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


def _targets(truth, seed, n_real):
    """Ragged lists: best, worst, row 7, random rows, a repeat, an out-of-range row; one empty list, one longer than a pass."""
    nq, n = truth.shape
    rng = np.random.default_rng(seed)
    order = np.argsort(-truth, axis=1, kind="stable")
    out = []
    for i in range(nq):
        if nq > 1 and i == 1:
            out.append([])
            continue
        t = [int(order[i, 0]), int(order[i, -1]), int(order[i, min(7, n - 1)])] + [int(x) for x in rng.integers(0, n, 3)]
        t += [t[3], n_real + 5]
        if i == nq - 1:
            t += [int(x) for x in rng.integers(0, n, 33)]       # 41 targets: three passes of 16
        out.append(t)
    return out


def _check_lists(truth, targets, ranks, scores, n):
    for i, t in enumerate(targets):
        r, s = ranks[i], scores[i]
        assert r.shape == (len(t),) and s.shape == (len(t),)
        if not t:
            continue
        exp = oracle.rank_of(truth[[i] * len(t)], t)
        for j, row in enumerate(t):
            if not (0 <= row < n) or truth[i, row] != truth[i, row]:
                assert r[j] == -1 and np.isnan(s[j]), (i, j, row)
                continue
            assert abs(float(s[j]) - truth[i, row]) <= SCORE_TOL, (i, j)
            close = int(np.sum(np.abs(truth[i] - truth[i, row]) <= GAP)) - 1
            assert abs(int(r[j]) - int(exp[j])) <= close, (i, j, row, r[j], exp[j])
        # self-consistency, exact: ranks follow (returned score desc, row asc); repeats share a rank
        seen = {}
        for j, row in enumerate(t):
            if r[j] >= 0:
                if row in seen:
                    assert seen[row] == (int(r[j]), float(s[j]))
                seen[row] = (int(r[j]), float(s[j]))
        rows = sorted(seen, key=lambda x: (-seen[x][1], x))
        rk = [seen[x][0] for x in rows]
        assert rk == sorted(rk) and len(set(rk)) == len(rk), (i, rows, rk)


@pytest.mark.parametrize("nq", [1, 5, 73, 256, 300])
@pytest.mark.parametrize("d", [384, 512, 768, 1024])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rank_many_matches_the_truth(ts, dtype, d, nq):
    n = 1999
    q, c = oracle.inputs(n, nq, d, 100 + d + nq, "cos")
    qp, cp = oracle.prepared_inputs(q, c, "cos", dtype)
    truth = oracle.scores_fp64(qp, cp)
    targets = _targets(truth, nq, n)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="cos") as ix:
        ranks, scores = ix.rank_many(q, targets)
    _check_lists(truth, targets, ranks, scores, n)
    assert ranks[0][0] == 0 and ranks[0][1] == n - 1 and ranks[0][2] == 7


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_duplicate_row_ranks_right_behind_its_twin(ts, dtype):
    """A row stored at two ids scores the same at both and ranks r, r + 1 - the gather launch's score of a target is the
    counting pass's score of that row, bit for bit."""
    n, d, nq = 3001, 768, 40
    q, c = oracle.inputs(n, nq, d, 7, "cos")
    c[901] = c[17]
    c[2999] = c[5]
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="cos") as ix:
        ranks, scores = ix.rank_many(q, [[17, 901, 2999, 5]] * nq)
    for i in range(nq):
        r, s = ranks[i], scores[i]
        assert s[0] == s[1] and r[1] == r[0] + 1, (i, r, s)
        assert s[2] == s[3] and r[2] == r[3] + 1, (i, r, s)


@pytest.mark.parametrize("dtype,d,n", [("bf16", 768, 10), ("bf16", 768, 63), ("bf16", 768, 65), ("bf16", 768, 129),
                                       ("f32", 768, 31), ("f32", 768, 33), ("f32", 1024, 97), ("f32", 384, 127),
                                       ("bf16", 100, 301), ("f32", 100, 77)])
@pytest.mark.parametrize("metric", ["cos", "ip"])
def test_small_corpora_and_last_partial_tile(ts, dtype, d, n, metric):
    nq = 19
    q, c = oracle.inputs(n, nq, d, n + d, metric)
    qp, cp = oracle.prepared_inputs(q, c, metric, dtype)
    truth = oracle.scores_fp64(qp, cp)
    targets = [[n - 1, 0, n // 2, n - 1 - (i % n)] for i in range(nq)]
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric=metric) as ix:
        ranks, scores = ix.rank_many(q, targets)
    _check_lists(truth, targets, ranks, scores, n)


def test_nan_rows_never_count_and_rank_nowhere(ts):
    n, d, nq = 700, 768, 6
    q, c = oracle.inputs(n, nq, d, 3, "ip")
    c[5, 3] = np.nan
    c[650, 0] = np.nan
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


def test_row_offset_and_subset_refusal(ts):
    from theoremsearch_amd import _ffi
    n, d, nq, off = 2500, 512, 7, 1_000_000
    q, c = oracle.inputs(n, nq, d, 9, "cos")
    qp, cp = oracle.prepared_inputs(q, c, "cos", "bf16")
    truth = oracle.scores_fp64(qp, cp)
    local = _targets(truth, 3, n)
    glob = [[x + off for x in t] for t in local]
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="cos", row_offset=off) as ix:
        ranks, scores = ix.rank_many(q, glob)
        _check_lists(truth, local, ranks, scores, n)
        r_local = ix.rank_many(q, [[0, 5]] * nq)[0]
        assert all((r == -1).all() for r in r_local)               # local ids are not rows of an offset index
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="cos") as ix:
        sub = ix.subset(np.arange(0, n, 2)) if hasattr(ix, "subset") else None
        if sub is not None:
            with sub:
                with pytest.raises(_ffi.TSearchError):
                    sub.rank_many(q, [[0]] * nq)


def test_deep_targets_on_half_a_million_rows(ts):
    """256 queries, targets at ranks ~N/2 and N - 1 (every score past the fast reject): exact against a chunked fp64
    count wherever the truth separates the target from its neighbours."""
    n, d, nq = 500_003, 384, 256
    q, c = oracle.inputs(n, nq, d, 21, "cos")
    qp = oracle.prepared_inputs(q, c[:1], "cos", "bf16")[0]
    # fp64 truth one chunk of rows at a time
    tr = np.empty((nq, n), dtype=np.float64)
    for a in range(0, n, 65536):
        cp = oracle.prepared_inputs(q[:1], c[a:a + 65536], "cos", "bf16")[1]
        tr[:, a:a + 65536] = oracle.scores_fp64(qp, cp)
    mid = np.argpartition(-tr, n // 2, axis=1)[:, n // 2]
    worst = np.argmin(tr, axis=1)
    targets = [[int(mid[i]), int(worst[i])] for i in range(nq)]
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="cos") as ix:
        ranks, scores = ix.rank_many(q, targets)
    for i in range(nq):
        for j, row in enumerate(targets[i]):
            s = tr[i]
            exp = int(np.sum(s > s[row]) + np.sum(s[:row] == s[row]))
            close = int(np.sum(np.abs(s - s[row]) <= GAP)) - 1
            assert abs(int(ranks[i][j]) - exp) <= close, (i, j, ranks[i][j], exp, close)
            assert abs(float(scores[i][j]) - s[row]) <= SCORE_TOL
        assert abs(int(ranks[i][0]) - n // 2) <= 1 + int(np.sum(np.abs(tr[i] - tr[i, targets[i][0]]) <= GAP))
    assert sum(int(ranks[i][1]) == n - 1 for i in range(nq)) >= nq - 2


def test_graded_metrics_past_the_top_k_depth(ts):
    """ndcg / err / q_measure at k=None and k=1000 on an IndexRanking (rank_many) equal the oracle's metric on the fp64
    truth, with graded docs the truth pins (no neighbour within GAP)."""
    from theoremsearch_amd import compare_embeddings as ce
    n, d, nq = 5000, 768, 12
    q, c = oracle.inputs(n, nq, d, 31, "cos")
    qp, cp = oracle.prepared_inputs(q, c, "cos", "f32")
    truth = oracle.scores_fp64(qp, cp)
    rng = np.random.default_rng(4)
    qrels = {}
    for i in range(nq):
        s = np.sort(truth[i])
        gaps = np.minimum(np.diff(s, prepend=-np.inf), np.diff(s, append=np.inf))
        pinned = np.flatnonzero(np.isin(truth[i], s[gaps > 10 * GAP]))
        pick = rng.choice(pinned, 10, replace=False)
        rels = {int(x): float(rng.choice([0.5, 1.0, 2.0])) for x in pick}
        rels[int(pick[0])] = 1.0
        rels[int(rng.integers(0, n))] = rels.get(int(rng.integers(0, n)), 0)
        qrels[i] = rels
    with ts.TheoremIndex.from_embeddings(c, dtype="f32", metric="cos") as ix:
        ranking = ce.IndexRanking(ix, q)
        for k in (None, 1000):
            for name in ("ndcg_at_k", "err_at_k", "q_measure_at_k"):
                got = getattr(ce, name)(ranking, qrels, k=k)
                want = getattr(oracle, name)(truth, qrels, k=k)
                assert abs(got - want) <= 1e-12, (name, k, got, want)
        for k in (None, 2000):
            assert ce.hit_at_k(ranking, qrels, k=k) == oracle.hit_at_k(truth, qrels, k=k)
