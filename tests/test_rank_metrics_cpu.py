"""The six retrieval metrics on an IndexRanking past the top-k depth (k=None or k > 256): the rank-based forms, fed by
`rank_many`, against the same functions on the full similarity matrix.  A numpy stand-in for the index (canonical order:
score descending, row ascending) makes this a host-only test; tests/test_rank_many_gpu.py covers the device index."""
import contextlib
import io

import numpy as np
import pytest

from theoremsearch_amd import compare_embeddings as ce

N = 1500
NQ = 9


class FakeIndex:
    """search / rank_of / rank_many of a TheoremIndex, computed on a dense score matrix."""

    def __init__(self, sim):
        self.sim = np.asarray(sim, dtype=np.float64)
        self.n = self.sim.shape[1]
        self.order = np.lexsort((np.arange(self.n)[None, :].repeat(self.sim.shape[0], 0), -self.sim), axis=1)
        self.pos = np.empty_like(self.order)
        np.put_along_axis(self.pos, self.order, np.arange(self.n)[None, :].repeat(self.sim.shape[0], 0), axis=1)
        self.rank_many_calls = 0

    def search(self, q, k):
        idx = self.order[:, :k]
        return np.take_along_axis(self.sim, idx, axis=1), idx

    def _rank(self, i, d):
        return int(self.pos[i, d]) if 0 <= d < self.n else -1

    def rank_of(self, q, docs):
        r = np.array([self._rank(i, int(d)) for i, d in enumerate(docs)], dtype=np.int64)
        return r, np.zeros(len(docs), dtype=np.float32)

    def rank_many(self, q, targets):
        self.rank_many_calls += 1
        ranks = [np.array([self._rank(i, int(d)) for d in t], dtype=np.int64) for i, t in enumerate(targets)]
        return ranks, [np.zeros(len(t), dtype=np.float32) for t in targets]


def _matrix(seed, nq=NQ, n=N):
    rng = np.random.default_rng(seed)
    # tie-free: a random permutation of distinct values per row
    return np.stack([rng.permutation(n).astype(np.float64) / n + 1e-3 * i for i in range(nq)])


def _qrels(sim, seed, empty_query=None):
    rng = np.random.default_rng(seed)
    nq, n = sim.shape
    order = np.argsort(-sim, axis=1)
    qrels = {}
    for q in range(nq):
        if q == empty_query:
            qrels[q] = {}
            continue
        rels = {}
        # graded docs at every depth: the head, the middle, the tail
        for d in rng.choice(order[q, :20], 2, replace=False):
            rels[int(d)] = 0.5
        for d in rng.choice(order[q, 200:], 6, replace=False):
            rels[int(d)] = float(rng.choice([0.5, 1.0, 2.0]))
        rels[int(order[q, rng.integers(250, 1200)])] = 1.0       # the exact doc
        for d in rng.choice(n, 5, replace=False):
            rels.setdefault(int(d), 0)                              # grade 0
        rels[n + 3] = 2.0                                           # not a row of the corpus
        rels[-7] = 1.0 if q % 2 else 0.5
        qrels[q] = rels
    return qrels


def _outcome(fn, *args, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        try:
            v = fn(*args, **kw)
        except Exception as e:        # the matrix form's own errors (P@None divides by None) must be the same
            return ("raise", type(e).__name__, buf.getvalue())
    return ("ok", v, buf.getvalue())


KS = [300, 1000, N, N + 5, None]
GRADED = [ce.ndcg_at_k, ce.err_at_k, ce.q_measure_at_k]
BINARY = [ce.precision_at_k, ce.hit_at_k, ce.mrr_at_k]


def _check(fn, sim, qrels, k, **kw):
    ranking = ce.IndexRanking(FakeIndex(sim), np.zeros((sim.shape[0], 4), dtype=np.float32))
    want = _outcome(fn, sim, qrels, k=k, **kw)
    got = _outcome(fn, ranking, qrels, k=k, **kw)
    assert got == want, (fn.__name__, k, got, want)
    return want


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fn", GRADED + BINARY, ids=lambda f: f.__name__)
def test_metric_equals_matrix_form(fn, k):
    sim = _matrix(1)
    qrels = _qrels(sim, 2)
    out = _check(fn, sim, qrels, k)
    if fn is not ce.precision_at_k or k is not None:
        assert out[0] == "ok" and out[1] > 0.0


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fn", GRADED, ids=lambda f: f.__name__)
def test_empty_query_and_too_small_stdout(fn, k):
    sim = _matrix(3)
    qrels = _qrels(sim, 4, empty_query=5)
    out = _check(fn, sim, qrels, k)
    assert out[0] == "ok"
    if fn is ce.ndcg_at_k:
        assert "TOO SMALL" in out[2]


@pytest.mark.parametrize("k", KS)
def test_linear_gain_and_explicit_max_rel(k):
    sim = _matrix(5)
    qrels = _qrels(sim, 6)
    _check(ce.ndcg_at_k, sim, qrels, k, gain="linear")
    _check(ce.ndcg_at_k, sim, _qrels(sim, 6, empty_query=0), k, gain="linear")
    for mr in (1.0, 3.0):
        _check(ce.err_at_k, sim, qrels, k, max_rel=mr)
        _check(ce.q_measure_at_k, sim, qrels, k, max_rel=mr)


@pytest.mark.parametrize("k", KS)
def test_err_stops_behind_a_saturated_prefix(k):
    # twelve docs of the top grade at the head: the running product falls below 1e-12 and the cascade stops
    sim = _matrix(7)
    order = np.argsort(-sim, axis=1)
    qrels = _qrels(sim, 8)
    for q in range(sim.shape[0]):
        for j in range(12):
            qrels[q][int(order[q, 3 * j + 1])] = 4.0
        qrels[q][int(order[q, 600])] = 4.0
    assert _check(ce.err_at_k, sim, qrels, k)[0] == "ok"
    assert _check(ce.q_measure_at_k, sim, qrels, k)[0] == "ok"
    assert _check(ce.ndcg_at_k, sim, qrels, k)[0] == "ok"


def test_one_rank_many_call_per_qrels():
    sim = _matrix(9)
    qrels = _qrels(sim, 10)
    index = FakeIndex(sim)
    ranking = ce.IndexRanking(index, np.zeros((NQ, 4), dtype=np.float32))
    for fn in GRADED:
        fn(ranking, qrels, k=None)
    ce.hit_at_k(ranking, qrels, k=1000)
    assert index.rank_many_calls == 1
    # grade-0 docs and docs outside the corpus are not positions
    for q, (r, g, docs) in enumerate(ranking.ranks_of_graded(qrels)):
        assert np.all(np.diff(r) > 0) and np.all(g != 0) and np.all((docs >= 0) & (docs < N))
        assert sorted(docs.tolist()) == sorted(d for d, v in qrels[q].items() if v != 0 and 0 <= d < N)


def test_shallow_depths_keep_the_top_k_path():
    # k <= 256 still goes through index.search, as before
    sim = _matrix(11)
    qrels = _qrels(sim, 12)
    index = FakeIndex(sim)
    ranking = ce.IndexRanking(index, np.zeros((NQ, 4), dtype=np.float32))
    for fn in GRADED + BINARY:
        assert fn(ranking, qrels, k=10) == fn(sim, qrels, k=10)
    assert index.rank_many_calls == 0
