"""ts_count_above_many / TheoremIndex.count_above_many: per shard, the rows that rank before each of many documents per
query, wherever the documents live; summed over the shards of a corpus, the documents' ranks.  On the exact lattice
corpora of tests/exact_common.py (scores exact in any summation order), so every check is np.array_equal: the matrix
pass at d = 320 (two-step tail group on bf16) and d = 768, the ts_count_above fallback at d = 200."""
import functools

import numpy as np
import pytest

import exact_common as E
from rank_common import ExactData, exact_many_targets

pytestmark = pytest.mark.gpu

N = 20_001


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


@functools.lru_cache(maxsize=4)
def _exact(metric, d, nq):
    return ExactData(metric, N, d, nq, 3000 + d + (metric == "cos"))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [320, 768, 200])
@pytest.mark.parametrize("metric", ["ip", "cos"])
def test_counts_summed_over_shards_cut_inside_piles_are_the_ranks(ts, metric, d, dtype):
    D = _exact(metric, d, 40)
    n, nq = D.c.shape[0], D.q.shape[0]
    rng = np.random.default_rng(d)
    targets = [exact_many_targets(D, i, rng) for i in range(nq)]
    with ts.TheoremIndex.from_embeddings(D.c, dtype=dtype, metric=metric) as ix:
        ranks, scores = ix.rank_many(D.q, targets)                 # the owner's scores
    cuts = [0, n // 3, n // 2, n]                                  # every cut has planted piles on both sides
    total = [np.zeros(len(t), np.int64) for t in targets]
    for a, b in zip(cuts, cuts[1:]):
        with ts.TheoremIndex.from_embeddings(D.c[a:b], dtype=dtype, metric=metric, row_offset=a) as sh:
            cnt = sh.count_above_many(D.q, scores, targets)
        for i, t in enumerate(targets):
            want = [E.ref_count_above(D.t[i], a, b, scores[i][j], row) if row < n else -1 for j, row in enumerate(t)]
            assert cnt[i].dtype == np.int64 and np.array_equal(cnt[i], want), (a, i, np.flatnonzero(cnt[i] != np.array(want))[:5])
            total[i] += cnt[i]
    for i, t in enumerate(targets):
        t = np.array(t)
        ok = t < n
        assert np.array_equal(total[i][ok], D.rank[i, t[ok]]), i
        assert np.array_equal(total[i][ok], ranks[i][ok]) and (ranks[i][~ok] == -1).all(), i


@pytest.mark.parametrize("dtype,d", [("bf16", 320), ("f32", 320), ("bf16", 200)])
def test_ragged_lists_foreign_ids_and_nan_scores(ts, dtype, d):
    """300 queries (two blocks) against the middle shard: an empty list, 41 targets (three passes), repeats, documents
    before the first and behind the last row of the shard, scores on and between the lattice values, a NaN score."""
    D = _exact("ip", d, 300)
    n, nq = D.c.shape[0], D.q.shape[0]
    a, b = n // 3, n // 2
    rng = np.random.default_rng(17 + d)
    ids, scs = [], []
    for i in range(nq):
        m = 0 if i == 1 else (41 if i in (0, nq - 1) else int(rng.integers(1, 7)))
        gid = rng.integers(0, n, m)                                  # before, inside and behind the shard
        sc = D.t[i, gid].copy()                                      # the documents' own scores: ties with rows of the shard
        if m >= 4:
            gid[1], sc[1] = gid[0], sc[0]                            # a repeat
            sc[2] += np.float32(2.0 ** -10)                          # between two lattice values
            gid[3] = n + 1000                                        # no row of any shard; behind this one
        if m >= 5:
            gid[4] = -7                                              # before every shard
        if m and i % 5 == 0:
            sc[m - 1] = np.nan
        ids.append(gid.astype(np.int64))
        scs.append(sc.astype(np.float32))
    with ts.TheoremIndex.from_embeddings(D.c[a:b], dtype=dtype, metric="ip", row_offset=a) as sh:
        cnt = sh.count_above_many(D.q, scs, ids)
        single = [i for i in range(nq) if len(ids[i]) == 1]
        one = sh.count_above(D.q[single], [scs[i][0] for i in single], [ids[i][0] for i in single])
        with pytest.raises(ValueError):
            sh.count_above_many(D.q, scs, ids[:-1] + [ids[-1][:-1]])
    assert len(cnt) == nq and cnt[1].shape == (0,)
    for i in range(nq):
        want = [-1 if s != s else E.ref_count_above(D.t[i], a, b, s, g) for s, g in zip(scs[i], ids[i])]
        assert np.array_equal(cnt[i], want), (i, cnt[i], want)
    assert len(single) > 10 and np.array_equal(one, [cnt[i][0] for i in single])
    assert any(s != s for sc in scs for s in sc)


def test_single_target_lists_equal_count_above_on_the_fallback(ts):
    """d = 200: one ts_count_above per target column, so a single-target list is ts_count_above's own answer."""
    D = _exact("cos", 200, 40)
    n, nq = D.c.shape[0], D.q.shape[0]
    a, b = n // 3, n // 2
    t = D.order[np.arange(nq), 3 * np.arange(nq) % 300].astype(np.int64)
    sc = D.t[np.arange(nq), t]
    with ts.TheoremIndex.from_embeddings(D.c[a:b], dtype="bf16", metric="cos", row_offset=a) as sh:
        many = sh.count_above_many(D.q, [[s] for s in sc], [[x] for x in t])
        one = sh.count_above(D.q, sc, t)
    assert np.array_equal(np.concatenate(many), one)
    assert np.array_equal(one, [E.ref_count_above(D.t[i], a, b, sc[i], t[i]) for i in range(nq)])


def test_sharded_searcher_rank_many_of_one_rank_is_the_index_answer(ts):
    from theoremsearch_amd.distributed import ShardedSearcher
    D = _exact("cos", 320, 40)
    rng = np.random.default_rng(3)
    targets = [exact_many_targets(D, i, rng) for i in range(D.q.shape[0])]
    with ts.TheoremIndex.from_embeddings(D.c, dtype="bf16", metric="cos") as ix:
        searcher = ShardedSearcher(index=ix)
        assert searcher.world == 1
        ranks, scores = searcher.rank_many(D.q, targets)
        want_r, want_s = ix.rank_many(D.q, targets)
    for i in range(len(targets)):
        assert np.array_equal(ranks[i], want_r[i]) and np.array_equal(scores[i], want_s[i], equal_nan=True), i
