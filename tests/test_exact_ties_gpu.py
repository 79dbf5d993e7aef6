"""Exact ties on every search, rank and count path.  The corpora of tests/exact_common.py have fp32 dot products that are
exact in any summation order, so the fp64 truth is the bit-exact answer of every kernel, dtype, tile shape, grid, batch
size and k-split, and the canonical order (score descending, then row ascending) is the only right one.  They carry piles
of exactly tied rows across tile, padding and shard edges and at the k-th positions.  Every check is np.array_equal:
no GAP window, no score tolerance."""
import functools

import numpy as np
import pytest

import exact_common as E

pytestmark = pytest.mark.gpu

N = 150_001                                 # > 16384 (the MFMA path), several tiles per workgroup, not a multiple of 256
NQ_BIG = 300                                # queries of the widths the batch-shape legs use
MFMA_D = (384, 512, 768, 1024)
FALLBACKS = {}                              # (leg, ...) -> fallback_queries of the MFMA pass: recorded, not forbidden


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


class Data:
    def __init__(self, metric, d):
        nq = NQ_BIG if d in (768, 1024) else 64
        self.metric, self.d = metric, d
        self.q, self.c, self.piles = E.make_corpus(metric, N, d, nq, 1000 + d + (metric == "cos"))
        t = E.truth(self.q, self.c, metric)
        self.t = t.astype(np.float32)                       # exact: every score is an fp32 value
        self.order = E.canonical_order(t).astype(np.int32)
        self.rank = E.rank_matrix(self.order)

    def topk(self, nq, k, allowed=None):
        return E.ref_topk(self.t[:nq], self.order[:nq], k, allowed)


@functools.lru_cache(maxsize=2)
def data(metric, d):
    return Data(metric, d)


def assert_topk(got_s, got_i, want_s, want_i, what):
    bad = np.argwhere(got_i != want_i)
    assert bad.size == 0, (what, bad[:5].tolist(), [(int(got_i[b, r]), int(want_i[b, r])) for b, r in bad[:5]])
    assert np.array_equal(got_s, want_s), what


def served(dtype, d):
    return ("scan", "mfma") if d in MFMA_D else ("scan",)


CASES = [(m, d, dt) for m in ("ip", "cos") for d in (200, 384, 512, 768, 1024) for dt in ("f32", "bf16")]


@pytest.fixture(scope="module", params=CASES, ids=lambda p: "-".join(map(str, p)))
def case(request, ts):
    metric, d, dtype = request.param
    D = data(metric, d)
    ix = ts.TheoremIndex.from_embeddings(D.c, dtype=dtype, metric=metric)
    yield D, ix, dtype
    ix.close()


# ---- search ------------------------------------------------------------------------------------------------------------
def _knobs(dtype, d):
    if dtype == "bf16" and d in (768, 1024):
        return [{"TS_MFMA_SHAPE": 32, "TS_MFMA_AHEAD": 1}, {"TS_MFMA_AHEAD": 2}, {"TS_MFMA_RUN": 4, "TS_MFMA_STAT": 0},
                {"TS_MFMA_GRID": 200, "TS_MFMA_AHEAD": 1}, {"TS_MFMA_SAMPLE": 0}]
    if dtype == "bf16" and d in MFMA_D:
        return [{"TS_MFMA_SHAPE": 32}, {"TS_MFMA_GRID": 64}]
    if dtype == "f32" and d == 768:
        return [{"TS_MFMA_F32": 32}, {"TS_MFMA_F32": 16, "TS_MFMA_GRID": 64}]
    return []


def test_search_returns_the_canonical_order(case):
    """dtype x d x metric x algo x k, then the knobs that change the tile shape, ring depth, runs and grid: the same answer,
    bit for bit, through piles at ranks 1, 10, 100, 256, a pile of ~n rows at 0 and the tile and padding edges."""
    D, ix, dtype = case
    nq = 40
    q = D.q[:nq]
    for k in (1, 10, 256):
        want_s, want_i = D.topk(nq, k)
        for algo in served(dtype, D.d):
            s, i, st = ix.search(q, k, algo=algo, return_stats=True)
            FALLBACKS[(D.metric, D.d, dtype, algo, k)] = st["fallback_queries"]
            assert_topk(s, i, want_s, want_i, (algo, k))
    for knobs in _knobs(dtype, D.d):
        try:
            for name, v in knobs.items():
                ix.set_option(name, v)
            for k in (10, 256):
                want_s, want_i = D.topk(nq, k)
                s, i = ix.search(q, k, algo="mfma")
                assert_topk(s, i, want_s, want_i, (knobs, k))
        finally:
            for name in knobs:
                ix.set_option(name, None)
    print("fallback_queries", {k: v for k, v in FALLBACKS.items() if k[:3] == (D.metric, D.d, dtype)})


# ---- ranks and counts --------------------------------------------------------------------------------------------------
def _rank_targets(D, nq, r):
    """Round r of one target per query: canonical positions at and around the k-th ranks and the pile edges, the last row
    of a tie group, the zero pile's last row."""
    n = D.c.shape[0]
    pos = [0, 1, 2, 3, 9, 10, 14, 15, 99, 100, 114, 115, 255, 256, 314, 315, n // 2, n - 1][r]
    return D.order[:nq, pos].astype(np.int64)


def _generic_rank_selectable(ix):
    """TS_SCAN_GENERIC is an option of the diagnostic build (TS_LIB=.../libtsearch_diag.so); the product build runs the
    generic rank kernel only at the other widths (d = 200 here)."""
    from theoremsearch_amd import _ffi
    try:
        ix.set_option("TS_SCAN_GENERIC", 1)
    except _ffi.TSearchError:
        return False
    ix.set_option("TS_SCAN_GENERIC", None)
    return True


def test_rank_of_agrees_with_the_truth_and_with_search(case):
    """rank_of on the eight specialised rank_kernel shapes (f32 / bf16 x 384 / 512 / 768 / 1024, four queries or one per
    pass) and on the generic kernel (d = 200; every width with TS_SCAN_GENERIC=1 in the diagnostic build): the canonical rank, and search idx[r] == t <=> rank_of(t)
    == r."""
    D, ix, dtype = case
    nq = 40
    q = D.q[:nq]
    _, top = ix.search(q, 256)
    forms = [None] + (["generic"] if D.d in MFMA_D and _generic_rank_selectable(ix) else [])
    for form in forms:
        try:
            if form:
                ix.set_option("TS_SCAN_GENERIC", 1)
            for r in range(18):
                t = _rank_targets(D, nq, r)
                ranks, scores = ix.rank_of(q, t)
                want = D.rank[np.arange(nq), t]
                assert np.array_equal(ranks, want), (form, r, np.flatnonzero(ranks != want)[:5])
                assert np.array_equal(scores, D.t[np.arange(nq), t]), (form, r)
                for b in range(nq):
                    assert (ranks[b] < 256 and top[b, ranks[b]] == t[b]) == (t[b] in top[b]), (form, r, b)
            for b in (0, 1, 2, 3):                                     # one query per pass
                ranks, _ = ix.rank_of(q[b:b + 1], D.order[b, [10 + b]])
                assert ranks[0] == 10 + b, (form, b)
        finally:
            if form:
                ix.set_option("TS_SCAN_GENERIC", None)


def _many_targets(D, i, rng):
    """A whole pile, > 16 rows of one pile (a pass boundary inside it), rows whose score many lower rows share (the fast
    reject's equality), repeats and a row outside the index."""
    n = D.c.shape[0]
    kind = E.kind_of(i)
    if kind == "pileA":
        p2, p3 = D.piles["pileA"][2], D.piles["pileA"][3]
        t = list(np.random.default_rng(i).permutation(p3)) + list(p2[::2][:40]) + [int(p3[0]), int(p2[-1])]
    elif kind in ("pileB", "neg"):
        zeros = D.order[i, 400:]                                      # inside the zero pile
        zeros = zeros[D.t[i, zeros] == 0]
        t = [int(zeros[-1]), int(zeros[-2]), int(zeros[len(zeros) // 2]), int(zeros[0]), n - 1, int(zeros[-1])]
        t += [int(x) for x in D.order[i, :7]]
    else:
        grp = np.flatnonzero(D.t[i] == D.t[i, D.order[i, 256]])       # the tie group at rank 256
        t = [int(x) for x in grp[-20:]] + [int(x) for x in rng.integers(0, n, 8)] + [int(grp[-1]), int(grp[0])]
    return [int(x) for x in t] + [n + 5]


def test_rank_many_agrees_with_rank_of_and_the_truth(case):
    """rank_many (one matrix pass per 256 queries and 16 targets; ts_rank_of per column at d = 200) on whole piles, piles
    split by a pass boundary, the zero pile and repeats, in blocks of 1, 255, 256 and 257 queries: the canonical rank."""
    D, ix, dtype = case
    n = D.c.shape[0]
    rng = np.random.default_rng(D.d)
    for nq in ((1, 255, 256, 257) if D.q.shape[0] >= 257 else (1, 48)):
        targets = [_many_targets(D, i, rng) for i in range(nq)]
        ranks, scores = ix.rank_many(D.q[:nq], targets)
        for i, t in enumerate(targets):
            t = np.array(t)
            ok = t < n
            want = np.where(ok, D.rank[i, np.minimum(t, n - 1)], -1)
            assert np.array_equal(ranks[i], want), (nq, i, np.flatnonzero(ranks[i] != want)[:5])
            assert np.array_equal(scores[i][ok], D.t[i, t[ok]]) and np.isnan(scores[i][~ok]).all(), (nq, i)
        # rank_of of the first target of every query: the same rank
        first = np.array([t[0] for t in targets])
        r1, _ = ix.rank_of(D.q[:nq], first)
        assert np.array_equal(r1, np.array([r[0] for r in ranks])), nq


def test_count_above_summed_over_shards_cut_inside_piles(case, ts):
    D, ix, dtype = case
    n, nq = D.c.shape[0], 40
    q = D.q[:nq]
    cuts = [0, n // 3, n // 2, n]                     # every cut has planted piles on both sides
    shards = [ts.TheoremIndex.from_embeddings(D.c[a:b], dtype=dtype, metric=D.metric, row_offset=a) for a, b in zip(cuts, cuts[1:])]
    try:
        for r in range(0, 18, 3):
            t = _rank_targets(D, nq, r)
            sc = D.t[np.arange(nq), t]
            total = np.zeros(nq, np.int64)
            for sh, a, b in zip(shards, cuts, cuts[1:]):
                cnt = sh.count_above(q, sc, t)
                want = [E.ref_count_above(D.t[i], a, b, sc[i], t[i]) for i in range(nq)]
                assert np.array_equal(cnt, want), (r, a)
                total += cnt
            assert np.array_equal(total, D.rank[np.arange(nq), t]), r
    finally:
        for sh in shards:
            sh.close()


# ---- batch shape and pass form -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "cos"])
@pytest.mark.parametrize("d", [768, 1024])
def test_answers_do_not_depend_on_batch_shape_or_pass_form(ts, d, metric):
    """The same queries in batches of 1 .. 300 (one or two query groups per wave, 192 per workgroup at d = 1024, the paired
    and k-split passes of 193 .. 256 queries, several launches), with TS_MFMA_PAIR default / 0 / 1 and TS_MFMA_GRID 64 /
    200 / 208: every query's answer is the canonical one, so every form gives the same ids and scores."""
    D = data(metric, d)
    want = {k: D.topk(NQ_BIG, k) for k in (10, 100)}
    with ts.TheoremIndex.from_embeddings(D.c, dtype="bf16", metric=metric) as ix:
        for name, values in (("TS_MFMA_PAIR", (None, 0, 1)), ("TS_MFMA_GRID", (64, 200, 208))):
            for v in values:
                try:
                    ix.set_option(name, v)
                    for nq in (1, 16, 17, 128, 129, 192, 193, 200, 256, 300):
                        for k in ((10, 100) if nq in (193, 256) else (10,)):
                            s, i, st = ix.search(D.q[:nq], k, algo="mfma", return_stats=True)
                            FALLBACKS[("batch", metric, d, name, v, nq, k)] = st["fallback_queries"]
                            assert_topk(s, i, want[k][0][:nq], want[k][1][:nq], (name, v, nq, k))
                finally:
                    ix.set_option(name, None)


# ---- filtered and biased search ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["ip", "cos"])
def test_filtered_and_biased_search(ts, metric, dtype):
    D = data(metric, 768)
    n, nq = D.c.shape[0], 40
    q = D.q[:nq]
    rng = np.random.default_rng(17)
    mask = rng.random(n) < 0.6
    for level in D.piles["pileA"] + D.piles["pileB"]:
        mask[level[::2]] = False                                    # the mask cuts through every pile
        mask[level[1::2]] = True
    bias = np.where(rng.random(n) < 0.3, rng.integers(-8, 9, n), 0).astype(np.float32) / np.float32(8)
    biased = D.t[:nq].astype(np.float64) + 0.5 * bias.astype(np.float64)[None, :]   # fmaf(0.5, bias, s): exact here
    border = E.canonical_order(biased)
    with ts.TheoremIndex.from_embeddings(D.c, dtype=dtype, metric=metric) as ix:
        for k in (10, 256):
            want_s, want_i = D.topk(nq, k, allowed=mask)
            for algo in ("scan", "mfma", "auto"):
                s, i = ix.search(q, k, algo=algo, mask=mask)
                assert_topk(s, i, want_s, want_i, ("mask", algo, k))
            for m in (None, mask):
                ws, wi = E.ref_topk(biased, border, k, m)
                s, sims, i = ix.search_biased(q, k, bias, 0.5, mask=m)
                assert_topk(s, i, ws, wi, ("biased", m is not None, k))
                assert np.array_equal(sims, D.t[np.arange(nq)[:, None], wi]), ("sims", k)


# ---- shards and merges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "cos"])
def test_shards_and_merges_keep_the_lower_global_id_first(ts, metric):
    from theoremsearch_amd.distributed import Shards
    D = data(metric, 768)
    n, nq = D.c.shape[0], 40
    q = D.q[:nq]
    with Shards(n, D.d, 3, dtype="bf16", metric=metric, devices=[0, 0, 0]) as sh:
        cuts = [sh.bounds(g)[0] for g in range(3)] + [n]
        for e in cuts[1:-1]:                                        # planted piles straddle the shard cuts
            assert any((lv < e).any() and (lv >= e).any() for lv in D.piles["pileA"] + D.piles["pileB"]), cuts
        sh.upload(D.c, 0)
        for k in (1, 10, 256):
            s, i = sh.search(q, k)
            assert_topk(s, i, *D.topk(nq, k), ("shards", k))
    # per-shard indexes + ts_merge_topk
    parts = [ts.TheoremIndex.from_embeddings(D.c[a:b], dtype="bf16", metric=metric, row_offset=a)
             for a, b in zip(cuts, cuts[1:])]
    try:
        for k in (10, 256):
            res = [p.search(q, k) for p in parts]
            ms, mi = ts.merge_topk(np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), k)
            assert_topk(ms, mi, *D.topk(nq, k), ("merge", k))
    finally:
        for p in parts:
            p.close()
    # parts that are all one score: the k lowest ids, whatever part they come from
    ids = np.random.default_rng(5).permutation(3 * 64).reshape(3, 1, 64).astype(np.int64) + (1 << 33)
    ms, mi = ts.merge_topk(np.zeros((3, 1, 64), np.float32), np.sort(ids, axis=2), 50)
    assert np.array_equal(mi[0], np.sort(ids.reshape(-1))[:50]) and (ms == 0).all()


# ---- metrics -----------------------------------------------------------------------------------------------------------
def test_metrics_on_an_index_ranking_equal_the_tie_broken_truth(ts):
    """The six metrics on an IndexRanking (top-k search for k <= 256, rank_of and rank_many past it) equal the oracle's
    metrics on the truth with ties broken by row: right only if the three kernels agree on the order of tied rows."""
    from oracle import oracle
    from theoremsearch_amd import compare_embeddings as ce
    D = data("cos", 768)
    n, nq = D.c.shape[0], 24
    broken = E.tie_broken(D.t[:nq].astype(np.float64))
    assert np.array_equal(np.argsort(-broken, axis=1), D.order[:nq])
    rng = np.random.default_rng(9)
    gold_pos = [0, 5, 9, 10, 100, 255, 300, 2000, n - 1]
    qrels = {}
    for i in range(nq):
        rels = {int(D.order[i, gold_pos[i % len(gold_pos)]]): 1}
        for p in (1, 2, 3, 11, 50, 256, 257, 999, 1000, 1001, 5000, n // 2):
            rels.setdefault(int(D.order[i, p]), float(rng.choice([0.5, 1.0, 2.0])))
        for j in rng.integers(0, n, 4):
            rels.setdefault(int(j), 0)
        qrels[i] = rels
    fns = ("precision_at_k", "hit_at_k", "mrr_at_k", "ndcg_at_k", "err_at_k", "q_measure_at_k")
    with ts.TheoremIndex.from_embeddings(D.c, dtype="f32", metric="cos") as ix:
        ranking = ce.IndexRanking(ix, D.q[:nq])
        for k in (1, 10, 256, 1000, None):
            for name in fns:
                if name == "precision_at_k" and k is None:
                    continue                                        # P@k divides by k
                got = getattr(ce, name)(ranking, qrels, k=k)
                want = getattr(oracle, name)(broken, qrels, k=k)
                assert abs(got - want) <= 1e-12, (name, k, got, want)
