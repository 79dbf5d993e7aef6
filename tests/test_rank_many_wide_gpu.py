"""ts_rank_many / ts_count_above_many on the k-chunked matrix pass (theoremsearch_amd/csrc/kernels_rank_wide.h; rank_wide_plan.h:
d % 256 == 0, a row of more than 4,096 and at most 16,384 bytes - bf16 d = 2,304 .. 8,192, fp32 d = 1,280 .. 4,096).  Bit for bit
on the block-marker corpus of tests/wide_common.py (integer scores, exact in fp32 in any order, many ties), against the fp64
truth of the oracle, against the bits the k-chunked search returns, and by the launches the profile brackets count.  The option
TS_MFMA_GRID sets the workgroups of the counting launch at these widths: 1 = one workgroup walks every tile (the buffer turn
crosses tiles), 3 = uneven ranges, unset = one per CU, most of them without a tile at these sizes."""
import functools

import numpy as np
import pytest

import rank_wide_common as RW
import wide_common as WC
from oracle import oracle
from rank_common import _check_lists, _targets

pytestmark = pytest.mark.gpu

MARKER = [(dtype, d) for dtype in ("bf16", "f32") for d in WC.MARKER_WIDTHS[dtype]]


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


@functools.lru_cache(maxsize=2)
def _marker(d):
    """The marker corpus with its canonical rank matrix (score descending, row ascending)."""
    q, c, exact = WC.marker_corpus(d)
    n = c.shape[0]
    rank = np.empty(exact.shape, dtype=np.int64)
    for i in range(exact.shape[0]):
        rank[i, np.lexsort((np.arange(n), -exact[i]))] = np.arange(n)
    return q, c, exact, rank


@pytest.mark.parametrize("dtype,d", MARKER, ids=lambda v: str(v))
def test_marker_corpus_ranks_canonically_with_the_integers_bits(ts, dtype, d):
    """A chunk dropped, added twice, taken from the wrong place of the row or read from a buffer that still holds an earlier
    chunk moves a score off its integer (tests/test_wide_common_cpu.py); a miscounted tie moves a rank."""
    q, c, exact, rank = _marker(d)
    n = c.shape[0]
    rng = np.random.default_rng(d)
    every = [list(range(n)) for _ in range(17)]                      # more than 16 a query: several passes
    some = []
    for i in range(256):
        t = [int(x) for x in rng.integers(0, n, 17)] + [n - 1]
        some.append(t + [t[3], n + 4])                               # a repeat and a row past n: 20 targets
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        for grid in (1, 3, None):
            ix.set_option("TS_MFMA_GRID", grid)
            for qq, targets in ((q[:17], every), (q, some)):
                ranks, scores = ix.rank_many(qq, targets)
                for i, t in enumerate(targets):
                    t = np.array(t)
                    ok = t < n
                    want = np.where(ok, rank[i, np.minimum(t, n - 1)], -1)
                    assert np.array_equal(ranks[i], want), (grid, len(targets), i, np.flatnonzero(ranks[i] != want)[:5])
                    assert np.array_equal(scores[i][ok].view(np.uint32), exact[i, t[ok]].astype(np.float32).view(np.uint32)), (grid, i)
                    assert np.isnan(scores[i][~ok]).all(), (grid, i)
        ix.set_option("TS_MFMA_GRID", None)


@pytest.mark.parametrize("nq", RW.PARITY_NQ)
@pytest.mark.parametrize("dtype,d", RW.PARITY_WIDTHS, ids=lambda v: str(v))
def test_rank_many_matches_the_truth_at_the_k_chunked_widths(ts, dtype, d, nq):
    n = RW.PARITY_N
    q, c, qp, cp = RW.parity_inputs(dtype, d, nq)
    truth = oracle.scores_fp64(qp, cp)
    targets = _targets(truth, nq, n)                                 # ragged, an empty list, 41 targets, a repeat, a row past n
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric=RW.PARITY_METRIC) as ix:
        ranks, scores = ix.rank_many(q, targets)
    _check_lists(truth, targets, ranks, scores, n)
    assert ranks[0][0] == 0 and ranks[0][1] == n - 1 and ranks[0][2] == 7


@pytest.mark.parametrize("dtype,d", [("bf16", 2560), ("f32", 1536)])
def test_the_top_ten_of_the_search_rank_zero_to_nine_with_the_searchs_bits(ts, dtype, d):
    """One chain of MFMAs per score at the same lanes with the same query addressing as the search's pass: the gather launch
    returns the search's bits, and the counting pass counts with them."""
    n, nq, k = 20_011, 256, 10
    q, c = oracle.inputs(n, nq, d, 31 + d, "ip")
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        s, idx, st = ix.search(q, k, algo="mfma", return_stats=True)
        assert st["fallback_queries"] == 0, st
        targets = [[int(x) for x in idx[i]] for i in range(nq)]
        for grid in (None, 16):                                      # 16: every workgroup walks about twenty tiles
            ix.set_option("TS_MFMA_GRID", grid)
            ranks, scores = ix.rank_many(q, targets)
            for i in range(nq):
                assert np.array_equal(ranks[i], np.arange(k)), (grid, i, ranks[i])
                assert np.array_equal(scores[i].view(np.uint32), s[i].view(np.uint32)), (grid, i)
        ix.set_option("TS_MFMA_GRID", None)


@pytest.mark.parametrize("dtype,d", [("bf16", 2304), ("f32", 1280)])
def test_duplicate_row_ranks_right_behind_its_twin(ts, dtype, d):
    """A row stored at two ids scores the same at both and ranks r, r + 1: the gather launch's score of a target is the
    counting pass's score of that row, bit for bit, also through the 512-byte last chunk of bf16 2,304."""
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


@pytest.mark.parametrize("n", [10, 63, 64, 65, 129, 257])
@pytest.mark.parametrize("dtype,d", [("bf16", 2304), ("f32", 1536)])
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


@pytest.mark.parametrize("dtype,d", [("bf16", 2304), ("f32", 1280)])
def test_nan_rows_never_count_and_rank_nowhere(ts, dtype, d):
    n, nq = 700, 6
    q, c = oracle.inputs(n, nq, d, 3, "ip")
    c[5, 3] = np.nan                          # in the first chunk
    c[650, d - 1] = np.nan                    # in the last chunk (bf16 2,304: the 512-byte one)
    qp, cp = oracle.prepared_inputs(q, c, "ip", dtype)
    truth = oracle.scores_fp64(qp, cp)
    order = np.argsort(-np.nan_to_num(truth, nan=-np.inf), axis=1, kind="stable")
    targets = [[5, int(order[i, 0]), int(order[i, 400]), 650, 699, int(order[i, n - 3])] for i in range(nq)]
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        ranks, scores = ix.rank_many(q, targets)
    for i in range(nq):
        assert ranks[i][0] == -1 and np.isnan(scores[i][0]) and ranks[i][3] == -1 and np.isnan(scores[i][3])
        assert ranks[i][1] == 0
    _check_lists(truth, targets, ranks, scores, n)       # the two rows move no other rank: the last real one ranks n - 3


def test_one_launch_per_256_queries_and_16_targets(ts):
    """The profile brackets the counting launches: ONE over all n rows for 40 queries with three targets each at bf16
    d = 2,560, four for 300 queries (two blocks) with 17 targets (two passes).  d = 2,368 is no multiple of 256: one streaming
    pass per target column, as before, and still the right ranks."""
    n = 5000
    for d, served in ((2560, True), (2368, False)):
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


def test_counts_summed_over_two_shards_are_the_ranks(ts):
    """count_above_many at bf16 d = 2,560: the corpus cut into two indexes with row offsets; for every target - its own shard's,
    the other shard's, a repeat, a document with a NaN score - the two counts add up to rank_many's rank on the whole index
    (a score's bits depend on the width and the storage type only, so the shards count with the owner's bits).  One counting
    launch per 256 queries and 16 targets on each shard."""
    n, nq, d, cut = 3001, 300, 2560, 1237
    q, c = oracle.inputs(n, nq, d, 23, "ip")
    c[2000, 9] = np.nan
    rng = np.random.default_rng(5)
    targets = []
    for i in range(nq):
        m = 17 if i in (0, nq - 1) else int(rng.integers(1, 7))
        t = [int(x) for x in rng.integers(0, n, m)]
        if m >= 3:
            t[1] = t[0]                                              # a repeat
            t[2] = 2000                                              # the NaN row
        targets.append(t)
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        ranks, scores = ix.rank_many(q, targets)
    total = [np.zeros(len(t), np.int64) for t in targets]
    for a, b in ((0, cut), (cut, n)):
        with ts.TheoremIndex.from_embeddings(c[a:b], dtype="bf16", metric="ip", row_offset=a) as sh:
            sh.profile_enable(True)
            sh.profile_read()
            cnt = sh.count_above_many(q, scores, targets)
            p = sh.profile_read()
            sh.profile_enable(False)
        assert p["launches"] == 4 and p["rows_per_launch"] == b - a, p      # two blocks of queries x two passes of targets
        for i in range(nq):
            assert cnt[i].dtype == np.int64 and cnt[i].shape == (len(targets[i]),)
            nan = np.isnan(scores[i])
            assert (cnt[i][nan] == -1).all() and (cnt[i][~nan] >= 0).all(), i
            total[i] += cnt[i]
    seen_nan = seen_foreign = 0
    for i, t in enumerate(targets):
        nan = np.isnan(scores[i])
        assert np.array_equal(nan, np.array(t) == 2000), i
        assert (ranks[i][nan] == -1).all() and np.array_equal(total[i][~nan], ranks[i][~nan]), (i, total[i], ranks[i])
        seen_nan += int(nan.sum())
        seen_foreign += int(any(x < cut for x in t) and any(x >= cut for x in t))     # each shard counts for the other's rows
    assert seen_nan > 10 and seen_foreign > 10
