"""The search behind a row set per query (ts_search_rowsets, TheoremIndex.search_rowsets) on the GPU: every output row is what
the search behind that query's own set returns - exactly, on lattice corpora where every score is exact; bit for bit against
the per-set calls on Gaussian rows - whichever way the batch was routed: the shared matrix pass, per-set calls, a delegated
call, the exact re-run behind the query's own set.  N = 20,000 leaves the last 64-row staging tile half full; one case has
16,417 rows, a last mask word of one bit."""
import numpy as np
import pytest

import exact_common as E
import rowsets_common as R
from rowsets_common import MFMA, N, N_ODD, SCAN

pytestmark = pytest.mark.gpu

K = 10


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    if _ffi.device_count() == 0:
        pytest.skip("no GPU")
    return ts


@pytest.fixture(scope="module")
def sets(ts):
    makers = {n: R.SetMaker(ts, n) for n in (N, N_ODD)}
    yield makers
    for m in makers.values():
        m.close()


def assign(nq, nsets, seed, with_unfiltered=True):
    """which[]: every set (and -1) named at least once, the rest at random."""
    rng = np.random.default_rng(seed)
    names = list(range(nsets)) + ([-1] if with_unfiltered else [])
    which = np.array(names + list(rng.choice(names, nq - len(names))), dtype=np.int32)
    return which[rng.permutation(nq)]


# ---- 1. exact-score corpora -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d,n", [("bf16", 768, N), ("bf16", 192, N), ("f32", 128, N), ("bf16", 192, N_ODD)],
                         ids=["bf16-768-hand-laid-width", "bf16-192-two-step-tail", "f32-128", "bf16-192-16417-rows"])
def test_exact_scores_behind_five_sets(ts, sets, dtype, d, n):
    nq = 37                                          # two whole blocks of 16 and a partial one; wave 2 holds one block
    q, c, t, order = R.lattice(n, d, nq)
    masks = [R.dense_mask(n, dens, 100 + i) for i, dens in enumerate((0.9, 0.5, 0.2, 0.11))]
    which = assign(nq, len(masks), 3)
    rs = [sets[n](m) for m in masks]
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        scores, idx, stats = ix.search_rowsets(q, K, rs, which, return_stats=True)
    print("stats", stats)
    assert stats["pass_queries"] == nq and stats["algo"] == MFMA and stats["scan_queries"] == 0 and stats["sets_used"] == 4
    for i in range(nq):
        want = E.ref_topk(t[i:i + 1], order[i:i + 1], K, allowed=None if which[i] < 0 else masks[which[i]])
        assert np.array_equal(idx[i], want[1][0]), (i, which[i])
        assert np.array_equal(R.bits(scores[i]), R.bits(want[0][0])), (i, which[i])


# ---- 2. the per-set calls' bits -----------------------------------------------------------------------------------------------
def per_set_mfma(ix, q, k, rs, which, window=16):
    """Row i of the matrix search behind query i's own set: the set's queries as one call - padded with its neighbours up to a
    batch the matrix path takes, since a score's bits do not depend on the batch.  Returns (scores, idx, calls that re-ran a query)."""
    nq = q.shape[0]
    scores, idx = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
    reran = 0
    for w in sorted(set(which.tolist())):
        mine = np.flatnonzero(which == w)
        batch = mine if mine.size >= window else np.concatenate([mine, np.setdiff1d(np.arange(nq), mine)[: window - mine.size]])
        s, i, st = ix.search(q[batch], k, algo="mfma", mask=None if w < 0 else rs[w], return_stats=True)
        assert st["algo"] == MFMA
        reran += 1 if st["fallback_queries"] else 0
        scores[mine], idx[mine] = s[: mine.size], i[: mine.size]
    return scores, idx, reran


def check_against_per_set(ix, q, k, rs, which, got, stats):
    want_s, want_i, reran = per_set_mfma(ix, q, k, rs, which)
    differ = [i for i in range(q.shape[0]) if not R.same_rows((got[0][i], got[1][i]), (want_s[i], want_i[i]))]
    print("rows that differ", differ, "re-run here", stats["fallback_queries"], "calls of the reference that re-ran", reran)
    # a row may differ only where one side re-ran the query (the scan's sum order), and is then the scan's row
    assert len(differ) <= stats["fallback_queries"] + reran * 16
    for i in differ:
        w = which[i]
        s, ids = ix.search(q[i:i + 1], k, algo="scan", mask=None if w < 0 else rs[w])
        assert R.same_rows((got[0][i], got[1][i]), (s[0], ids[0])) or R.same_rows((want_s[i], want_i[i]), (s[0], ids[0])), i


@pytest.mark.parametrize("dtype,d", [("f32", 128), ("bf16", 192)])
@pytest.mark.parametrize("nq,nsets", [(256, 256), (300, 3)], ids=["256-distinct-sets", "300-queries-3-sets"])
def test_same_bits_as_the_per_set_calls(ts, sets, dtype, d, nq, nsets):
    q, c = R.gaussian(d, 300, 900 + d)
    q = q[:nq]
    masks = [R.dense_mask(N, 0.5, 7000 + i) for i in range(nsets)]
    which = np.arange(nq, dtype=np.int32) % nsets
    # the CPU model of the estimate, each query behind its own mask, predicts no re-run for these seeds
    assert R.model_fallbacks(q, c, dtype, K, masks, which) == (0, 0)
    rs = [sets[N](m) for m in masks]
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        scores, idx, stats = ix.search_rowsets(q, K, rs, which, return_stats=True)
        print("stats", stats)
        assert stats["pass_queries"] == nq and stats["algo"] == MFMA and stats["sets_used"] == nsets
        assert stats["fallback_queries"] <= nq // 8
        for i in range(nq):
            assert masks[which[i]][idx[i]].all() and (idx[i] >= 0).all()
        check_against_per_set(ix, q, K, rs, which, (scores, idx), stats)


# ---- 3. mixed routing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("f32", 128), ("bf16", 192)])
def test_mixed_routing_under_auto(ts, sets, dtype, d):
    from theoremsearch_amd import _ffi
    nq = 64
    q, c = R.gaussian(d, 300, 900 + d)
    q = q[:nq]
    masks = [R.dense_mask(N, 0.5, 1), R.dense_mask(N, 0.05, 2), np.zeros(N, dtype=bool)]
    which = np.arange(nq, dtype=np.int32) % 4 - 1            # 16 queries each: -1, dense, sparse, empty
    rs = [sets[N](m) for m in masks]
    ride, groups, calls = R.route(N, [int(m.sum()) for m in masks], which, K, 8 if dtype == "f32" else 4)
    assert sorted(ride.tolist()) == sorted(np.flatnonzero(which <= 0).tolist()) and sorted(groups) == [1, 2] and calls == 1
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        scores, idx, stats = ix.search_rowsets(q, K, rs, which, return_stats=True)
        print("stats", stats)
        assert (stats["pass_queries"], stats["scan_queries"], stats["scan_calls"]) == (ride.size, 32, calls)
        assert stats["algo"] == MFMA and stats["sets_used"] == 3
        # the pass's rows against the per-set matrix calls, the sparse set's against its own call under auto (the scan)
        check_against_per_set(ix, q[ride], K, rs, which[ride], (scores[ride], idx[ride]), stats)
        sparse = np.flatnonzero(which == 1)
        want = ix.search(q[sparse], K, algo="auto", mask=rs[1], return_stats=True)
        assert want[2]["algo"] == SCAN and R.same_rows((scores[sparse], idx[sparse]), want[:2])
        empty = np.flatnonzero(which == 2)
        assert np.all(np.isneginf(scores[empty])) and np.all(idx[empty] == -1)
        with pytest.raises(_ffi.TSearchError) as e:
            ix.search_rowsets(q, K, rs, which, algo="mfma")
        assert e.value.code == -5 and "TS_ALGO_MFMA" in str(e.value)
        # algo = scan: every set's queries through the scan, the per-set scan's bits
        s2, i2, st2 = ix.search_rowsets(q, K, rs, which, algo="scan", return_stats=True)
        assert (st2["algo"], st2["pass_queries"], st2["scan_queries"], st2["scan_calls"]) == (SCAN, 0, nq, 3)
        for w in (-1, 0, 1):
            mine = np.flatnonzero(which == w)
            assert R.same_rows((s2[mine], i2[mine]), ix.search(q[mine], K, algo="scan", mask=None if w < 0 else rs[w])), w
        assert np.all(np.isneginf(s2[empty])) and np.all(i2[empty] == -1)


# ---- 4. delegation ----------------------------------------------------------------------------------------------------------
def test_one_set_and_no_set_are_the_existing_calls(ts, sets):
    nq = 64
    q, c, t, order = R.lattice(N, 768, 37)
    q = np.concatenate([q, q[:27]])
    mask = R.dense_mask(N, 0.5, 11)
    rs = [sets[N](mask), None]
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        for algo in ("auto", "mfma", "scan"):
            got = ix.search_rowsets(q, K, rs, np.zeros(nq, np.int32), algo=algo, return_stats=True)
            want = ix.search(q, K, algo=algo, mask=rs[0], return_stats=True)
            assert R.same_rows(got[:2], want[:2]), algo
            assert got[2]["algo"] == want[2]["algo"] and got[2]["pass_queries"] == 0 and got[2]["sets_used"] == 1
            assert (got[2]["scan_queries"], got[2]["scan_calls"]) == (nq, 1)
            got = ix.search_rowsets(q, K, rs, np.full(nq, -1, np.int32), algo=algo, return_stats=True)
            want = ix.search(q, K, algo=algo, return_stats=True)
            assert R.same_rows(got[:2], want[:2]) and got[2]["algo"] == want[2]["algo"] and got[2]["sets_used"] == 0, algo
        assert ix.search(q, K, algo="auto", mask=rs[0], return_stats=True)[2]["screened"] == 1      # the screened path was the one compared
        got = ix.search_rowsets(q, K, [], np.full(nq, -1, np.int32))
        assert R.same_rows(got, ix.search(q, K))
        s, i = ix.search_rowsets(q[:0], K, rs, np.zeros(0, np.int32))
        assert s.shape == (0, K) and i.shape == (0, K)


# ---- 5. the re-run obeys the query's own set ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("f32", 128), ("bf16", 192)])
def test_rerun_runs_behind_the_querys_own_set(ts, sets, dtype, d):
    nq = 64
    q, c = R.gaussian(d, 300, 900 + d)
    q, c = q[:nq], c.copy()
    rng = np.random.default_rng(8)
    picked = rng.permutation(N)[:2005]
    nan_rows, good = picked[:2000], np.sort(picked[2000:])
    c[nan_rows, rng.integers(0, d, 2000)] = np.nan
    small = np.zeros(N, dtype=bool)
    small[picked] = True                                     # 2,005 rows: a tenth of the corpus, five of them with a score
    dense = R.dense_mask(N, 0.5, 12)
    which = np.zeros(nq, np.int32)
    which[17] = 1
    rs = [sets[N](dense), sets[N](small)]
    t = R.stored(q, dtype).astype(np.float64) @ R.stored(np.nan_to_num(c), dtype).astype(np.float64).T
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        scores, idx, stats = ix.search_rowsets(q, K, rs, which, return_stats=True)
        print("stats", stats)
        assert stats["pass_queries"] == nq and stats["fallback_queries"] >= 1
        want = good[np.argsort(-t[17, good], kind="stable")]
        assert idx[17].tolist() == want.tolist() + [-1] * (K - 5)
        # (a sum of d products of stored values, each at most 1 in magnitude, in fp32: d * 2^-24 < 1e-4)
        assert np.allclose(scores[17, :5], t[17, want], rtol=0, atol=1e-4) and np.all(np.isneginf(scores[17, 5:]))
        others = np.flatnonzero(which == 0)
        check_against_per_set(ix, q[others], K, rs, which[others], (scores[others], idx[others]), dict(stats, fallback_queries=0))
        live = dense & ~np.isnan(c).any(axis=1)
        for i in others:
            assert live[idx[i]].all() and np.unique(idx[i]).size == K, i
            kth = np.sort(t[i, live])[-K]
            assert (t[i, idx[i]] >= kth - 1e-4).all() and np.allclose(scores[i], t[i, idx[i]], rtol=0, atol=1e-4), i


# ---- 6. large k -------------------------------------------------------------------------------------------------------------
def test_large_k_rides_the_pass_from_two_queries_on(ts, sets):
    k, nq = 200, 8
    q, c, t, order = R.lattice(N, 192, 37)
    q, t, order = q[:nq], t[:nq], order[:nq]
    masks = [R.dense_mask(N, 0.9, 100), R.dense_mask(N, 0.5, 101)]
    which = np.arange(nq, dtype=np.int32) % 2
    rs = [sets[N](m) for m in masks]
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        scores, idx, stats = ix.search_rowsets(q, k, rs, which, return_stats=True)
    print("stats", stats)
    assert stats["pass_queries"] == nq and stats["algo"] == MFMA
    for i in range(nq):
        want = E.ref_topk(t[i:i + 1], order[i:i + 1], k, allowed=masks[which[i]])
        assert np.array_equal(idx[i], want[1][0]) and np.array_equal(R.bits(scores[i]), R.bits(want[0][0])), i


# ---- 7. the device form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [256, 100], ids=["256-read-in-place", "100-prepared"])
def test_device_form_gives_the_host_forms_bits(ts, sets, nq):
    import torch
    q, c = R.gaussian(128, 300, 900 + 128)
    q = q[:nq]
    masks = [R.dense_mask(N, 0.5, 7000 + i) for i in range(3)] + [R.dense_mask(N, 0.05, 2)]
    which = np.arange(nq, dtype=np.int32) % 5 - 1            # -1, three dense sets and a sparse one (gathered on the device)
    rs = [sets[N](m) for m in masks]
    with ts.TheoremIndex.from_embeddings(c, dtype="f32", metric="ip") as ix:
        want = ix.search_rowsets(q, K, rs, which, return_stats=True)
        qd = torch.from_numpy(q).cuda()
        out_s = torch.full((nq, K), 7.0, dtype=torch.float32, device="cuda")
        out_i = torch.full((nq, K), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            stats = ix.search_rowsets_device(qd.data_ptr(), "f32", nq, K, rs, which, out_s.data_ptr(), out_i.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert R.same_rows((out_s.cpu().numpy(), out_i.cpu().numpy()), want[:2])
        assert {k: v for k, v in stats.items() if k != "candidates"} == {k: v for k, v in want[2].items() if k != "candidates"}
        assert stats["pass_queries"] == int((which != 3).sum()) and stats["scan_calls"] == 1
        # all queries on the pass: no gather, the caller's buffers themselves
        dense_only = np.arange(nq, dtype=np.int32) % 3
        want = ix.search_rowsets(q, K, rs, dense_only)
        with torch.cuda.stream(stream):
            ix.search_rowsets_device(qd.data_ptr(), "f32", nq, K, rs, dense_only, out_s.data_ptr(), out_i.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert R.same_rows((out_s.cpu().numpy(), out_i.cpu().numpy()), want)


# ---- 8. sessions ----------------------------------------------------------------------------------------------------------------
def test_sessions_equal_one_search_per_session(ts, sets):
    from theoremsearch_amd import pgvector
    nq = 32
    q, c, t, order = R.lattice(N, 192, 37)               # exact scores: the same similarity on whichever path a session runs
    q = q[:nq]
    masks = [R.dense_mask(N, 0.5, 101), R.dense_mask(N, 0.2, 102), R.dense_mask(N, 0.05, 2)]
    rs = [sets[N](m) for m in masks]
    rng = np.random.default_rng(4)
    session_masks = [None if w < 0 else rs[w] for w in rng.integers(-1, 3, nq)]
    top_ks = [1 + (7 * i) % 20 for i in range(nq)]
    assert min(top_ks) == 1 and max(top_ks) == 20
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        got = pgvector.search_sessions(ix, q, top_ks, session_masks)
        assert len(got) == nq
        for i in range(nq):
            assert got[i] == pgvector.search(ix, q[i], top_ks[i], mask=session_masks[i]), i
            assert len(got[i]) == top_ks[i]
