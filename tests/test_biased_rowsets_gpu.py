"""The citation-weighted search with a weight and a row set per query (ts_search_biased_rowsets,
TheoremIndex.search_biased_rowsets) on the GPU: every output row is what the biased search returns for that query alone with its
own weight behind its own set - exactly, on lattice corpora where every weighted score is exact; bit for bit against the
per-class calls on Gaussian rows; within the oracle's tolerances - whichever way the batch was routed: the shared matrix pass,
per-class calls, a delegated call, the exact re-run behind the query's own set with its own weight.  Each test asserts on the
routing's counters which path answered.  N = 20,000 leaves the last 64-row staging tile half full; one case has 16,417 rows, a
last mask word of one bit."""
import numpy as np
import pytest

import biased_rowsets_common as B
import exact_common as E
import rowsets_common as R
from oracle import oracle
from rowsets_common import MFMA, N, N_ODD, SCAN

pytestmark = pytest.mark.gpu

K = 10
W4 = (0.0, 0.01, 0.02, -0.02)                 # around the citation weight of tests/test_biased_mfma_gpu.py


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


def mask_of(masks, w):
    return None if w < 0 else masks[w]


# ---- 1. exact corpora ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d,n", [("bf16", 768, N), ("bf16", 192, N), ("f32", 128, N), ("bf16", 192, N_ODD)],
                         ids=["bf16-768-hand-laid-width", "bf16-192-two-step-tail", "f32-128", "bf16-192-16417-rows"])
def test_exact_weighted_scores_behind_five_sets(ts, sets, dtype, d, n):
    nq = 37                                          # two whole blocks of 16 and a partial one; wave 2 holds one block
    q, c, t, _ = R.lattice(n, d, nq)
    bias = B.lattice_bias(n)
    masks = [R.dense_mask(n, dens, 100 + i) for i, dens in enumerate((0.9, 0.5, 0.2, 0.11))]
    which, weights = B.classes(nq, len(masks), B.LATTICE_WEIGHTS, 3)
    assert len(set(zip(which.tolist(), weights.tolist()))) == 25
    rs = [sets[n](m) for m in masks]
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        scores, sims, idx, stats = ix.search_biased_rowsets(q, K, bias, weights, rs, which, return_stats=True)
    print("stats", stats)
    assert stats["pass_queries"] == nq and stats["algo"] == MFMA and stats["scan_queries"] == 0 and stats["sets_used"] == 4
    for i in range(nq):
        want_w, want_s, want_i = B.weighted_ref(t[i], bias, weights[i], K, mask_of(masks, which[i]))
        assert np.array_equal(idx[i], want_i), (i, which[i], weights[i])
        assert np.array_equal(R.bits(scores[i]), R.bits(want_w)), (i, which[i], weights[i])
        assert np.array_equal(R.bits(sims[i] + np.float32(0)), R.bits(want_s + np.float32(0))), (i, which[i], weights[i])


# ---- 2. the per-class calls' bits ----------------------------------------------------------------------------------------------
def per_class_mfma(ix, q, k, bias, rs, which, weights, window=16):
    """Row i of the biased matrix search of query i's own class: the class's queries as one call - padded with its neighbours up
    to a batch the matrix path takes, since a score's bits do not depend on the batch.  Returns (scores, sims, idx, calls that
    re-ran a query)."""
    nq = q.shape[0]
    scores, sims, idx = np.empty((nq, k), np.float32), np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
    reran = 0
    for s, w in sorted(set(zip(which.tolist(), weights.tolist()))):
        mine = np.flatnonzero((which == s) & (weights == np.float32(w)))
        batch = mine if mine.size >= window else np.concatenate([mine, np.setdiff1d(np.arange(nq), mine)[: window - mine.size]])
        ws, sm, i, st = ix.search_biased(q[batch], k, bias, w, algo="mfma", mask=mask_of(rs, s), return_stats=True)
        assert st["algo"] == MFMA
        reran += 1 if st["fallback_queries"] else 0
        scores[mine], sims[mine], idx[mine] = ws[: mine.size], sm[: mine.size], i[: mine.size]
    return scores, sims, idx, reran


def same3(a, b):
    return R.same_rows((a[0], a[2]), (b[0], b[2])) and np.array_equal(R.bits(a[1]), R.bits(b[1]))


def check_against_per_class(ix, q, k, bias, rs, which, weights, got, stats):
    want = per_class_mfma(ix, q, k, bias, rs, which, weights)
    reran = want[3]
    differ = [i for i in range(q.shape[0]) if not same3([g[i] for g in got], [w[i] for w in want[:3]])]
    print("rows that differ", differ, "re-run here", stats["fallback_queries"], "calls of the reference that re-ran", reran)
    # a row may differ only where one side re-ran the query (the scan's sum order), and is then the scan's row
    assert len(differ) <= stats["fallback_queries"] + reran * 16
    for i in differ:
        scan = ix.search_biased(q[i:i + 1], k, bias, float(weights[i]), algo="scan", mask=mask_of(rs, which[i]))
        scan = [x[0] for x in scan]
        assert same3([g[i] for g in got], scan) or same3([w[i] for w in want[:3]], scan), i


@pytest.mark.parametrize("dtype,d", [("f32", 128), ("bf16", 192)])
@pytest.mark.parametrize("nq,nsets,nweights", [(256, 64, 4), (300, 3, 2)], ids=["256-classes", "300-queries-6-classes"])
def test_same_bits_as_the_per_class_calls(ts, sets, dtype, d, nq, nsets, nweights):
    q, c = R.gaussian(d, 300, 900 + d)
    q = q[:nq]
    _, bias = B.recipe(N)
    masks = [R.dense_mask(N, 0.5, 7000 + i) for i in range(nsets)]
    which = (np.arange(nq, dtype=np.int32) % nsets).astype(np.int32)
    weights = np.asarray(W4[-nweights:], dtype=np.float32)[(np.arange(nq) // nsets) % nweights]
    assert len(set(zip(which.tolist(), weights.tolist()))) == nsets * nweights
    # the CPU model of the estimate, each query with its own weight behind its own mask, predicts no re-run for these seeds
    assert B.model_fallbacks(q, c, dtype, K, bias, masks, which, weights) == (0, 0)
    rs = [sets[N](m) for m in masks]
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        got = ix.search_biased_rowsets(q, K, bias, weights, rs, which, return_stats=True)
        stats = got[3]
        print("stats", stats, "candidates per query", stats["candidates"] / nq)
        assert stats["pass_queries"] == nq and stats["algo"] == MFMA and stats["sets_used"] == nsets and stats["scan_calls"] == 0
        assert stats["fallback_queries"] <= nq // 8
        for i in range(nq):
            assert masks[which[i]][got[2][i]].all() and (got[2][i] >= 0).all()
        check_against_per_class(ix, q, K, bias, rs, which, weights, got[:3], stats)


# ---- 3. parity with the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d,metric", [("bf16", 192, "cos"), ("f32", 128, "ip")])
def test_parity_with_the_oracle(ts, sets, dtype, d, metric):
    nq = 40
    q, c = oracle.inputs(N, nq, d, 300 + d, metric)
    qp, cp = oracle.prepared_inputs(q, c, metric, dtype)
    sim64 = oracle.scores_fp64(qp, cp)
    cites, bias = B.recipe(N)
    masks = [np.random.default_rng(5).random(N) < 0.4, R.dense_mask(N, 0.9, 31)]
    which = (np.arange(nq, dtype=np.int32) % 3 - 1).astype(np.int32)                   # -1, the 40 % mask, the 90 % mask
    weights = np.asarray((0.02, -0.02, 0.0, 0.05), dtype=np.float32)[(np.arange(nq) // 3) % 4]
    rs = [sets[N](m) for m in masks]
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric=metric) as ix:
        ws, sims, idx, stats = ix.search_biased_rowsets(q, K, bias, weights, rs, which, return_stats=True)
    print("stats", stats, "candidates per query", stats["candidates"] / nq)
    assert stats["pass_queries"] == nq and stats["algo"] == MFMA and stats["fallback_queries"] <= nq // 8
    assert idx.min() >= 0
    for i in range(nq):
        allowed = None if which[i] < 0 else np.flatnonzero(masks[which[i]])
        if allowed is not None:
            assert masks[which[i]][idx[i]].all(), i
        B.check_weighted_query(sim64[i], cites, bias, weights[i], K, ws[i], sims[i], idx[i], allowed, against_oracle=(i == 0))
    assert np.intersect1d(idx[0], np.flatnonzero(bias > 10)).size > 0       # weight 0.02, no filter: the heavily cited rows made it


# ---- 4. mixed routing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("f32", 128), ("bf16", 192)])
def test_mixed_routing_under_auto(ts, sets, dtype, d):
    from theoremsearch_amd import _ffi
    nq = 64
    q, c = R.gaussian(d, 300, 900 + d)
    q = q[:nq]
    _, bias = B.recipe(N)
    masks = [R.dense_mask(N, 0.5, 1), R.dense_mask(N, 0.05, 2), np.zeros(N, dtype=bool)]
    which = (np.arange(nq, dtype=np.int32) % 4 - 1).astype(np.int32)    # 16 queries each: -1, dense, sparse, empty
    weights = np.full(nq, 0.02, dtype=np.float32)
    weights[(which == 0) & (np.arange(nq) % 8 >= 4)] = -0.02           # the dense set under two weights
    rs = [sets[N](m) for m in masks]
    ride, groups, calls = B.route(N, [int(m.sum()) for m in masks], which, weights, K, 8 if dtype == "f32" else 4)
    assert sorted(ride.tolist()) == sorted(np.flatnonzero(which <= 0).tolist()) and sorted(s for s, _ in groups) == [1, 2] and calls == 1
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        got = ix.search_biased_rowsets(q, K, bias, weights, rs, which, return_stats=True)
        stats = got[3]
        print("stats", stats)
        assert (stats["pass_queries"], stats["scan_queries"], stats["scan_calls"]) == (ride.size, 32, calls)
        assert stats["algo"] == MFMA and stats["sets_used"] == 3
        # the pass's rows against the per-class matrix calls, the sparse set's against its own call under auto (the scan)
        check_against_per_class(ix, q[ride], K, bias, rs, which[ride], weights[ride], [g[ride] for g in got[:3]], stats)
        sparse = np.flatnonzero(which == 1)
        want = ix.search_biased(q[sparse], K, bias, 0.02, algo="auto", mask=rs[1], return_stats=True)
        assert want[3]["algo"] == SCAN and same3([g[sparse] for g in got[:3]], want[:3])
        empty = np.flatnonzero(which == 2)
        assert np.all(np.isneginf(got[0][empty])) and np.all(np.isneginf(got[1][empty])) and np.all(got[2][empty] == -1)
        with pytest.raises(_ffi.TSearchError) as e:
            ix.search_biased_rowsets(q, K, bias, weights, rs, which, algo="mfma")
        assert e.value.code == -5 and "TS_ALGO_MFMA" in str(e.value)
        # algo = scan: every class through the scan, the per-class scan's bits
        g2 = ix.search_biased_rowsets(q, K, bias, weights, rs, which, algo="scan", return_stats=True)
        st2 = g2[3]
        assert (st2["algo"], st2["pass_queries"], st2["scan_queries"], st2["scan_calls"]) == (SCAN, 0, nq, 4)
        for s, w in ((-1, 0.02), (0, 0.02), (0, -0.02), (1, 0.02)):
            mine = np.flatnonzero((which == s) & (weights == np.float32(w)))
            assert mine.size and same3([g[mine] for g in g2[:3]], ix.search_biased(q[mine], K, bias, w, algo="scan", mask=mask_of(rs, s))), (s, w)
        assert np.all(np.isneginf(g2[0][empty])) and np.all(g2[2][empty] == -1)


# ---- 5. delegation ------------------------------------------------------------------------------------------------------------------
def test_one_class_is_the_existing_call(ts, sets):
    nq = 64
    q, c, _, _ = R.lattice(N, 768, 37)
    q = np.concatenate([q, q[:27]])
    bias = B.lattice_bias(N)
    mask = R.dense_mask(N, 0.5, 11)
    rs = [sets[N](mask), None]
    w = np.full(nq, 0.25, dtype=np.float32)
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        for algo in ("auto", "mfma", "scan"):
            got = ix.search_biased_rowsets(q, K, bias, w, rs, np.zeros(nq, np.int32), algo=algo, return_stats=True)
            want = ix.search_biased(q, K, bias, 0.25, algo=algo, mask=rs[0], return_stats=True)
            assert same3(got[:3], want[:3]), algo
            assert got[3]["algo"] == want[3]["algo"] and got[3]["pass_queries"] == 0 and got[3]["sets_used"] == 1
            assert (got[3]["scan_queries"], got[3]["scan_calls"]) == (nq, 1)
            got = ix.search_biased_rowsets(q, K, bias, w, rs, np.full(nq, -1, np.int32), algo=algo, return_stats=True)
            want = ix.search_biased(q, K, bias, 0.25, algo=algo, return_stats=True)
            assert same3(got[:3], want[:3]) and got[3]["algo"] == want[3]["algo"] and got[3]["sets_used"] == 0, algo
        s, m, i = ix.search_biased_rowsets(q[:0], K, bias, w[:0], rs, np.zeros(0, np.int32))
        assert s.shape == (0, K) and m.shape == (0, K) and i.shape == (0, K)


# ---- 6. weight zero beside other weights ----------------------------------------------------------------------------------------
def test_weight_zero_queries_are_the_plain_row_set_search(ts, sets):
    nq = 64
    q, c = R.gaussian(128, 300, 900 + 128)
    q = q[:nq]
    _, bias = B.recipe(N)
    masks = [R.dense_mask(N, 0.5, 7000 + i) for i in range(3)]
    which = (np.arange(nq, dtype=np.int32) % 4 - 1).astype(np.int32)
    weights = np.asarray((0.0, 0.02, 0.0, -0.02, 0.05), dtype=np.float32)[np.arange(nq) % 5]
    rs = [sets[N](m) for m in masks]
    with ts.TheoremIndex.from_embeddings(c, dtype="f32", metric="ip") as ix:
        ws, sims, idx, stats = ix.search_biased_rowsets(q, K, bias, weights, rs, which, return_stats=True)
        plain_s, plain_i, pst = ix.search_rowsets(q, K, rs, which, return_stats=True)
    print("stats", stats, pst)
    assert stats["pass_queries"] == nq and pst["pass_queries"] == nq and stats["fallback_queries"] == 0 and pst["fallback_queries"] == 0
    zero = np.flatnonzero(weights == 0)
    assert zero.size >= 20 and len(set(which[zero].tolist())) == 4
    assert np.array_equal(idx[zero], plain_i[zero]) and np.array_equal(R.bits(ws[zero]), R.bits(plain_s[zero]))
    assert np.array_equal(R.bits(sims[zero]), R.bits(plain_s[zero]))
    assert not np.array_equal(idx[weights != 0], plain_i[weights != 0])         # the other queries were ranked by their weight


# ---- 7. the re-run obeys the query's own set and weight ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("f32", 128), ("bf16", 192)])
def test_rerun_runs_behind_the_querys_own_set_with_its_weight(ts, sets, dtype, d):
    nq = 64
    q, c = R.gaussian(d, 300, 900 + d)
    q, c = q[:nq], c.copy()
    _, bias = B.recipe(N)
    rng = np.random.default_rng(8)
    picked = rng.permutation(N)[:2005]
    nan_rows, good = picked[:2000], np.sort(picked[2000:])
    c[nan_rows, rng.integers(0, d, 2000)] = np.nan
    small = np.zeros(N, dtype=bool)
    small[picked] = True                                     # 2,005 rows: a tenth of the corpus, five of them with a score
    dense = R.dense_mask(N, 0.5, 12)
    which = np.zeros(nq, np.int32)
    which[17] = 1
    weights = np.where(np.arange(nq) % 2 == 0, 0.02, -0.02).astype(np.float32)
    weights[17] = 0.05
    rs = [sets[N](dense), sets[N](small)]
    t = R.stored(q, dtype).astype(np.float64) @ R.stored(np.nan_to_num(c), dtype).astype(np.float64).T
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        got = ix.search_biased_rowsets(q, K, bias, weights, rs, which, return_stats=True)
        ws, sims, idx, stats = got
        print("stats", stats)
        assert stats["pass_queries"] == nq and stats["fallback_queries"] >= 1
        weighted17 = t[17, good] + 0.05 * bias[good].astype(np.float64)
        want = good[np.argsort(-weighted17, kind="stable")]
        assert np.diff(np.sort(weighted17)).min() > 2e-4        # the five rows' order does not hang on the scores' 1e-4
        assert idx[17].tolist() == want.tolist() + [-1] * (K - 5)
        # (a sum of d products of stored values, each at most 1 in magnitude, in fp32: d * 2^-24 < 1e-4)
        assert np.allclose(sims[17, :5], t[17, want], rtol=0, atol=1e-4) and np.all(np.isneginf(ws[17, 5:])) and np.all(np.isneginf(sims[17, 5:]))
        assert np.allclose(ws[17, :5], t[17, want] + 0.05 * bias[want].astype(np.float64), rtol=0, atol=1e-4)
        others = np.flatnonzero(which == 0)
        check_against_per_class(ix, q[others], K, bias, rs, which[others], weights[others], [g[others] for g in got[:3]],
                                dict(stats, fallback_queries=0))
        live = dense & ~np.isnan(c).any(axis=1)
        for i in others:
            assert live[idx[i]].all() and np.unique(idx[i]).size == K, i
            wt = t[i] + float(weights[i]) * bias.astype(np.float64)
            kth = np.sort(wt[live])[-K]
            assert (wt[idx[i]] >= kth - 1e-4).all() and np.allclose(ws[i], wt[idx[i]], rtol=0, atol=1e-4), i


# ---- 8. large k -----------------------------------------------------------------------------------------------------------------
def test_large_k_rides_the_pass(ts, sets):
    k, nq = 200, 8
    q, c, t, _ = R.lattice(N, 192, 37)
    q, t = q[:nq], t[:nq]
    bias = B.lattice_bias(N)
    masks = [R.dense_mask(N, 0.9, 100), R.dense_mask(N, 0.5, 101)]
    which = (np.arange(nq, dtype=np.int32) % 2).astype(np.int32)
    weights = np.where(np.arange(nq) % 4 < 2, 0.25, -0.5).astype(np.float32)             # 2 sets x 2 weights
    rs = [sets[N](m) for m in masks]
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        scores, sims, idx, stats = ix.search_biased_rowsets(q, k, bias, weights, rs, which, return_stats=True)
    print("stats", stats)
    assert stats["pass_queries"] == nq and stats["algo"] == MFMA and stats["scan_calls"] == 0
    for i in range(nq):
        want_w, want_s, want_i = B.weighted_ref(t[i], bias, weights[i], k, masks[which[i]])
        assert np.array_equal(idx[i], want_i) and np.array_equal(R.bits(scores[i]), R.bits(want_w)), i
        assert np.array_equal(R.bits(sims[i] + np.float32(0)), R.bits(want_s + np.float32(0))), i


# ---- 9. the device form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [256, 100], ids=["256-read-in-place", "100-prepared"])
def test_device_form_gives_the_host_forms_bits(ts, sets, nq):
    import torch
    q, c = R.gaussian(128, 300, 900 + 128)
    q = q[:nq]
    _, bias = B.recipe(N)
    masks = [R.dense_mask(N, 0.5, 7000 + i) for i in range(3)] + [R.dense_mask(N, 0.05, 2)]
    which = (np.arange(nq, dtype=np.int32) % 5 - 1).astype(np.int32)    # -1, three dense sets and a sparse one (gathered on the device)
    weights = np.asarray(W4, dtype=np.float32)[np.arange(nq) % 4]
    rs = [sets[N](m) for m in masks]
    with ts.TheoremIndex.from_embeddings(c, dtype="f32", metric="ip") as ix:
        want = ix.search_biased_rowsets(q, K, bias, weights, rs, which, return_stats=True)
        qd, bd = torch.from_numpy(q).cuda(), torch.from_numpy(bias).cuda()
        out_s = torch.full((nq, K), 7.0, dtype=torch.float32, device="cuda")
        out_m = torch.full((nq, K), 7.0, dtype=torch.float32, device="cuda")
        out_i = torch.full((nq, K), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            stats = ix.search_biased_rowsets_device(qd.data_ptr(), "f32", nq, K, bd.data_ptr(), weights, rs, which, out_s.data_ptr(),
                                                    out_m.data_ptr(), out_i.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert same3((out_s.cpu().numpy(), out_m.cpu().numpy(), out_i.cpu().numpy()), want[:3])
        assert {k: v for k, v in stats.items() if k != "candidates"} == {k: v for k, v in want[3].items() if k != "candidates"}
        assert stats["pass_queries"] == int((which != 3).sum()) and stats["scan_calls"] == len(set(weights[which == 3].tolist()))
        # all queries on the pass: no gather, the caller's buffers themselves; no out_sims
        dense_only = (np.arange(nq, dtype=np.int32) % 3).astype(np.int32)
        want = ix.search_biased_rowsets(q, K, bias, weights, rs, dense_only)
        with torch.cuda.stream(stream):
            st = ix.search_biased_rowsets_device(qd.data_ptr(), "f32", nq, K, bd.data_ptr(), weights, rs, dense_only, out_s.data_ptr(), 0,
                                                 out_i.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert st["pass_queries"] == nq
        assert R.same_rows((out_s.cpu().numpy(), out_i.cpu().numpy()), (want[0], want[2]))


# ---- 10. sessions ------------------------------------------------------------------------------------------------------------------
def test_sessions_equal_one_weighted_search_per_session(ts, sets):
    from theoremsearch_amd import pgvector
    nq = 32
    q, c, _, _ = R.lattice(N, 192, 37)                    # exact scores: the same similarity on whichever path a session runs
    q = q[:nq]
    bias = B.lattice_bias(N)
    masks = [R.dense_mask(N, 0.5, 101), R.dense_mask(N, 0.2, 102), R.dense_mask(N, 0.05, 2)]
    rs = [sets[N](m) for m in masks]
    rng = np.random.default_rng(4)
    session_masks = [None if w < 0 else rs[w] for w in rng.integers(-1, 3, nq)]
    top_ks = [1 + (7 * i) % 20 for i in range(nq)]
    ws = [B.LATTICE_WEIGHTS[i % 5] for i in range(nq)]
    assert min(top_ks) == 1 and max(top_ks) == 20 and ws.count(0.0) >= 6
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        got = pgvector.search_sessions(ix, q, top_ks, session_masks, citation_weights=ws, bias=bias)
        assert len(got) == nq
        for i in range(nq):
            assert got[i] == pgvector.search(ix, q[i], top_ks[i], citation_weight=ws[i], exact=True, bias=bias, mask=session_masks[i]), i
            assert len(got[i]) == top_ks[i]
        # without the new keywords: what it returned before
        plain = pgvector.search_sessions(ix, q, top_ks, session_masks)
        for i in range(nq):
            assert plain[i] == pgvector.search(ix, q[i], top_ks[i], mask=session_masks[i]), i
