"""The batched search on the k-chunked matrix kernel (theoremsearch_amd/csrc/kernels_mfma_wide.h, kernels_sample_wide.h): row
widths that are a multiple of 256 with a row of more than 4,096 and at most 16,384 bytes (bf16 d = 2,304 .. 8,192, fp32
d = 1,280 .. 4,096).  Exact block markers (a dropped, doubled, misplaced or stale k-chunk changes an integer score), parity
with the fp64 oracle through the two-level search, score bits that do not depend on the batch or the grid, the refused
widths and AUTO's routing, tiny indexes, NaN rows, masks, the verified threshold, the biased search, and the handles.
The helpers and what they promise without a GPU: tests/wide_common.py, tests/test_wide_common_cpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import wide_common as WC
from oracle import oracle

pytestmark = pytest.mark.gpu

GAP, SCORE_TOL = WC.GAP, WC.SCORE_TOL
AUTO_LIMIT = {"bf16": 4, "f32": 8}      # largest batch AUTO still sends to the scan at these widths (wide_plan.h: wide_scan_max_queries), k <= 64
W = 0.02          # the citation weight of tests/test_biased_mfma_gpu.py


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


def truth_of(q, c, metric, dtype):
    qp, cp = oracle.prepared_inputs(q, c, metric, dtype)
    return oracle.scores_fp64(qp, cp)


def check(truth, k, scores, idx):
    stats = oracle.check_topk_against_truth(truth, idx, scores, k, gap=GAP, score_tol=SCORE_TOL)
    assert stats["recall"] == 1.0
    return stats


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def k_limit(dtype, k):
    """wide_plan.h: wide_scan_limit."""
    return (2 if dtype == "f32" else 1) if k > 64 else AUTO_LIMIT[dtype]


# ---- 1. exact block markers ------------------------------------------------------------------------------------------------
MARKERS = [(dtype, d) for dtype in ("bf16", "f32") for d in WC.MARKER_WIDTHS[dtype]]


@functools.lru_cache(maxsize=2)
def marker(d):
    return WC.marker_corpus(d)


@pytest.mark.parametrize("dtype,d", MARKERS, ids=lambda v: str(v))
def test_block_markers_come_back_exact(ts, dtype, d):
    """3 d / 64 + 1 rows: the only level of the search is the whole kernel, every k-chunk of it, unthresholded.  Both forms of
    the chunk loop (one barrier a chunk, and the plain two-barrier one) give the integers."""
    q, c, exact = marker(d)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        for serial in (None, 1):
            ix.set_option("TS_MFMA_WIDE_SERIAL", serial)
            for grid in (None, 16, 1024):
                ix.set_option("TS_MFMA_GRID", grid)
                for nq in (17, 256):
                    for k in (10, 256):
                        want_s, want_i = WC.canonical_topk(exact[:nq], k)
                        s, i, st = ix.search(q[:nq], k, algo="mfma", return_stats=True)
                        assert st["algo"] == 2 and st["levels"] == 1, st
                        bad = np.argwhere(i != want_i)
                        assert bad.size == 0, (serial, grid, nq, k, bad[:5].tolist())
                        assert same_bits(s, want_s), (serial, grid, nq, k)
            ix.set_option("TS_MFMA_GRID", None)


# ---- 2. parity through the two-level search --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d,n,nq,k,metric", WC.PARITY, ids=lambda v: str(v))
def test_parity_with_the_oracle(ts, dtype, d, n, nq, k, metric):
    q, c = oracle.inputs(n, nq, d, WC.PARITY_SEED, metric)
    truth = truth_of(q, c, metric, dtype)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric=metric) as ix:
        cands = []
        for algo in ("mfma", "auto"):
            assert nq > k_limit(dtype, k)
            scores, idx, st = ix.search(q, k, algo=algo, return_stats=True)
            assert st["algo"] == 2 and st["levels"] == 2 and st["screened"] == 0, (algo, st)
            assert st["fallback_queries"] == 0 and 0 < st["candidates"] <= min(nq, 256) * 8192, (algo, st)
            cands.append(st["candidates"])
            stats = check(truth, k, scores, idx)
            print(algo, "pinned", stats["pinned"], "of", stats["positions"], "fallbacks", st["fallback_queries"], "candidates", st["candidates"])
            assert stats["pinned"] > 0.9 * stats["positions"]
        assert cands[0] == cands[1], cands


# ---- 3. the same bits whatever the batch and the grid ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("bf16", 2560), ("f32", 1536)])
def test_scores_do_not_depend_on_the_batch_or_the_grid(ts, dtype, d):
    k = 10
    for n in (20_011, 16_384):
        q, c = oracle.inputs(n, 256, d, 11, "ip")
        with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
            s256, i256, st = ix.search(q, k, algo="mfma", return_stats=True)
            assert st["algo"] == 2 and st["levels"] == 2
            check(truth_of(q, c, "ip", dtype), k, s256, i256)
            s17, i17 = ix.search(q[:17], k, algo="mfma")
            assert np.array_equal(i17, i256[:17]) and same_bits(s17, s256[:17])
            for grid in (16, 1024):        # 16,384 rows at grid 1,024: workgroups without a tile
                ix.set_option("TS_MFMA_GRID", grid)
                sg, ig = ix.search(q, k, algo="mfma")
                assert np.array_equal(ig, i256) and same_bits(sg, s256), (n, grid)
                sg, ig = ix.search(q[:17], k, algo="mfma")
                assert np.array_equal(ig, i17) and same_bits(sg, s17), (n, grid)
            ix.set_option("TS_MFMA_GRID", None)


# ---- 4. refusals and routing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("bf16", 2112), ("bf16", 2176), ("bf16", 8448), ("f32", 1088), ("f32", 1344), ("f32", 4352)])
def test_widths_the_matrix_path_does_not_serve_are_refused(ts, dtype, d):
    rng = np.random.default_rng(3)
    c = rng.standard_normal((16_400, d), dtype=np.float32)
    q = rng.standard_normal((20, d), dtype=np.float32)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        with pytest.raises(ts.TSearchError) as e:
            ix.search(q, 5, algo="mfma")
        assert e.value.code == -5
        _, _, st = ix.search(q, 5, return_stats=True)
        assert st["algo"] == 1


@pytest.mark.parametrize("dtype,d,knob", [("bf16", 2560, "TS_MFMA_STAT"), ("f32", 1536, "TS_MFMA_STAT"), ("f32", 1536, "TS_MFMA_F32")])
def test_a_served_width_with_its_condition_switched_off_is_refused(ts, dtype, d, knob):
    q, c = oracle.inputs(16_400, 40, d, 3, "ip")
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        ix.set_option(knob, 0)
        with pytest.raises(ts.TSearchError) as e:
            ix.search(q, 5, algo="mfma")
        assert e.value.code == -5
        _, _, st = ix.search(q, 5, return_stats=True)
        assert st["algo"] == 1
        ix.set_option(knob, None)
        s2, i2, st = ix.search(q, 5, algo="mfma", return_stats=True)
        assert st["algo"] == 2
        check(truth_of(q, c, "ip", dtype), 5, s2, i2)


@pytest.mark.parametrize("dtype,d", [("bf16", 2560), ("f32", 1536)])
def test_small_batches_stay_on_the_scan_and_the_paths_agree(ts, dtype, d):
    n, nq, k = 20_011, 40, 10
    q, c = oracle.inputs(n, nq, d, 12, "cos")
    truth = truth_of(q, c, "cos", dtype)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="cos") as ix:
        auto = AUTO_LIMIT[dtype]
        for batch, want in ((auto, 1), (auto + 1, 2)):
            sb, ib, stb = ix.search(q[:batch], k, return_stats=True)
            assert stb["algo"] == want, (batch, stb)
            check(truth[:batch], k, sb, ib)
        # k = 100 (the scan serves one query per pass): wide_scan_limit
        limit = k_limit(dtype, 100)
        for batch in (1, 2, 3):
            sw, iw, stw = ix.search(q[:batch], 100, return_stats=True)
            assert stw["algo"] == (1 if batch <= limit else 2), (batch, stw)
            check(truth[:batch], 100, sw, iw)
        sm, im, stm = ix.search(q, k, algo="mfma", return_stats=True)
        ss, is_, sts = ix.search(q, k, algo="scan", return_stats=True)
        assert (stm["algo"], sts["algo"]) == (2, 1)
        check(truth, k, sm, im)
        check(truth, k, ss, is_)
        pin = WC.pinned_positions(truth, k)
        assert pin.mean() > 0.9 and np.array_equal(im[pin], is_[pin])
        s4, i4 = ix.search(q[:auto], k)                             # the scan's batch against the matrix answer
        assert np.array_equal(i4[pin[:auto]], im[:auto][pin[:auto]])


# ---- 5. tiny indexes: the single-level, unthresholded pass -----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33, 100])
def test_tiny_indexes_under_algo_mfma(ts, n):
    d, nq = 2560, 20
    q, c = oracle.inputs(n, nq, d, 13, "ip")
    truth = truth_of(q, c, "ip", "bf16")
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        for k in (1, 10, 256):
            scores, idx, st = ix.search(q, k, algo="mfma", return_stats=True)
            assert st["algo"] == 2 and st["levels"] == 1
            m = min(k, n)
            assert (idx[:, m:] == -1).all() and np.isneginf(scores[:, m:]).all()
            assert ((idx[:, :m] >= 0) & (idx[:, :m] < n)).all()
            check(truth, k, scores, idx)


# ---- 6. special rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("bf16", 2560), ("f32", 1536)])
def test_nan_rows_are_never_returned(ts, dtype, d):
    rng = np.random.default_rng(9)
    c = rng.standard_normal((300, d), dtype=np.float32)
    c[7, d - 5] = np.nan              # in the last k-chunk
    c[200, :] = np.nan
    c[100, :] = 0
    c[299, :] = 0
    q = rng.standard_normal((20, d), dtype=np.float32)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        for algo in ("scan", "mfma"):
            scores, idx = ix.search(q, 256, algo=algo)
            assert 7 not in idx and 200 not in idx
            assert not np.isnan(scores).any()
            want_s, want_i = oracle.search(q, c, 256, "ip", dtype)
            for b in range(q.shape[0]):
                assert set(idx[b].tolist()) == set(want_i[b].tolist()), (algo, b)


# ---- 7. masks --------------------------------------------------------------------------------------------------------------
def test_masked_batches(ts):
    import torch
    from theoremsearch_amd import _ffi
    n, d, nq, k = 40_000, 2560, 40, 10
    q, c = oracle.inputs(n, nq, d, 14, "cos")
    rng = np.random.default_rng(6)
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="cos") as ix:
        def verify(mask, scores, idx):
            allowed = np.flatnonzero(mask)
            assert mask[idx].all()
            truth = truth_of(q, c[allowed], "cos", "bf16")
            check(truth, k, scores, np.searchsorted(allowed, idx))

        for frac, algo in ((0.5, 2), (0.1, 2), (0.05, 1)):
            mask = np.zeros(n, bool)
            mask[rng.choice(n, int(n * frac), replace=False)] = True       # exactly this share of the rows
            scores, idx, st = ix.search(q, k, mask=mask, return_stats=True)
            assert st["algo"] == algo, (frac, st)
            verify(mask, scores, idx)
        # the 50 % mask again, resident on the device (no count comes with it): the scan
        mask = rng.random(n) < 0.5
        words = np.zeros((n + 31) // 32 * 4, dtype=np.uint8)
        bits = np.packbits(mask, bitorder="little")
        words[:bits.shape[0]] = bits
        mdev = torch.from_numpy(words.view(np.int32)).cuda()
        torch.cuda.synchronize()
        scores = np.empty((nq, k), np.float32)
        idx = np.empty((nq, k), np.int64)
        st = _ffi.SearchStats()
        _ffi.check(_ffi.load().ts_search_filtered_ex(ix.handle, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, nq, k, C.c_void_p(mdev.data_ptr()), 1,
                                                     _ffi.as_ptr(scores), _ffi.as_ptr(idx), 0, None, 0, C.byref(st)))
        assert st.algo == 1
        verify(mask, scores, idx)
        s_un, i_un, st = ix.search(q, k, return_stats=True)          # the next unfiltered batch is unaffected
        assert st["algo"] == 2
        check(truth_of(q, c, "cos", "bf16"), k, s_un, i_un)


# ---- 8. the threshold is verified, not trusted -----------------------------------------------------------------------------
def test_candidate_overflow_falls_back_exactly(ts):
    rng = np.random.default_rng(10)
    d = 2560
    c = rng.standard_normal((60_000, d), dtype=np.float32) * np.float32(0.05)
    hot = rng.standard_normal(d).astype(np.float32)
    rows = rng.choice(60_000, size=20_000, replace=False)
    c[rows] = hot
    q = np.stack([hot, rng.standard_normal(d).astype(np.float32)])
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="cos") as ix:
        scores, idx, st = ix.search(q, 10, algo="mfma", return_stats=True)
        assert st["algo"] == 2 and st["fallback_queries"] >= 1
        assert idx[0].tolist() == sorted(rows.tolist())[:10]
        check(truth_of(q, c, "cos", "bf16"), 10, scores, idx)


# ---- 9. the biased search --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def recipe(n):
    """Citation counts of tests/test_biased_mfma_gpu.py: None / 0 / 1..399, twelve rows at 1e6..1e8."""
    from theoremsearch_amd import pgvector
    rng = np.random.default_rng(9)
    cites = [None if u < 0.1 else (0 if u < 0.2 else int(v)) for u, v in zip(rng.random(n), rng.integers(1, 400, n))]
    for r in rng.choice(n, 12, replace=False):
        cites[int(r)] = int(10 ** rng.integers(6, 9))
    return cites, pgvector.citation_bias(cites)


def weighted_topk(sim, bonus, w, k):
    """oracle.citation_weighted_rerank over the whole row (weighted DESC, similarity DESC, row ASC), from the best 4 k + 64."""
    weighted = sim + w * bonus
    m = min(sim.shape[0], 4 * k + 64)
    top = np.argpartition(-weighted, m - 1)[:m] if m < sim.shape[0] else np.arange(sim.shape[0])
    order = top[np.lexsort((top, -sim[top], -weighted[top]))][:k]
    return order, sim[order], weighted[order]


def check_weighted(sim64, cites, bias, w, k, ws, sims, idx):
    """tests/test_biased_mfma_gpu.py's check and tolerances: pinned ranks (fp64 gap > 1e-6 on both sides) exact, nothing worse
    than the k-th best, weighted scores and similarities within 1e-5."""
    bonus = bias.astype(np.float64)
    for b in range(sim64.shape[0]):
        want_i, want_sim, want_w = weighted_topk(sim64[b], bonus, w, k)
        if b == 0:       # the helper is the oracle's restatement
            o_i, o_sim, o_w = oracle.citation_weighted_rerank(np.arange(sim64.shape[1]), sim64[b], cites, w, k)
            assert np.array_equal(o_i, want_i) and np.allclose(o_w, want_w, atol=1e-12)
        got_w = (sim64[b] + w * bonus)[idx[b]]
        gaps = want_w[:-1] - want_w[1:]
        for r in range(k):
            lo = gaps[r - 1] if r else np.inf
            hi = gaps[r] if r < k - 1 else np.inf
            if lo > 1e-6 and hi > 1e-6 and r < k - 1:
                assert idx[b, r] == want_i[r], (b, r)
        assert np.all(got_w >= want_w[-1] - 1e-6), b
        assert np.allclose(ws[b], want_w, atol=1e-5) and np.allclose(sims[b], sim64[b][idx[b]], atol=1e-5), b


@pytest.mark.parametrize("dtype,d", [("bf16", 2560), ("f32", 1536)])
def test_biased_search_on_the_matrix_path(ts, dtype, d):
    n, nq, k = 16_385, 40, 10
    q, c = oracle.inputs(n, nq, d, 300 + d, "ip")
    sim64 = truth_of(q, c, "ip", dtype)
    cites, bias = recipe(n)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        ws, sims, idx, st = ix.search_biased(q, k, bias, W, algo="mfma", return_stats=True)
        print("stats", (dtype, d), st, "candidates per query", st["candidates"] / nq)
        assert st["algo"] == 2 and st["levels"] == 2 and st["screened"] == 0, st
        assert idx.min() >= 0
        check_weighted(sim64, cites, bias, W, k, ws, sims, idx)
        assert st["fallback_queries"] <= nq // 8, st
        _, _, _, st = ix.search_biased(q, k, bias, W, algo="auto", return_stats=True)
        assert st["algo"] == 2
        # algo = scan is ts_search_biased bit for bit
        u = ix.search_biased(q, k, bias, W)
        s = ix.search_biased(q, k, bias, W, algo="scan", return_stats=True)
        assert s[3]["algo"] == 1
        for a, b in zip(u, s[:3]):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize("dtype,d", MARKERS, ids=lambda v: str(v))
def test_biased_block_markers_come_back_exact(ts, dtype, d):
    """The marker corpus with an integer bias and w = 1: every weighted score is an integer, exact in fp32."""
    q, c, exact = marker(d)
    n = c.shape[0]
    bias = ((np.arange(n) * 7) % 23 - 11).astype(np.float32)
    weighted = exact + bias.astype(np.int64)[None, :]
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        for nq in (17, 256):
            for k in (10, 256):
                want_s, want_i = WC.canonical_topk(weighted[:nq], k)
                ws, sims, idx, st = ix.search_biased(q[:nq], k, bias, 1.0, algo="mfma", return_stats=True)
                assert st["algo"] == 2 and st["levels"] == 1, st
                bad = np.argwhere(idx != want_i)
                assert bad.size == 0, (nq, k, bad[:5].tolist())
                assert same_bits(ws, want_s), (nq, k)
                m = min(k, n)
                assert np.array_equal(sims[:, :m], np.take_along_axis(exact[:nq], want_i[:, :m], axis=1).astype(np.float32)), (nq, k)


# ---- 10. handles -----------------------------------------------------------------------------------------------------------
def test_view_and_subset(ts):
    n, d, k = 40_000, 2560, 10
    q, c = oracle.inputs(n, 64, d, 15, "ip")
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        want_s, want_i, st = ix.search(q, k, algo="mfma", return_stats=True)
        assert st["algo"] == 2
        check(truth_of(q, c, "ip", "bf16"), k, want_s, want_i)
        v = ix.view()
        s, i, st = v.search(q, k, return_stats=True)
        v.close()
        assert st["algo"] == 2 and np.array_equal(i, want_i) and np.array_equal(s, want_s)
        # a subset that keeps every answer of the first 40 queries and half of the other rows
        keep = np.zeros(n, bool)
        keep[::2] = True
        keep[want_i[:40].ravel()] = True
        with ix.subset(keep) as sub:
            s, i, st = sub.search(q[:40], k, algo="mfma", return_stats=True)
            assert st["algo"] == 2 and np.array_equal(i, want_i[:40]) and np.allclose(s, want_s[:40], atol=SCORE_TOL)
