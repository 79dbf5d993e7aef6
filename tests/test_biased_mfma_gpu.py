"""The batched citation-weighted search on the matrix path (ts_search_biased_ex; theoremsearch_amd/csrc/kernels_mfma_anyd.h
with the bias term in its epilogue, kernels_sample_biased.h for the threshold): parity with the fp64 oracle under the
citation recipe of tests/test_api_gpu.py's biased test, a cap on the exact re-runs (so that no case passes on the scan
alone), score bits that do not depend on the batch or the grid, masks, exact ties, special bias values, the handles, the
refusals and AUTO."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

W = 0.02
AUTO_LIMIT = {"bf16": 4, "f32": 8}      # largest batch AUTO still sends to the scan (bias_plan.h: bias_scan_max_queries), k <= 64


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


@functools.lru_cache(maxsize=4)
def recipe(n):
    """Citation counts of tests/test_api_gpu.py's biased test: None / 0 / 1..399, twelve rows at 1e6..1e8."""
    from theoremsearch_amd import pgvector
    rng = np.random.default_rng(9)
    cites = [None if u < 0.1 else (0 if u < 0.2 else int(v)) for u, v in zip(rng.random(n), rng.integers(1, 400, n))]
    for r in rng.choice(n, 12, replace=False):
        cites[int(r)] = int(10 ** rng.integers(6, 9))
    return cites, pgvector.citation_bias(cites)


@functools.lru_cache(maxsize=2)
def case_data(dtype, d, n, nq, metric):
    q, c = oracle.inputs(n, nq, d, 300 + d, metric)
    qp, cp = oracle.prepared_inputs(q, c, metric, dtype)
    return q, c, oracle.scores_fp64(qp, cp)


def weighted_topk(sim, bonus, w, k, allowed=None):
    """oracle.citation_weighted_rerank over the whole row (weighted DESC, similarity DESC, row ASC), from the best 4 k + 64."""
    weighted = sim + w * bonus
    rows = np.arange(sim.shape[0]) if allowed is None else allowed
    m = min(rows.shape[0], 4 * k + 64)
    top = rows[np.argpartition(-weighted[rows], m - 1)[:m]] if m < rows.shape[0] else rows
    order = top[np.lexsort((top, -sim[top], -weighted[top]))][:k]
    return order, sim[order], weighted[order]


def check_weighted(sim64, cites, bias, w, k, ws, sims, idx, allowed=None):
    """As test_biased_search_is_the_citation_weighted_ranking_over_all_rows: pinned ranks (fp64 gap > 1e-6 on both sides)
    exact, nothing worse than the k-th best, weighted scores and similarities within 1e-5."""
    bonus = bias.astype(np.float64)
    for b in range(sim64.shape[0]):
        want_i, want_sim, want_w = weighted_topk(sim64[b], bonus, w, k, allowed)
        if b == 0 and allowed is None:       # the helper is the oracle's restatement
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


# ---- parity ---------------------------------------------------------------------------------------------------------------
PARITY = [("bf16", 768, 20_011, 40, 10, "ip"),       # a hand-laid width
          ("f32", 1024, 16_385, 17, 10, "ip"),       # 4,096-byte rows, 32-row tiles
          ("bf16", 192, 20_011, 256, 10, "cos"),     # last k-group of two steps
          ("bf16", 2048, 16_384, 33, 100, "ip"),     # the mean + z sd rule on the weighted scores under-fills every query here
          ("f32", 640, 20_011, 65, 256, "cos")]      # large k, 1,536-candidate target


@pytest.mark.parametrize("dtype,d,n,nq,k,metric", PARITY, ids=lambda v: str(v))
def test_parity_with_the_oracle(ts, dtype, d, n, nq, k, metric):
    """n % 64 of 43 and 1: the bias reads of the last tile are guarded row by row.  fallback_queries <= nq // 8 keeps the
    case from passing on the exact re-run alone (the CPU model of the estimate gives 0 at every one of these shapes)."""
    q, c, sim64 = case_data(dtype, d, n, nq, metric)
    cites, bias = recipe(n)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric=metric) as ix:
        ws, sims, idx, st = ix.search_biased(q, k, bias, W, algo="mfma", return_stats=True)
        print("stats", (dtype, d, n, nq, k), st, "candidates per query", st["candidates"] / nq)
        assert st["algo"] == 2 and st["levels"] == 2 and st["screened"] == 0, st
        assert idx.min() >= 0
        check_weighted(sim64, cites, bias, W, k, ws, sims, idx)
        assert np.intersect1d(idx[0], np.flatnonzero(bias > 10)).size > 0       # the heavily cited rows made it
        assert st["fallback_queries"] <= nq // 8, st
        assert st["candidates"] >= nq * k


def test_one_million_rows(ts):
    """bf16 d = 128, 1,000,003 rows, 64 queries: the CPU model of the estimate gives 41-105 candidates per query."""
    dtype, d, n, nq, k = "bf16", 128, 1_000_003, 64, 10
    q, c, sim64 = case_data(dtype, d, n, nq, "ip")
    cites, bias = recipe(n)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        ws, sims, idx, st = ix.search_biased(q, k, bias, W, algo="mfma", return_stats=True)
        print("stats", (dtype, d, n, nq, k), st, "candidates per query", st["candidates"] / nq)
        assert st["algo"] == 2 and st["levels"] == 2
        check_weighted(sim64, cites, bias, W, k, ws, sims, idx)
        assert st["fallback_queries"] <= nq // 8, st


# ---- the same bits whatever the batch and the grid -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("bf16", 768), ("f32", 640)])
def test_scores_do_not_depend_on_the_batch_or_the_grid(ts, dtype, d):
    n, k = 20_011, 10
    q, c = oracle.inputs(n, 256, d, 11, "ip")
    cites, bias = recipe(n)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        s256, m256, i256, st = ix.search_biased(q, k, bias, W, algo="mfma", return_stats=True)
        assert st["algo"] == 2 and st["fallback_queries"] == 0, st      # (a re-run query would carry the scan's arithmetic)
        s17, m17, i17, st17 = ix.search_biased(q[:17], k, bias, W, algo="mfma", return_stats=True)
        assert st17["algo"] == 2 and st17["fallback_queries"] == 0, st17
        assert np.array_equal(i17, i256[:17]) and np.array_equal(s17.view(np.uint32), s256[:17].view(np.uint32))
        assert np.array_equal(m17.view(np.uint32), m256[:17].view(np.uint32))
        for grid in (16, 1024):
            ix.set_option("TS_MFMA_GRID", grid)
            sg, mg, ig = ix.search_biased(q, k, bias, W, algo="mfma")
            assert np.array_equal(ig, i256) and np.array_equal(sg.view(np.uint32), s256.view(np.uint32)), grid
            assert np.array_equal(mg.view(np.uint32), m256.view(np.uint32)), grid
            sg, mg, ig = ix.search_biased(q[:17], k, bias, W, algo="mfma")
            assert np.array_equal(ig, i17) and np.array_equal(sg.view(np.uint32), s17.view(np.uint32)), grid
            assert np.array_equal(mg.view(np.uint32), m17.view(np.uint32)), grid
        ix.set_option("TS_MFMA_GRID", None)


def test_weight_zero_is_the_plain_matrix_search(ts):
    n, d, nq, k = 20_011, 576, 40, 10
    q, c = oracle.inputs(n, nq, d, 12, "ip")
    cites, bias = recipe(n)
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        p_s, p_i, pst = ix.search(q, k, algo="mfma", return_stats=True)
        z_s, z_sim, z_i, st = ix.search_biased(q, k, bias, 0.0, algo="mfma", return_stats=True)
        assert pst["algo"] == 2 and st["algo"] == 2 and pst["fallback_queries"] == 0 and st["fallback_queries"] == 0
        assert np.array_equal(z_i, p_i) and np.array_equal(z_s.view(np.uint32), p_s.view(np.uint32))
        assert np.array_equal(z_sim.view(np.uint32), p_s.view(np.uint32))


# ---- masks -----------------------------------------------------------------------------------------------------------------
def test_host_masks(ts):
    dtype, d, n, nq, k = "bf16", 768, 20_011, 40, 10
    q, c, sim64 = case_data(dtype, d, n, nq, "ip")
    cites, bias = recipe(n)
    rng = np.random.default_rng(5)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        mask = rng.random(n) < 0.4
        ws, sims, idx, st = ix.search_biased(q, k, bias, W, mask=mask, algo="mfma", return_stats=True)
        print("stats masked", st, "candidates per query", st["candidates"] / nq)
        assert st["algo"] == 2 and st["levels"] == 2 and st["fallback_queries"] <= nq // 8, st
        assert mask[idx].all()
        check_weighted(sim64, cites, bias, W, k, ws, sims, idx, allowed=np.flatnonzero(mask))
        # two allowed rows, k = 5: so sparse a mask is refused under "mfma" (the refusals' test) and AUTO routes it to the scan.
        # This pins AUTO's routing through the new entry; the padding itself is the scan's, not new code
        two = np.zeros(n, bool)
        two[[123, 15_000]] = True
        ws, sims, idx, st = ix.search_biased(q, 5, bias, W, mask=two, algo="auto", return_stats=True)
        assert st["algo"] == 1
        assert (np.sort(idx[:, :2], axis=1) == [123, 15_000]).all()
        assert (idx[:, 2:] == -1).all() and np.isneginf(ws[:, 2:]).all()
        # the next unmasked batch is unaffected
        ws, sims, idx, st = ix.search_biased(q, k, bias, W, algo="mfma", return_stats=True)
        assert st["algo"] == 2
        check_weighted(sim64, cites, bias, W, k, ws, sims, idx)


# ---- exact ties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("bf16", 192), ("f32", 640)])
def test_exact_ties_come_back_in_row_order(ts, dtype, d):
    """Small-integer rows and queries, a bias in halves and w = 0.5: every weighted score is exact in fp32 whatever the order
    of the additions.  500 distinct rows repeated over 20,011, equal rows with equal bias: weighted score descending, then
    row ascending."""
    rng = np.random.default_rng(21)
    n, nq, k, distinct = 20_011, 40, 10, 500
    base = rng.integers(-2, 3, size=(distinct, d)).astype(np.float32)
    base_bias = (rng.integers(0, 9, size=distinct) * 0.5).astype(np.float32)
    which = np.arange(n) % distinct
    c, bias = base[which], base_bias[which]
    q = rng.integers(-1, 2, size=(nq, d)).astype(np.float32)
    weighted = q.astype(np.float64) @ c.T.astype(np.float64) + 0.5 * bias.astype(np.float64)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        for kk in (k, 100):
            ws, sims, idx, st = ix.search_biased(q, kk, bias, 0.5, algo="mfma", return_stats=True)
            assert st["algo"] == 2
            for b in range(nq):
                order = np.lexsort((np.arange(n), -weighted[b]))[:kk]
                assert np.array_equal(idx[b], order), (kk, b)
                assert np.array_equal(ws[b], weighted[b][order].astype(np.float32)), (kk, b)


# ---- special bias values ---------------------------------------------------------------------------------------------------
def test_infinite_and_nan_bias_rows_as_the_scan_ranks_them(ts):
    n, d, nq, k = 20_011, 768, 20, 10
    q, c = oracle.inputs(n, nq, d, 31, "ip")
    cites, bias = recipe(n)
    bias = bias.copy()
    bias[[5, 7_000, 19_999]] = np.inf
    bias[[6, 9_000]] = -np.inf
    bias[[8, 11_000, 20_010]] = np.nan
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        _, _, i_scan = ix.search_biased(q, k, bias, W, algo="scan")
        _, _, i_mfma, st = ix.search_biased(q, k, bias, W, algo="mfma", return_stats=True)
        assert st["algo"] == 2
        assert np.array_equal(i_mfma, i_scan)
        assert (i_mfma[:, :3] == [5, 7_000, 19_999]).all()
        assert not np.isin(i_mfma, [6, 9_000, 8, 11_000, 20_010]).any()


# ---- handles ---------------------------------------------------------------------------------------------------------------
def test_device_buffers_view_and_row_offset(ts):
    import torch
    n, d, k = 20_011, 768, 10
    q, c = oracle.inputs(n, 256, d, 15, "ip")
    qb = oracle.f32_to_bf16_bits(q)
    qh = oracle.bf16_bits_to_f32(qb)                         # the queries as bf16 holds them: host and device calls see the same values
    cites, bias = recipe(n)
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        want_s, want_m, want_i, st = ix.search_biased(qh, k, bias, W, algo="mfma", return_stats=True)
        assert st["algo"] == 2 and st["fallback_queries"] == 0
        # device-resident bias (exactly n floats), queries and outputs: 256 queries are read in place, 70 go through the prepared copy
        bd = torch.from_numpy(bias).cuda()
        qd = torch.from_numpy(qb.view(np.int16)).cuda()
        for nq in (256, 70):
            out_s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            out_m = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            out_i = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ix.search_biased_device(qd.data_ptr(), "bf16", nq, k, bd.data_ptr(), W, out_s.data_ptr(), out_m.data_ptr(), out_i.data_ptr(), 0,
                                    algo="mfma")
            ix.synchronize()
            assert np.array_equal(out_i.cpu().numpy(), want_i[:nq]), nq
            assert np.array_equal(out_s.cpu().numpy(), want_s[:nq]) and np.array_equal(out_m.cpu().numpy(), want_m[:nq]), nq
        # a view
        v = ix.view()
        s, m, i, st = v.search_biased(qh, k, bias, W, algo="auto", return_stats=True)
        v.close()
        assert st["algo"] == 2 and np.array_equal(i, want_i) and np.array_equal(s, want_s) and np.array_equal(m, want_m)
        # the row offset is applied to the ids (and taken off again where the similarities are made)
        ix.set_row_offset(1_000_000)
        s, m, i, st = ix.search_biased(qh, k, bias, W, algo="mfma", return_stats=True)
        ix.set_row_offset(0)
        assert st["algo"] == 2 and np.array_equal(i, want_i + 1_000_000) and np.array_equal(s, want_s) and np.array_equal(m, want_m)


def test_pgvector_search_batch_is_the_exact_form_per_query(ts):
    from theoremsearch_amd import pgvector
    n, d, k = 20_011, 768, 5
    q, c = oracle.inputs(n, 12, d, 77, "ip")
    cites, bias = recipe(n)
    with ts.TheoremIndex.from_embeddings(c, dtype="f32", metric="ip") as ix:
        batch = pgvector.search_batch(ix, q, k, W, citations=cites)
        assert len(batch) == 12
        for b in (0, 5, 11):
            one = pgvector.search(ix, q[b], k, citation_weight=W, citations=cites, exact=True)
            assert [r["row"] for r in batch[b]] == [r["row"] for r in one]
            assert np.allclose([r["score"] for r in batch[b]], [r["score"] for r in one], atol=1e-5)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def refused(ts, call, code=-5):
    with pytest.raises(ts.TSearchError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))


def test_what_the_biased_matrix_search_does_not_serve_is_refused(ts):
    import torch
    from theoremsearch_amd import _ffi
    n, nq, k = 16_400, 20, 5
    rng = np.random.default_rng(3)
    bias = rng.random(n).astype(np.float32)
    q, c = oracle.inputs(n, nq, 192, 3, "ip")
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        ws, _, wi, st = ix.search_biased(q, k, bias, W, algo="mfma", return_stats=True)
        assert st["algo"] == 2
        # a subset index
        with ix.subset(np.arange(0, n, 2)) as sub:
            refused(ts, lambda: sub.search_biased(q, k, bias[::2], W, algo="mfma"))
        # no two-level search
        for knob in ("TS_MFMA_STAT", "TS_MFMA_SAMPLE"):
            ix.set_option(knob, 0)
            refused(ts, lambda: ix.search_biased(q, k, bias, W, algo="mfma"))
            _, _, _, st = ix.search_biased(q, k, bias, W, algo="auto", return_stats=True)
            assert st["algo"] == 1
            ix.set_option(knob, None)
        # a host mask too sparse (5 % of the rows), and a mask in device memory
        sparse = np.zeros(n, bool)
        sparse[rng.choice(n, n // 20, replace=False)] = True
        refused(ts, lambda: ix.search_biased(q, k, bias, W, mask=sparse, algo="mfma"))
        dense = rng.random(n) < 0.5
        words = np.zeros((n + 31) // 32 * 4, dtype=np.uint8)
        bits = np.packbits(dense, bitorder="little")
        words[:bits.shape[0]] = bits
        mdev = torch.from_numpy(words.view(np.int32)).cuda()
        torch.cuda.synchronize()
        out_s, out_m, out_i = np.empty((nq, k), np.float32), np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)

        def device_mask(algo):
            st = _ffi.SearchStats()
            _ffi.check(_ffi.load().ts_search_biased_ex(ix.handle, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, nq, k, _ffi.as_ptr(bias), 0, W,
                                                       C.c_void_p(mdev.data_ptr()), 1, _ffi.as_ptr(out_s), _ffi.as_ptr(out_m),
                                                       _ffi.as_ptr(out_i), 0, None, algo, C.byref(st)))
            return st.algo
        refused(ts, lambda: device_mask(2))
        assert device_mask(0) == 1 and dense[out_i].all()
        # a weight that is not a number
        refused(ts, lambda: ix.search_biased(q, k, bias, float("nan"), algo="mfma"), code=-1)
        # and the served call still answers as before
        ws2, _, wi2 = ix.search_biased(q, k, bias, W, algo="mfma")
        assert np.array_equal(wi2, wi) and np.array_equal(ws2, ws)
    # widths the pass does not serve
    for dtype, d in (("bf16", 64), ("bf16", 200), ("bf16", 2112), ("f32", 1088)):
        q, c = oracle.inputs(n, nq, d, 3, "ip")
        with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
            refused(ts, lambda: ix.search_biased(q, k, bias, W, algo="mfma"))
            _, _, _, st = ix.search_biased(q, k, bias, W, algo="auto", return_stats=True)
            assert st["algo"] == 1
    # an fp32 index with the fp32 matrix kernels switched off
    q, c = oracle.inputs(n, nq, 640, 3, "ip")
    with ts.TheoremIndex.from_embeddings(c, dtype="f32", metric="ip") as ix:
        ix.set_option("TS_MFMA_F32", 0)
        refused(ts, lambda: ix.search_biased(q, k, bias, W, algo="mfma"))
        ix.set_option("TS_MFMA_F32", None)
        _, _, _, st = ix.search_biased(q, k, bias, W, algo="mfma", return_stats=True)
        assert st["algo"] == 2


# ---- AUTO, and the entry without a hint ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("bf16", 768), ("f32", 640)])
def test_auto_and_the_unhinted_entry(ts, dtype, d):
    n, nq, k = 20_011, 40, 10
    q, c, sim64 = case_data(dtype, d, n, nq, "ip")
    cites, bias = recipe(n)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        for batch, want in ((1, 1), (AUTO_LIMIT[dtype], 1), (AUTO_LIMIT[dtype] + 1, 2), (nq, 2)):
            ws, sims, idx, st = ix.search_biased(q[:batch], k, bias, W, algo="auto", return_stats=True)
            assert st["algo"] == want, (batch, st)
            check_weighted(sim64[:batch], cites, bias, W, k, ws, sims, idx)
        for batch, want in ((1, 1), (2, 2)):                 # k > 64: the scan serves one query per pass
            _, _, _, st = ix.search_biased(q[:batch], 100, bias, W, algo="auto", return_stats=True)
            assert st["algo"] == want, (batch, st)
        # no hint: ts_search_biased, which is the scan bit for bit
        u = ix.search_biased(q, k, bias, W)
        s = ix.search_biased(q, k, bias, W, algo="scan", return_stats=True)
        assert s[3]["algo"] == 1 and s[3]["levels"] == 0
        for a, b in zip(u, s[:3]):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
