"""The batched search on the general-width matrix kernel (theoremsearch_amd/csrc/kernels_mfma_anyd.h): any row width that is
a multiple of 64 from 128 up to a 4,096-byte row, other than the four hand-laid widths.  Parity with the fp64 oracle as
tests/test_search_gpu.py::check does it, the refused widths, score bits that do not depend on the batch or the grid, exact
ties, masks, the verified threshold, and the handles (subset, view, shards, device queries)."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_common as E
from oracle import oracle

pytestmark = pytest.mark.gpu

GAP = 1e-6        # fp64 gap below which two ranks count as tied
SCORE_TOL = 1e-5
AUTO_LIMIT = 4    # largest batch AUTO still sends to the scan at these widths (anyd_plan.h), k <= 64


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


def pinned_positions(truth, k):
    """[nq x k] bool: positions of the fp64 ranking whose neighbours on both sides are more than GAP away."""
    top = -np.sort(-truth, axis=1)[:, :k + 1]
    gaps = top[:, :-1] - top[:, 1:]
    hi = gaps > GAP
    lo = np.ones_like(hi)
    lo[:, 1:] = hi[:, :-1]
    return lo & hi


# ---- parity ---------------------------------------------------------------------------------------------------------------
PARITY = [("bf16", 128, 16_384, 17, 1, "ip"), ("bf16", 192, 16_385, 40, 10, "cos"), ("bf16", 576, 20_011, 256, 10, "ip"),
          ("bf16", 1088, 20_011, 300, 100, "cos"), ("bf16", 1536, 20_011, 17, 256, "ip"), ("bf16", 2048, 16_384, 33, 100, "ip"),
          ("f32", 128, 20_011, 33, 256, "ip"), ("f32", 192, 16_385, 65, 10, "cos"), ("f32", 640, 20_011, 17, 256, "cos"),
          ("f32", 960, 20_011, 256, 10, "ip")]


@pytest.mark.parametrize("dtype,d,n,nq,k,metric", PARITY, ids=lambda v: str(v))
def test_parity_with_the_oracle(ts, dtype, d, n, nq, k, metric):
    q, c = oracle.inputs(n, nq, d, 7, metric)
    truth = truth_of(q, c, metric, dtype)
    limit = (2 if dtype == "f32" else 1) if k > 64 else AUTO_LIMIT         # k > 64: the scan serves one query per pass
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric=metric) as ix:
        cands = []
        for algo in ("mfma", "auto") if nq > limit else ("mfma", "mfma"):
            scores, idx, st = ix.search(q, k, algo=algo, return_stats=True)
            assert st["algo"] == 2 and st["levels"] == 2 and st["screened"] == 0, (algo, st)
            # Gaussian scores: the estimated threshold holds for every query, and it is the same threshold call after call
            # (a sample kernel that multiplied a register nobody wrote sent whole batches to the exact re-run)
            assert st["fallback_queries"] == 0 and 0 < st["candidates"] <= min(nq, 256) * 8192, (algo, st)
            cands.append(st["candidates"])
            stats = check(truth, k, scores, idx)
            print(algo, "pinned", stats["pinned"], "of", stats["positions"], "fallbacks", st["fallback_queries"], "candidates", st["candidates"])
            assert stats["pinned"] > 0.9 * stats["positions"]
        assert cands[0] == cands[1], cands


# ---- refused ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("bf16", 64), ("f32", 64), ("bf16", 200), ("f32", 200), ("bf16", 2112), ("f32", 1088)])
def test_widths_the_matrix_path_does_not_serve_are_refused(ts, dtype, d):
    q, c = oracle.inputs(16_400, 20, d, 3, "ip")
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        with pytest.raises(ts.TSearchError) as e:
            ix.search(q, 5, algo="mfma")
        assert e.value.code == -5
        _, _, st = ix.search(q, 5, return_stats=True)
        assert st["algo"] == 1


def test_a_served_width_without_the_two_level_search_is_refused(ts):
    q, c = oracle.inputs(16_400, 40, 192, 3, "ip")
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        ix.set_option("TS_MFMA_STAT", 0)
        with pytest.raises(ts.TSearchError) as e:
            ix.search(q, 5, algo="mfma")
        assert e.value.code == -5
        s1, i1, st = ix.search(q, 5, return_stats=True)
        assert st["algo"] == 1
        ix.set_option("TS_MFMA_STAT", None)
        s2, i2, st = ix.search(q, 5, algo="mfma", return_stats=True)
        assert st["algo"] == 2
        check(truth_of(q, c, "ip", "bf16"), 5, s2, i2)


# ---- the same bits whatever the batch and the grid -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("bf16", 576), ("f32", 640)])
def test_scores_do_not_depend_on_the_batch_or_the_grid(ts, dtype, d):
    k = 10
    for n in (20_011, 16_384):
        q, c = oracle.inputs(n, 256, d, 11, "ip")
        with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
            s256, i256, st = ix.search(q, k, algo="mfma", return_stats=True)
            assert st["algo"] == 2
            check(truth_of(q, c, "ip", dtype), k, s256, i256)
            s17, i17 = ix.search(q[:17], k, algo="mfma")
            assert np.array_equal(i17, i256[:17]) and np.array_equal(s17.view(np.uint32), s256[:17].view(np.uint32))
            for grid in (16, 1024):        # 16,384 rows at grid 1,024: workgroups without a tile
                ix.set_option("TS_MFMA_GRID", grid)
                sg, ig = ix.search(q, k, algo="mfma")
                assert np.array_equal(ig, i256) and np.array_equal(sg.view(np.uint32), s256.view(np.uint32)), (n, grid)
                sg, ig = ix.search(q[:17], k, algo="mfma")
                assert np.array_equal(ig, i17) and np.array_equal(sg.view(np.uint32), s17.view(np.uint32)), (n, grid)
            ix.set_option("TS_MFMA_GRID", None)


# ---- AUTO, and agreement with the scan -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("bf16", 576), ("f32", 640)])
def test_small_batches_stay_on_the_scan_and_the_paths_agree(ts, dtype, d):
    n, nq, k = 20_011, 40, 10
    q, c = oracle.inputs(n, nq, d, 12, "cos")
    truth = truth_of(q, c, "cos", dtype)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="cos") as ix:
        s4, i4, st4 = ix.search(q[:4], k, return_stats=True)
        assert st4["algo"] == 1
        check(truth[:4], k, s4, i4)
        # k > 64 (the scan serves one query per pass): two queries take the kernel on bf16, the scan on fp32; three take the kernel
        for nq_wide, want in ((1, 1), (2, 1 if dtype == "f32" else 2), (3, 2)):
            sw, iw, stw = ix.search(q[:nq_wide], 100, return_stats=True)
            assert stw["algo"] == want, (nq_wide, stw)
            check(truth[:nq_wide], 100, sw, iw)
        sm, im, stm = ix.search(q, k, algo="mfma", return_stats=True)
        ss, is_, sts = ix.search(q, k, algo="scan", return_stats=True)
        assert (stm["algo"], sts["algo"]) == (2, 1)
        check(truth, k, sm, im)
        check(truth, k, ss, is_)
        pin = pinned_positions(truth, k)
        assert pin.mean() > 0.9 and np.array_equal(im[pin], is_[pin])


# ---- tiny indexes: the single-level, unthresholded pass --------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33, 100])
def test_tiny_indexes_under_algo_mfma(ts, n):
    d, nq = 192, 20
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


# ---- special rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [("bf16", 576), ("f32", 640)])
def test_nan_rows_are_never_returned(ts, dtype, d):
    rng = np.random.default_rng(9)
    c = rng.standard_normal((300, d), dtype=np.float32)
    c[7, 5] = np.nan
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


# ---- exact ties ------------------------------------------------------------------------------------------------------------
TIE_N = 20_011


@functools.lru_cache(maxsize=4)
def tie_data(metric, d):
    q, c, _ = E.make_corpus(metric, TIE_N, d, 256, 2000 + d + (metric == "cos"))
    t = E.truth(q, c, metric)
    return q, c, t.astype(np.float32), E.canonical_order(t)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("d", [192, 640])
@pytest.mark.parametrize("metric", ["ip", "cos"])
def test_exact_ties_come_back_in_the_canonical_order(ts, metric, d, dtype):
    q, c, t, order = tie_data(metric, d)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric=metric) as ix:
        for nq in (17, 256):
            for k in (10, 256):
                want_s, want_i = E.ref_topk(t[:nq], order[:nq], k)
                s, i, st = ix.search(q[:nq], k, algo="mfma", return_stats=True)
                assert st["algo"] == 2
                bad = np.argwhere(i != want_i)
                assert bad.size == 0, (nq, k, bad[:5].tolist())
                assert np.array_equal(s, want_s), (nq, k)


# ---- masks -----------------------------------------------------------------------------------------------------------------
def test_masked_batches(ts):
    import torch
    from theoremsearch_amd import _ffi
    n, d, nq, k = 40_000, 1536, 40, 10
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
        # the 50 % mask again, resident on the device: the scan
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


# ---- the threshold is verified, not trusted --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["outliers", "light_tail", "shifted"])
def test_estimated_threshold_is_verified_not_trusted(ts, kind):
    rng = np.random.default_rng(44)
    n, d = 60_000, 1536
    c = rng.standard_normal((n, d), dtype=np.float32) * np.float32(1 / np.sqrt(d))
    q = rng.standard_normal((24, d), dtype=np.float32) * np.float32(1 / np.sqrt(d))
    if kind == "outliers":            # 1 % of the rows 20x longer: sample variance inflated, heavy tail
        c[rng.choice(n, n // 100, replace=False)] *= np.float32(20.0)
    elif kind == "light_tail":        # scores bounded: rows are signed unit vectors of 4 coordinates
        c = np.zeros((n, d), np.float32)
        cols = rng.integers(0, d, size=(n, 4))
        c[np.arange(n)[:, None], cols] = rng.choice([-0.5, 0.5], size=(n, 4)).astype(np.float32)
    else:                             # every score shifted far from zero by a common component
        c += q.mean(axis=0) * np.float32(30.0)
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        scores, idx, st = ix.search(q, 10, algo="mfma", return_stats=True)
        assert st["algo"] == 2
        check(truth_of(q, c, "ip", "bf16"), 10, scores, idx)


def test_candidate_overflow_falls_back_exactly(ts):
    rng = np.random.default_rng(10)
    d = 576
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


# ---- handles ---------------------------------------------------------------------------------------------------------------
def test_subset_view_shards_and_device_queries(ts):
    import torch
    from theoremsearch_amd.distributed import Shards
    n, d, k = 60_000, 1536, 10
    q, c = oracle.inputs(n, 256, d, 15, "ip")
    qb = oracle.f32_to_bf16_bits(q)
    qh = oracle.bf16_bits_to_f32(qb)                         # the queries as bf16 holds them: host and device calls see the same values
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        want_s, want_i, st = ix.search(qh, k, algo="mfma", return_stats=True)
        assert st["algo"] == 2
        check(truth_of(qh, c, "ip", "bf16"), k, want_s, want_i)
        # a view
        v = ix.view()
        s, i, st = v.search(qh, k, return_stats=True)
        v.close()
        assert st["algo"] == 2 and np.array_equal(i, want_i) and np.array_equal(s, want_s)
        # a subset that keeps every answer of the first 40 queries and a third of the other rows
        keep = np.zeros(n, bool)
        keep[::3] = True
        keep[want_i[:40].ravel()] = True
        with ix.subset(keep) as sub:
            s, i, st = sub.search(qh[:40], k, algo="mfma", return_stats=True)
            assert st["algo"] == 2 and np.array_equal(i, want_i[:40]) and np.allclose(s, want_s[:40], atol=SCORE_TOL)
        # device-resident queries in the storage dtype: 256 are read in place, 70 go through the prepared copy
        qd = torch.from_numpy(qb.view(np.int16)).cuda()
        for nq in (256, 70):
            out_s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            out_i = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ix.search_device(qd.data_ptr(), "bf16", nq, k, out_s.data_ptr(), out_i.data_ptr(), 0, algo="mfma")
            ix.synchronize()
            assert np.array_equal(out_i.cpu().numpy(), want_i[:nq]) and np.array_equal(out_s.cpu().numpy(), want_s[:nq]), nq
    # three shards on one device (20,000 rows each: above the matrix path's minimum)
    with Shards(n, d, 3, dtype="bf16", metric="ip", devices=[0, 0, 0]) as sh:
        sh.upload(c, 0)
        s, i = sh.search(qh, k)
        assert np.array_equal(i, want_i) and np.allclose(s, want_s, atol=SCORE_TOL)
