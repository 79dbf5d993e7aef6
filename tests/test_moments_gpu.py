"""Moments of the stored rows on the device (ts_index_moments, ts_index_group_sums; theoremsearch_amd/csrc/kernels_moments.h)
and the PCA built on them (theoremsearch_amd/pca.py).  The truth is numpy in int64 / fp64 over `index.download()`, the stored
values.  Integer-valued rows make every partial sum exact, so those cases compare bits; Gaussian rows are held to the derived
bound (L + 2) 2^-23 sum_r |x_ri x_rj| (include/tsearch.h), L read from ts_moments_plan."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NULL = -2 ** 31


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


@functools.lru_cache(maxsize=None)
def flush_rows():
    from theoremsearch_amd import _ffi
    L = C.c_int32(0)
    _ffi.check(_ffi.load().ts_moments_plan(_ffi.TS_BF16, 768, 1, 256, C.byref(L), None, None, None))
    return L.value


def stored(ix):
    """the stored rows as float64"""
    r = ix.download()
    if r.dtype == np.uint16:
        r = (r.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return r.astype(np.float64)


@functools.lru_cache(maxsize=None)
def small_ints(n, d):
    x = np.random.default_rng(1000 * d + n).integers(-2, 3, size=(n, d)).astype(np.float32)
    x.setflags(write=False)
    return x


def exact_truth(xi):
    """count, column sums and Gram matrix in int64 (the products through fp64, exact for these small integers: every sum stays
    far below 2^53)"""
    xf = xi.astype(np.float64)
    return xi.shape[0], xi.astype(np.int64).sum(axis=0), np.rint(xf.T @ xf).astype(np.int64)


def assert_exact(got, xi):
    n, s, g = exact_truth(xi)
    cnt, gs, gg = got
    bad = np.argwhere(gg != g)
    print(f"count {cnt} / {n}, sum mismatches {int((gs != s).sum())}, gram mismatches {len(bad)}{' first ' + str(bad[:4].tolist()) if len(bad) else ''}")
    assert cnt == n and np.array_equal(gs, s) and np.array_equal(gg, g)


# ---- exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("d", [128, 192, 768, 1024])
@pytest.mark.parametrize("n", [1, 33, 257, "L+33"])
def test_integer_rows_give_the_int64_moments_exactly(ts, dtype, d, n):
    """d = 128: one diagonal panel pair; 192: an odd panel count with a ragged last pair; n = L + 33 is more than one flush
    interval and spans several row ranges (a flush in the MIDDLE of a range needs more rows: the next test)."""
    n = flush_rows() + 33 if n == "L+33" else n
    x = small_ints(n, d)
    with ts.TheoremIndex.from_embeddings(x, dtype=dtype, metric="ip") as ix:
        assert np.array_equal(stored(ix), x)
        assert_exact(ix.moments(), x)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_a_row_range_longer_than_L_flushes_in_the_middle(ts, dtype):
    """At d = 1024 the device's CUs get few row ranges (36 panel pairs each); with more than ranges x L rows every workgroup adds
    its accumulators into its partial tile at least once before the end of its range.  The sizes come from ts_moments_plan."""
    from theoremsearch_amd import _ffi
    d, L = 1024, flush_rows()
    cus = _ffi.device_info(0)["compute_units"]
    ranges = C.c_int32(0)
    _ffi.check(_ffi.load().ts_moments_plan(_ffi.TS_BF16, d, 1 << 30, cus, None, None, C.byref(ranges), None))
    n = ranges.value * L + 33
    _ffi.check(_ffi.load().ts_moments_plan(_ffi.TS_BF16, d, n, cus, None, None, C.byref(ranges), None))
    assert n > ranges.value * L and n * d * 4 < 1 << 30, (n, ranges.value)
    x = small_ints(n, d)
    with ts.TheoremIndex.from_embeddings(x, dtype=dtype, metric="ip") as ix:
        assert_exact(ix.moments(), x)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_views_and_subsets_are_served(ts, dtype):
    x = small_ints(257, 192)
    keep = np.arange(0, 257, 3)
    with ts.TheoremIndex.from_embeddings(x, dtype=dtype, metric="ip") as ix:
        with ix.view() as v:
            assert_exact(v.moments(), x)
        with ix.subset(keep) as sub:
            assert_exact(sub.moments(), x[keep])


# ---- bound ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("d", [768, 1024])
def test_gaussian_rows_stay_inside_the_derived_bound(ts, dtype, d):
    """|G_ij - G64_ij| <= (L + 2) 2^-23 sum_r |x_ri x_rj| for every entry, and the same form for the sums: the first-order bound of
    an fp32 chain of L terms in any order, doubled (bf16 products are exact in fp32, an fp32 product adds one rounding)."""
    L = flush_rows()
    n = 2 * L + 77
    x = np.random.default_rng(d).normal(size=(n, d)).astype(np.float32)
    with ts.TheoremIndex.from_embeddings(x, dtype=dtype, metric="cos") as ix:
        cnt, s, g = ix.moments()
        x64 = stored(ix)
    assert abs(np.linalg.norm(x64[5]) - 1) < 1e-2                    # normalised rows
    f = (L + 2) * 2.0 ** -23
    ax = np.abs(x64)
    g_err, g_bound = np.abs(g - x64.T @ x64), f * (ax.T @ ax)
    s_err, s_bound = np.abs(s - x64.sum(axis=0)), f * ax.sum(axis=0)
    print(f"gram: worst error / bound {np.max(g_err / g_bound):.3e}, sums: {np.max(s_err / s_bound):.3e}")
    assert cnt == n
    assert np.all(g_err <= g_bound)
    assert np.all(s_err <= s_bound)


# ---- excluded rows -------------------------------------------------------------------------------------------------
def flag_table(ts, flags):
    return ts.MetaTable.from_columns([np.asarray(flags, dtype=np.int32)])


def allow_ones(ts_mod):
    from theoremsearch_amd.metadata import Atom, RANGE
    return [Atom(RANGE, 0, 1, 1)]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_disallowed_rows_contribute_nothing_whatever_they_hold(ts, dtype):
    n, d = 1000, 192
    rng = np.random.default_rng(5)
    x = small_ints(n, d).copy()
    allow = rng.random(n) < 0.5
    allow[[7, 500, 999]] = False
    x[7] = np.nan
    x[500, 3] = np.inf
    x[999] = np.nan                                                    # the last row: beside the padding
    with ts.TheoremIndex.from_embeddings(x, dtype=dtype, metric="ip") as ix, flag_table(ts, allow) as table:
        with table.eval(allow_ones(ts)) as rs:
            assert rs.allowed == allow.sum()
            got = ix.moments(rowset=rs)
            assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
            assert_exact(got, x[allow])
        # allowed non-finite rows propagate as in numpy
        cnt, s, g = ix.moments()
        with np.errstate(invalid="ignore"):
            want_nan = np.isnan(x.astype(np.float64).sum(axis=0))
        assert cnt == n and np.array_equal(np.isnan(s), want_nan) and np.isnan(g).all()
        with table.eval([]) as everything, flag_table(ts, np.zeros(n)) as none_table:
            assert everything.allowed == n
            with none_table.eval(allow_ones(ts)) as nothing:
                cnt, s, g = ix.moments(rowset=nothing)
                assert cnt == 0 and not s.any() and not g.any()
                names, counts, sums = ix.group_sums(none_table, 0, rowset=nothing, ngroups=3)
                assert not counts.any() and not sums.any()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_nan_in_the_padding_of_an_attached_buffer_is_never_read_as_data(ts, dtype):
    import torch
    n, d = 300, 256
    cap = 512
    x = small_ints(n, d)
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    dev = torch.full((cap, d), float("nan"), dtype=tdt, device="cuda")
    dev[:n] = torch.from_numpy(x.copy()).cuda().to(tdt)
    torch.cuda.synchronize()
    with ts.TheoremIndex(n, d, dtype=dtype, metric="ip") as ix:
        ix.attach_device(dev.data_ptr(), cap, keep_alive=dev)
        got = ix.moments()
        assert np.isfinite(got[2]).all()
        assert_exact(got, x)


# ---- bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_same_bits_on_every_call_and_a_symmetric_gram(ts, dtype):
    n, d = flush_rows() + 500, 320
    x = np.random.default_rng(9).normal(size=(n, d)).astype(np.float32)
    with ts.TheoremIndex.from_embeddings(x, dtype=dtype, metric="ip") as ix:
        c1, s1, g1 = ix.moments()
        c2, s2, g2 = ix.moments()
        c3, s3, g3 = ix.moments(gram=None)
    assert c1 == c2 == c3 == n
    assert s1.tobytes() == s2.tobytes() == s3.tobytes() and g1.tobytes() == g2.tobytes()
    assert g3 is None
    assert np.array_equal(g1.view(np.uint64), g1.T.view(np.uint64))
    assert np.abs(g1).max() > 0


# ---- groups --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("ngroups", [1, 17, 40])
def test_group_sums_equal_add_at_in_int64(ts, dtype, ngroups):
    from theoremsearch_amd.metadata import Atom, RANGE
    n, d = 1500, 192
    rng = np.random.default_rng(ngroups)
    x = small_ints(n, d)
    codes = rng.integers(0, ngroups, size=n).astype(np.int32)
    empty = ngroups // 2
    if ngroups > 1:
        codes[codes == empty] = (empty + 1) % ngroups                # one group without a row
    codes[[0, 31, 64]] = NULL
    codes[[1, 33, 1499]] = -1
    codes[[2, 65, 700]] = ngroups
    allow = (rng.random(n) < 0.5).astype(np.int32)
    with ts.TheoremIndex.from_embeddings(x, dtype=dtype, metric="ip") as ix, ts.MetaTable.from_columns([codes, allow]) as table:
        for rs in (None, table.eval([Atom(RANGE, 1, 1, 1)])):
            sel = (codes >= 0) & (codes < ngroups) & (np.ones(n, bool) if rs is None else allow.astype(bool))
            names, counts, sums = ix.group_sums(table, 0, rowset=rs, ngroups=ngroups)
            want_sums, want_counts = np.zeros((ngroups, d), np.int64), np.zeros(ngroups, np.int64)
            np.add.at(want_sums, codes[sel], x[sel].astype(np.int64))
            np.add.at(want_counts, codes[sel], 1)
            print(f"rowset {rs is not None}: counts {counts.tolist()[:8]} sum mismatches {int((sums != want_sums).sum())}")
            assert names == list(range(ngroups))
            assert np.array_equal(counts, want_counts) and np.array_equal(sums, want_sums)
            assert counts.sum() == sel.sum()
            if ngroups > 1:
                assert counts[empty] == 0 and not sums[empty].any()
            if rs is not None:
                rs.close()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_rows_whose_code_goes_nowhere_contribute_nothing_whatever_they_hold(ts, dtype):
    n, d, ngroups = 300, 128, 5
    x = small_ints(n, d).copy()
    codes = (np.arange(n) % ngroups).astype(np.int32)
    for row, code in ((3, NULL), (70, -1), (299, ngroups), (150, 2 ** 31 - 1)):
        x[row] = np.nan
        codes[row] = code
    with ts.TheoremIndex.from_embeddings(x, dtype=dtype, metric="ip") as ix, ts.MetaTable.from_columns([codes]) as table:
        names, counts, sums = ix.group_sums(table, 0, ngroups=ngroups)
    sel = (codes >= 0) & (codes < ngroups)
    want = np.zeros((ngroups, d), np.int64)
    np.add.at(want, codes[sel], x[sel].astype(np.int64))
    assert np.isfinite(sums).all() and np.array_equal(sums, want) and counts.sum() == sel.sum() == n - 4


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_carry_a_status_and_a_message(ts):
    from theoremsearch_amd import _ffi
    from theoremsearch_amd.metadata import Atom, RANGE
    for d in (64, 1088, 2048):
        with ts.TheoremIndex.from_embeddings(np.ones((10, d), np.float32), dtype="bf16", metric="ip") as ix:
            with pytest.raises(_ffi.TSearchError) as e:
                ix.moments()
            assert e.value.code == -5 and "no kernel" in str(e.value), d
            with ts.MetaTable.from_columns([np.zeros(10, np.int32)]) as t, pytest.raises(_ffi.TSearchError) as e:
                ix.group_sums(t, 0)
            assert e.value.code == -5 and "no kernel" in str(e.value), d
    x = small_ints(257, 128)
    offsets = np.arange(258, dtype=np.int64)
    with ts.TheoremIndex.from_embeddings(x, dtype="f32", metric="ip") as ix:
        with ts.MetaTable.from_columns([np.zeros(257, np.int32), (offsets, np.zeros(257, np.int32))]) as t:
            with pytest.raises(_ffi.TSearchError) as e:
                ix.group_sums(t, 1, ngroups=2)
            assert e.value.code == -1 and "list column" in str(e.value)
            for g in (0, 257):
                with pytest.raises(_ffi.TSearchError) as e:
                    ix.group_sums(t, 0, ngroups=g)
                assert e.value.code == -5 and "ngroups" in str(e.value)
        with ts.MetaTable.from_columns([np.ones(100, np.int32)]) as other:
            with pytest.raises(_ffi.TSearchError) as e:
                ix.group_sums(other, 0)
            assert e.value.code == -1 and "100 rows" in str(e.value)
            with other.eval([Atom(RANGE, 0, 1, 1)]) as rs, pytest.raises(_ffi.TSearchError) as e:
                ix.moments(rowset=rs)
            assert e.value.code == -1 and "the row set has 100 rows, the index 257" in str(e.value)
        lib = _ffi.load()
        cnt = C.c_int64(0)
        assert lib.ts_index_moments(ix.handle, None, C.byref(cnt), None, None, None) == -1


def test_a_meta_table_on_another_device_is_refused(ts):
    from theoremsearch_amd import _ffi
    if _ffi.device_count() < 2:
        pytest.skip("needs two GPUs")
    x = small_ints(257, 128)
    with ts.TheoremIndex.from_embeddings(x, dtype="f32", metric="ip") as ix, ts.MetaTable.from_columns([np.zeros(257, np.int32)], device=1) as t:
        with pytest.raises(_ffi.TSearchError) as e:
            ix.group_sums(t, 0)
        assert e.value.code == -1 and "device" in str(e.value)


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_pca_and_category_means_of_planted_clusters(ts):
    """5,000 x 768 bf16 rows around six centres in one plane; the centres of math.AG and math.NT are the closest pair by far.
    The means come from group sums, so they must agree with numpy fp64 on the downloaded rows within the bound on the sums,
    carried through the linear map (sum_j |V_kj| bound_cj / count_c) plus the rounding of M to float32."""
    from theoremsearch_amd import pca
    n, d = 5000, 768
    rng = np.random.default_rng(42)
    cats = ["math.AG", "math.NT", "math.CO", "math.AP", "math.PR", "math.GT"]
    plane = np.array([[0.0, 0.0], [0.4, 0.0], [3.0, 0.5], [-2.5, 2.0], [0.5, -3.0], [-2.0, -2.5]])
    e = np.linalg.qr(rng.normal(size=(d, 2)))[0].T
    which = rng.integers(0, len(cats), size=n)
    x = (plane[which] @ e + rng.normal(size=(n, d)) * 0.02 + 0.1).astype(np.float32)
    rows = [{"link": "https://arxiv.org/abs/1", "title": "t", "primary_category": cats[k], "citations": 0} for k in which]
    with ts.TheoremIndex.from_embeddings(x, dtype="bf16", metric="ip") as ix, ts.MetaTable.from_sql_rows(rows) as table:
        model = pca.fit(ix, n_components=2)
        got_cats, M, counts = pca.category_means(ix, table, "primary_category", model)
        x64 = stored(ix)
        sample = pca.project_sample(ix, model, [5, 6, 7, 100, 4999, 0])
    assert model.n_samples_seen_ == n and model.explained_variance_ratio_.sum() > 0.9
    assert got_cats == sorted(cats) and counts.sum() == n
    pairs = pca.closest_pairs(got_cats, M, topk=3)
    print("closest pairs", pairs)
    assert (pairs[0][1], pairs[0][2]) == ("math.AG", "math.NT")
    f = (flush_rows() + 2) * 2.0 ** -23
    for row, c in enumerate(got_cats):
        sel = which == cats.index(c)
        assert counts[row] == sel.sum()
        ref = (x64[sel].mean(axis=0) - model.mean_) @ model.components_.T
        bound = np.abs(model.components_) @ (f * np.abs(x64[sel]).sum(axis=0)) / sel.sum() + 2.0 ** -23 * np.abs(ref).max() + 1e-12
        assert np.all(np.abs(M[row] - ref) <= bound), (c, M[row], ref, bound)
    assert np.allclose(sample, model.transform(x64[[5, 6, 7, 100, 4999, 0]]), rtol=0, atol=1e-9)
