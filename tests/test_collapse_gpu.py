"""The grouped search's two kernels on their own (theoremsearch_amd/csrc/kernels_group.h): ts_collapse_topk against the numpy
walk of tests/grouped_common.py on random sorted lists and on hand-made ones, with host and with device buffers; and
ts_rowset_exclude - mask, count and the bits past n - against numpy, then used in a search against the same search through
the bool array.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import grouped_common as gc
from grouped_common import NULL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


def assert_collapse(got, want):
    for g, w, what in zip(got, want, ("scores", "ids", "groups", "found", "complete")):
        assert g.shape == w.shape and np.array_equal(g, w), what


def random_lists(rng, nq, k_in, n, row_offset):
    """sorted lists with tied scores, a padded tail in some, ids outside the column in some; a column of few codes with NULLs
    and negative ids, so that most lists hold duplicates"""
    column = rng.integers(-6, 40, size=n).astype(np.int32)
    column[rng.random(n) < 0.15] = NULL
    scores = np.sort(rng.integers(-8, 8, size=(nq, k_in)).astype(np.float32) / 4, axis=1)[:, ::-1].copy()
    idx = rng.integers(0, n, size=(nq, k_in)).astype(np.int64) + row_offset
    for q in range(nq):
        # ids ascending within a run of equal scores: the canonical order
        for s in np.unique(scores[q]):
            run = scores[q] == s
            idx[q, run] = np.sort(idx[q, run])
        kind = q % 4
        if kind == 1:                                   # the allowed rows ran out: a padded tail
            cut = int(rng.integers(0, k_in + 1))
            scores[q, cut:], idx[q, cut:] = -np.inf, -1
        elif kind == 2 and k_in > 2:                    # ids that are not rows of this column
            idx[q, int(rng.integers(0, k_in))] = row_offset + n
            idx[q, int(rng.integers(0, k_in))] = row_offset - 1 if row_offset else 2**40
    return scores, idx, column


@pytest.mark.parametrize("k_in", [1, 63, 64, 65, 255, 256])
def test_random_sorted_lists_equal_the_walk(ts, k_in):
    rng = np.random.default_rng(100 + k_in)
    n = 500
    for nq in (0, 1, 300):
        for row_offset in (0, 10**9):
            scores, idx, column = random_lists(rng, nq, k_in, n, row_offset)
            for k_out in sorted({1, k_in, 256}):
                got = ts.collapse_topk(scores, idx, column, k_out, row_offset=row_offset)
                assert_collapse(got, gc.collapse_walk(scores, idx, column, k_out, row_offset))


def special_lists():
    n = 600
    column = (np.arange(n) // 3).astype(np.int32)
    ids = np.arange(256, dtype=np.int64)
    desc = -np.arange(256, dtype=np.float32)
    cases = {}
    cases["all padding"] = (np.full(256, -np.inf, np.float32), np.full(256, -1, np.int64), column)
    s, i = desc.copy(), ids.copy()
    s[200:], i[200:] = -np.inf, -1
    cases["padding only in the tail"] = (s, i, column)
    cases["one group throughout"] = (desc, ids, np.full(n, 77, np.int32))
    cases["all NULL"] = (desc, ids, np.full(n, NULL, np.int32))
    # every row its own group, but for one pair: across the edge of the first wave, of a later wave, and the last two entries
    # of a full list (entries 255 and 256, counted from one)
    for a, b in ((63, 64), (191, 192), (254, 255)):
        col = np.arange(n, dtype=np.int32)
        col[a] = col[b] = -9
        cases[f"a duplicate pair at {a}|{b}"] = (desc, ids, col)
    s = desc.copy()
    s[100:] = -np.inf                                   # valid rows that score -inf are entries, not padding
    cases["valid rows with score -inf"] = (s, ids, column)
    cases["negative codes"] = (desc, ids, (-1 - np.arange(n) // 5).astype(np.int32))
    i = ids.copy()
    i[::7] += 10**6
    i[3] = -5
    cases["ids outside the column"] = (desc, i, column)
    s = desc.copy()
    s[10] = np.nan
    cases["a NaN score is padding"] = (s, ids, column)
    return cases


@pytest.mark.parametrize("name", list(special_lists()))
def test_special_lists(ts, name):
    scores, idx, column = special_lists()[name]
    for k_in in (256, 65, 64):
        s, i = scores[None, :k_in].copy(), idx[None, :k_in].copy()
        for k_out in (1, 10, k_in, 256):
            got = ts.collapse_topk(s, i, column, k_out)
            want = gc.collapse_walk(s, i, column, k_out)
            assert_collapse(got, want)
    if name == "all padding":
        assert got[3][0] == 0 and got[4][0] and (got[1] == -1).all() and (got[2] == NULL).all() and np.isneginf(got[0]).all()
    if name == "one group throughout":
        assert got[3][0] == 1 and not got[4][0]
    if name == "all NULL":
        assert got[3][0] == 64 and not got[4][0]
    if name == "a duplicate pair at 63|64":
        f = ts.collapse_topk(scores[None, :65].copy(), idx[None, :65].copy(), column, 65)
        assert f[3][0] == 64 and 64 not in f[1][0]


def test_device_buffers_give_the_host_answer(ts):
    import torch
    from theoremsearch_amd import _ffi
    rng = np.random.default_rng(5)
    for k_in, k_out, nq in ((64, 10, 7), (256, 256, 33), (200, 300, 2)):
        scores, idx, column = random_lists(rng, nq, k_in, 500, 1000)
        want = gc.collapse_walk(scores, idx, column, k_out, 1000)
        dev = [torch.from_numpy(a).cuda() for a in (scores, idx, column)]
        os_ = torch.full((nq, k_out), 7.0, dtype=torch.float32, device="cuda")
        oi = torch.full((nq, k_out), 7, dtype=torch.int64, device="cuda")
        og = torch.full((nq, k_out), 7, dtype=torch.int32, device="cuda")
        found = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
        complete = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for with_groups in (True, False):
            _ffi.check(_ffi.load().ts_collapse_topk(0, C.c_void_p(dev[0].data_ptr()), C.c_void_p(dev[1].data_ptr()), nq, k_in, k_out,
                                                    C.c_void_p(dev[2].data_ptr()), column.shape[0], 1000, C.c_void_p(os_.data_ptr()),
                                                    C.c_void_p(oi.data_ptr()), C.c_void_p(og.data_ptr()) if with_groups else None,
                                                    C.c_void_p(found.data_ptr()), C.c_void_p(complete.data_ptr()), 1, None))
            torch.cuda.synchronize()
            got = (os_.cpu().numpy(), oi.cpu().numpy(), og.cpu().numpy(), found.cpu().numpy(), complete.cpu().numpy().astype(bool))
            assert_collapse(got, want)


# ---- the exclusion ---------------------------------------------------------------------------------------------------------
def check_rowset(rs, want):
    """mask, count and the bits past n of a row set against the bool array it must equal"""
    n = want.shape[0]
    assert rs.n == n and rs.allowed == int(want.sum())
    assert np.array_equal(rs.to_numpy(), want)
    words = rs.words()
    assert words.shape[0] == (n + 31) // 32
    if n % 32:
        assert int(words[-1]) >> (n % 32) == 0


def edge_rows(n):
    rows = {0, n - 1}
    for m in (32, 64, 256):
        for b in range(m, n + m, m):
            rows |= {b - 1, b, b + 1}
    return sorted(r for r in rows if 0 <= r < n)


@pytest.mark.parametrize("n", [1, 3000, 4096])
def test_exclusion_mask_count_and_tail_equal_numpy(ts, n):
    from theoremsearch_amd.metadata import Atom, RANGE
    rng = np.random.default_rng(n)
    column = rng.integers(-50, 400, size=n).astype(np.int32)
    column[rng.random(n) < 0.2] = NULL
    flag = (rng.random(n) < 0.6).astype(np.int32)
    present = np.unique(column[column != NULL])
    absent = np.arange(1000, 1256, dtype=np.int32)
    code_lists = {"none": [], "one present": present[:1].tolist(), "one absent": [999],
                  "256 present": np.resize(present, 256).tolist() if present.size else absent.tolist(),     # repeats, unsorted
                  "256 absent": absent[::-1].tolist(),
                  "mixed": np.concatenate([present[::2][:128], absent[:128]])[::-1].tolist()}
    edges = edge_rows(n)
    row_lists = {"none": [], "edges": edges[:256], "last edges": edges[-256:][::-1] + edges[-1:]}
    with ts.MetaTable.from_columns([column, flag]) as table, table.eval([Atom(RANGE, 1, 1, 1)]) as base:
        check_rowset(base, flag == 1)
        for cname, codes in code_lists.items():
            for rname, rows in row_lists.items():
                rows = rows[:256]
                gone = np.isin(column, np.asarray(codes, dtype=np.int32)) & (column != NULL)
                gone[np.asarray(rows, dtype=np.int64)] = True
                for b, bmask in ((None, np.ones(n, dtype=bool)), (base, flag == 1)):
                    with table.exclude(0, codes, rows, base=b) as rs:
                        check_rowset(rs, bmask & ~gone)
        # malformed lists are refused with a message
        from theoremsearch_amd import _ffi
        for codes, rows, text in (([NULL], [], "TS_META_NULL is not a code"), ([], [n], "outside [0, n)"), ([], [-1], "outside [0, n)"),
                                  (list(range(257)), [], "ncodes outside"), ([], [0] * 257, "nrows outside")):
            with pytest.raises(_ffi.TSearchError) as e:
                table.exclude(0, codes, rows)
            assert e.value.code == -1 and text in str(e.value)
        with pytest.raises(_ffi.TSearchError):
            table.exclude(5, [1])                          # no such column


def test_exclusion_row_set_searches_like_the_bool_array(ts):
    import exact_common as ec
    n, d, nq = 3000, 128, 8
    q, c, _ = ec.make_corpus("ip", n, d, nq, seed=3)
    column = (np.arange(n) // 8).astype(np.int32)
    column[::5] = NULL
    t = ec.truth(q, c, "ip")
    order = ec.canonical_order(t)
    codes = column[order[0][:40]]
    codes = np.unique(codes[codes != NULL])
    rows = order[1][:30]
    allowed = ~(np.isin(column, codes) & (column != NULL))
    allowed[rows] = False
    with ts.TheoremIndex.from_embeddings(c, dtype="f32", metric="ip") as ix, ts.MetaTable.from_columns([column]) as table, \
            table.exclude(0, codes, rows) as rs:
        check_rowset(rs, allowed)
        for k in (10, 256):
            want_s, want_i = ec.ref_topk(t, order, k, allowed)
            via_set = ix.search(q, k, mask=rs)
            via_bool = ix.search(q, k, mask=allowed)
            for got in (via_set, via_bool):
                assert np.array_equal(got[0], want_s) and np.array_equal(got[1], want_i)
            assert np.array_equal(via_set[0].view(np.uint32), via_bool[0].view(np.uint32))
