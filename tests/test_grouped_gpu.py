"""Grouped search on the device (ts_search_grouped) against the brute-force model of tests/grouped_common.py on exact corpora
(tests/exact_common.py: the same score bits in every arithmetic): ids, score bits and groups equal the walk of the whole
canonical order on every path, and ts_grouped_stats equals the ladder model's counts - so the stages really ran, and a
"fix" that always searches deep fails here.  Every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import exact_common as ec
import grouped_common as gc
from grouped_common import N, NQ, NULL
from oracle import oracle

pytestmark = pytest.mark.gpu

DESIGNS = ("row8", "pile", "two", "null")
INVALID, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


def make_table(ts, columns, allowed):
    """(table, row set): the designs as columns 0 .., a 0 / 1 flag as the last one, evaluated to the row set of `allowed`"""
    from theoremsearch_amd.metadata import Atom, RANGE
    table = ts.MetaTable.from_columns(list(columns) + [allowed.astype(np.int32)])
    return table, table.eval([Atom(RANGE, len(columns), 1, 1)])


def stage1_path(ix, q, k, rowset, algo):
    """the path stage 1 must report: the one the plain search takes at the first depth (forced: that one)"""
    if algo != "auto":
        return 1 if algo == "scan" else 2
    return ix.search(q, gc.depths(k)[0], mask=rowset, return_stats=True)[2]["algo"]


def assert_case(got, name, design, masked, k, row_offset=0, queries=slice(None)):
    """scores (bits), ids, groups and the stats of one call against the models"""
    s, i, g, stage, passes = gc.reference(name, design, masked, k)
    s, i, g, stage, passes = s[queries], i[queries], g[queries], stage[queries], passes[queries]
    first, deep = gc.depths(k)
    what = (name, design, masked, k)
    assert np.array_equal(got[1], np.where(i >= 0, i + row_offset, -1)), what
    assert np.array_equal(got[0].view(np.uint32), s.view(np.uint32)), what
    assert np.array_equal(got[2], g), what
    st = got[3]
    assert st["depth"] == first, what
    assert st["deep_queries"] == (int((stage >= 2).sum()) if first < deep else 0), (what, st)
    assert st["excluded_queries"] == int((stage == 3).sum()), (what, st)
    assert st["exclusion_passes"] == int(passes.sum()), (what, st)


@pytest.fixture(scope="module", params=[("ip128", "bf16"), ("ip128", "f32"), ("cos768", "bf16"), ("cos768", "f32")], ids="-".join)
def setup(ts, request):
    name, dtype = request.param
    metric, d = gc.CORPORA[name]
    q, c, piles, t, order = gc.corpus(name)
    designs = gc.designs(piles)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric=metric) as ix:
        table, rs = make_table(ts, [designs[x] for x in DESIGNS], gc.row_mask())
        with table, rs:
            yield name, dtype, ix, table, rs, q


@pytest.mark.parametrize("algo", ["auto", "scan", "mfma"])
def test_grouped_search_equals_the_brute_force_walk(ts, setup, algo):
    name, dtype, ix, table, rs, q = setup
    for col, design in enumerate(DESIGNS):
        for k in gc.KS:
            for masked in (False, True):
                got = ix.search_grouped(q, k, table, col, mask=rs if masked else None, algo=algo, return_groups=True, return_stats=True)
                assert got[3]["algo"] == stage1_path(ix, q, k, rs if masked else None, algo), (design, k, masked)
                assert_case(got, name, design, masked, k)


def test_k_256_sends_every_query_to_the_exclusion(ts, setup):
    name, dtype, ix, table, rs, q = setup
    for masked in (False, True):
        got = ix.search_grouped(q, 256, table, 0, mask=rs if masked else None, return_groups=True, return_stats=True)
        assert got[3]["excluded_queries"] == NQ and got[3]["deep_queries"] == 0
        assert_case(got, name, "row8", masked, 256)


def test_one_query_and_no_query(ts, setup):
    name, dtype, ix, table, rs, q = setup
    for b in (0, 1, 3):                                    # pileA (stage 3 under the pile design), pileB, a dense query
        got = ix.search_grouped(q[b], 10, table, 1, return_groups=True, return_stats=True)
        assert got[3]["algo"] == 1                         # the UI's call: one query runs on the scan
        assert_case(got, name, "pile", False, 10, queries=slice(b, b + 1))
    got = ix.search_grouped(q[:0], 10, table, 1, return_groups=True, return_stats=True)
    assert got[0].shape == (0, 10) and got[1].shape == (0, 10) and got[2].shape == (0, 10) and got[3]["depth"] == 26


def test_view_row_offset_and_names(ts, setup):
    name, dtype, ix, table, rs, q = setup
    with ix.view() as v:
        assert_case(v.search_grouped(q, 10, table, 1, mask=rs, return_groups=True, return_stats=True), name, "pile", True, 10)
    ix.set_row_offset(10**10)
    try:
        assert_case(ix.search_grouped(q, 10, table, "c1", return_groups=True, return_stats=True), name, "pile", False, 10, row_offset=10**10)
        assert_case(ix.search_grouped(q, 100, table, "c2", mask=rs, return_groups=True, return_stats=True), name, "two", True, 100, row_offset=10**10)
    finally:
        ix.set_row_offset(0)
    s, i = ix.search_grouped(q, 10, table, 0)              # the plain form: two arrays
    assert np.array_equal(i, gc.reference(name, "row8", False, 10)[1])


def test_device_queries_and_device_outputs(ts, setup):
    import torch
    name, dtype, ix, table, rs, q = setup
    k = 10
    qs = oracle.f32_to_bf16_bits(q) if dtype == "bf16" else np.array(q)      # the lattices' values are exact in bf16
    qd = torch.from_numpy(qs.view(np.int16) if dtype == "bf16" else qs).cuda()
    for col, design in ((1, "pile"), (2, "two")):
        o_s = torch.zeros((NQ, k), dtype=torch.float32, device="cuda")
        o_i = torch.zeros((NQ, k), dtype=torch.int64, device="cuda")
        o_g = torch.zeros((NQ, k), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for groups_ptr in (o_g.data_ptr(), 0):
            st = ix.search_grouped_device(qd.data_ptr(), dtype, NQ, k, table, col, o_s.data_ptr(), o_i.data_ptr(), groups_ptr, rowset=rs)
            got = (o_s.cpu().numpy(), o_i.cpu().numpy(), o_g.cpu().numpy(), st)      # the call has waited for its result
            assert_case(got, name, design, True, k)


def test_columns_with_nulls_and_negative_ids_and_a_sparse_row_set(ts, setup):
    name, dtype, ix, table, rs, q = setup
    _, _, piles, t, order = gc.corpus(name)
    mixed = gc.designs(piles)["mixed"]
    few = np.zeros(N, dtype=bool)
    few[np.random.default_rng(3).choice(N, 20, replace=False)] = True      # fewer rows than k = 32 and than `first` = 64: every list is padded
    table2, rs2 = make_table(ts, [mixed], few)
    with table2, rs2:
        for k in (10, 32):
            for algo in ("auto", "scan"):
                got = ix.search_grouped(q, k, table2, 0, algo=algo, return_groups=True, return_stats=True)
                assert_case(got, name, "mixed", False, k)
        got = ix.search_grouped(q, 32, table2, 0, mask=rs2, return_groups=True, return_stats=True)
        want = gc.brute_force(t, order, mixed, 32, few)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want))
        assert got[3]["deep_queries"] == 0 and got[3]["excluded_queries"] == 0       # padding certifies in stage 1
        assert (got[1] == -1).any() and (got[2][got[1] == -1] == NULL).all()
        from theoremsearch_amd import _ffi
        with pytest.raises(_ffi.TSearchError) as e:                                # 20 of 16,869 rows: too sparse for the matrix path
            ix.search_grouped(q, 10, table2, 0, mask=rs2, algo="mfma")
        assert e.value.code == UNSUPPORTED


def test_attached_rows(ts):
    import torch
    name = "ip128"
    q, c, piles, t, order = gc.corpus(name)
    cap = (N + 255) // 256 * 256
    dev = torch.zeros((cap, c.shape[1]), dtype=torch.float32, device="cuda")
    dev[:N] = torch.from_numpy(np.array(c)).cuda()
    torch.cuda.synchronize()
    table, rs = make_table(ts, [gc.designs(piles)["pile"]], gc.row_mask())
    with ts.TheoremIndex(N, c.shape[1], dtype="f32", metric="ip") as ix, table, rs:
        ix.attach_device(dev.data_ptr(), cap, keep_alive=dev)
        for masked in (False, True):
            got = ix.search_grouped(q, 10, table, 0, mask=rs if masked else None, return_groups=True, return_stats=True)
            assert_case(got, name, "pile", masked, 10)


def test_k_chunked_width(ts):
    """bf16 d = 2304: the ip corpus with zero columns behind it - the same scores, on the k-chunked matrix kernel"""
    name = "ip128"
    q, c, piles, t, order = gc.corpus(name)
    wide_q = np.zeros((NQ, 2304), dtype=np.float32)
    wide_c = np.zeros((N, 2304), dtype=np.float32)
    wide_q[:, :q.shape[1]], wide_c[:, :c.shape[1]] = q, c
    designs = gc.designs(piles)
    table, rs = make_table(ts, [designs[x] for x in DESIGNS], gc.row_mask())
    with ts.TheoremIndex.from_embeddings(wide_c, dtype="bf16", metric="ip") as ix, table, rs:
        for algo in ("auto", "scan", "mfma"):
            for col, design in enumerate(DESIGNS):
                for masked in (False, True):
                    got = ix.search_grouped(wide_q, 10, table, col, mask=rs if masked else None, algo=algo, return_groups=True, return_stats=True)
                    assert got[3]["algo"] == stage1_path(ix, wide_q, 10, rs if masked else None, algo)
                    assert_case(got, name, design, masked, 10)


def test_refusals(ts, setup):
    from theoremsearch_amd import _ffi
    name, dtype, ix, table, rs, q = setup

    def refused(code, text, fn, *a, **kw):
        with pytest.raises(_ffi.TSearchError) as e:
            fn(*a, **kw)
        assert e.value.code == code and text in str(e.value), str(e.value)

    with ix.subset(np.arange(0, N, 2)) as sub:
        refused(UNSUPPORTED, "subset index", sub.search_grouped, q, 10, table, 0)
    lists = (np.arange(N + 1, dtype=np.int64), np.zeros(N, dtype=np.int32))
    with ts.MetaTable.from_columns([np.zeros(N, np.int32), lists]) as t2:
        refused(INVALID, "list column", ix.search_grouped, q, 10, t2, 1)
        refused(INVALID, "outside [0, 2)", ix.search_grouped, q, 10, t2, 2)
    with ts.MetaTable.from_columns([np.zeros(N - 1, np.int32)]) as t3:
        refused(INVALID, "the meta table has", ix.search_grouped, q, 10, t3, 0)
        with t3.exclude(0, [5]) as foreign:
            refused(INVALID, "the row set has", ix.search_grouped, q, 10, table, 0, mask=foreign)
    # a column that was never set: a table made through the C ABI with two columns, one of them uploaded
    lib, h = _ffi.load(), C.c_void_p()
    _ffi.check(lib.ts_meta_create(0, N, 2, C.byref(h)))
    try:
        zeros = np.zeros(N, dtype=np.int32)
        _ffi.check(lib.ts_meta_set_column(h, 0, _ffi.as_ptr(zeros), 0, N))
        out_s, out_i = np.zeros((NQ, 10), np.float32), np.zeros((NQ, 10), np.int64)
        rc = lib.ts_search_grouped(ix.handle, _ffi.as_ptr(q), 0, 0, NQ, 10, h, 1, None, _ffi.as_ptr(out_s), _ffi.as_ptr(out_i), None, 0, None, 0, None)
        assert rc == INVALID and "never set" in lib.ts_last_error().decode()
    finally:
        _ffi.check(lib.ts_meta_destroy(h))
    refused(INVALID, "k outside", ix.search_grouped, q, 0, table, 0)
    refused(INVALID, "k outside", ix.search_grouped, q, 257, table, 0)
    with pytest.raises(TypeError):
        ix.search_grouped(q, 10, table, 0, mask=gc.row_mask())            # a bare mask is not served
    # forced MFMA where stage 1 has no matrix path: a width the matrix kernels do not serve
    x = np.zeros((300, 96), dtype=np.float32)
    with ts.TheoremIndex.from_embeddings(x, dtype="f32", metric="ip") as narrow, ts.MetaTable.from_columns([np.zeros(300, np.int32)]) as t4:
        refused(UNSUPPORTED, "MFMA", narrow.search_grouped, x[:2], 5, t4, 0, algo="mfma")
        s, i = narrow.search_grouped(x[:2], 5, t4, 0)                      # served on the scan: one group, then padding
        assert i[:, 0].tolist() == [0, 0] and (i[:, 1:] == -1).all()


# ---- the pgvector adapter -------------------------------------------------------------------------------------------------
def test_pgvector_distinct_returns_one_hit_per_paper(ts):
    from filters_common import make_sql_rows
    from theoremsearch_amd import pgvector
    n, d = 3000, 128
    rows = make_sql_rows(n)
    q, c, _ = ec.make_corpus("ip", n, d, 4, seed=11)
    t = ec.truth(q, c, "ip")
    order = ec.canonical_order(t)
    with ts.TheoremIndex.from_embeddings(c, dtype="f32", metric="ip") as ix, ts.MetaTable.from_sql_rows(rows) as meta:
        paper = np.asarray(meta.columns[meta.col["paper"]])
        assert np.unique(paper).size < n                       # papers have several rows
        want = gc.brute_force(t, order, paper, 10)
        hits = pgvector.search_batch(ix, q, 10, 0.0, distinct=(meta, "paper"))
        for b in range(4):
            one = pgvector.search(ix, q[b], 10, distinct=(meta, "paper"))
            assert one == hits[b]
            assert [h["row"] for h in one] == want[1][b].tolist() and [h["group"] for h in one] == want[2][b].tolist()
            assert [h["similarity"] for h in one] == [1.0 + float(s) for s in want[0][b]]
            assert len({h["group"] for h in one}) == 10
        with pytest.raises(ValueError):
            pgvector.search(ix, q[0], 10, citation_weight=0.1, citations=[1] * n, distinct=(meta, "paper"))
        with pytest.raises(ValueError):
            pgvector.search_batch(ix, q, 10, 0.1, citations=[1] * n, distinct=(meta, "paper"))
        # the default is what it was: the plain top 10, papers repeated
        plain = pgvector.search(ix, q[0], 10)
        want_s, want_i = ec.ref_topk(t, order, 10)
        assert [h["row"] for h in plain] == want_i[0].tolist() and all("group" not in h for h in plain)
