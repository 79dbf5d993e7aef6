"""Metadata filters evaluated on the device (ts_meta_eval; theoremsearch_amd/csrc/kernels_meta.h) and the searches behind a row
set (ts_search_rowset, ts_search_biased_rowset): the mask, its count and its tail bits against filters.filter_mask /
sql_filter_mask and against the numpy model of the atom semantics (tests/metadata_common.py), the upsert, and the search
through a row set against the same search through the bool array - ids and score bits - on the scan and on the matrix
path.  Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

from filters_common import filter_states, make_sql_rows, make_theorems, sql_filter_states
from metadata_common import model_mask, random_columns, random_programs
from oracle import oracle

pytestmark = pytest.mark.gpu

SCAN, MFMA = 1, 2
DENSE = ["types_tags", "authors", "preprints_cited"]
SPARSE = ["arxiv_years_journal", "selective"]


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


@pytest.fixture(scope="module")
def showcase(ts):
    data = make_theorems(3000)
    with ts.MetaTable.from_theorems(data) as table:
        yield data, table


@pytest.fixture(scope="module")
def sql(ts):
    rows = make_sql_rows(4000)
    with ts.MetaTable.from_sql_rows(rows) as table:
        yield rows, table


def check_rowset(rs, want):
    """mask, count and the bits past n of a row set against the bool array it must equal"""
    n = want.shape[0]
    assert rs.n == n and rs.allowed == int(want.sum())
    assert np.array_equal(rs.to_numpy(), want)
    words = rs.words()
    assert words.shape[0] == (n + 31) // 32
    if n % 32:
        assert int(words[-1]) >> (n % 32) == 0


@pytest.mark.parametrize("state", list(filter_states()))
def test_showcase_state_evaluates_to_filter_mask(ts, showcase, state):
    from theoremsearch_amd.filters import filter_mask
    data, table = showcase                     # n = 3000: no multiple of 32
    f = filter_states()[state]
    with table.eval(f) as rs:
        check_rowset(rs, filter_mask(data, f))


@pytest.mark.parametrize("state", list(sql_filter_states()))
def test_sql_state_evaluates_to_sql_filter_mask(ts, sql, state):
    from theoremsearch_amd.filters import sql_filter_mask
    rows, table = sql                          # n = 4000: a multiple of 32
    f = sql_filter_states()[state]
    with table.eval(f) as rs:
        check_rowset(rs, sql_filter_mask(rows, f))


@pytest.mark.parametrize("n", [1, 31, 33, 63, 64, 65, 257])
def test_partial_word_partial_wave_and_one_row_more(ts, n):
    from theoremsearch_amd.filters import sql_filter_mask
    rows = make_sql_rows(n)
    with ts.MetaTable.from_sql_rows(rows) as table:
        for state in ("everything", "open"):
            f = sql_filter_states()[state]
            with table.eval(f) as rs:
                check_rowset(rs, sql_filter_mask(rows, f))
        with table.eval([]) as rs:             # the empty program: every row, and still no bit past n
            check_rowset(rs, np.ones(n, dtype=bool))


def test_random_programs_against_the_numpy_model(ts):
    n = 5000
    cols = random_columns(n)
    with ts.MetaTable.from_columns(cols) as table:
        for i, prog in enumerate(random_programs()):
            with table.eval(prog) as rs:
                want = model_mask(prog, cols, n)
                assert rs.allowed == int(want.sum()), i
                assert np.array_equal(rs.to_numpy(), want), i


def test_more_rows_than_one_pass_of_the_grid(ts):
    """The kernel's grid is capped at 8 workgroups per CU, each taking a block of 256 rows per step: beyond
    256 CUs x 8 x 256 = 524,288 rows a workgroup walks on by the grid.  4.5M rows - eight or nine steps per workgroup -
    and no multiple of anything."""
    from theoremsearch_amd.metadata import ANY_IN, IN, IS_NULL, NULL, RANGE, Atom, code_set
    n = 4_500_003
    rng = np.random.default_rng(44)
    a = rng.integers(0, 40, n).astype(np.int32)
    a[rng.random(n) < 0.1] = NULL
    b = rng.integers(1990, 2030, n).astype(np.int32)
    lens = rng.integers(0, 3, n)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    cols = [a, b, (offsets, rng.integers(0, 9, int(offsets[-1])).astype(np.int32))]
    progs = [[],
             [Atom(RANGE, 1, 2000, 2019, group=0), Atom(IN, 0, negate=1, group=1, set=code_set([1, 5, 39], 40), set_bits=40)],
             [Atom(ANY_IN, 2, group=0, set=code_set([2, 7], 9), set_bits=9), Atom(IS_NULL, 0, group=0), Atom(RANGE, 1, 1995, 1995, group=3)]]
    with ts.MetaTable.from_columns(cols) as table:
        for i, prog in enumerate(progs):
            with table.eval(prog) as rs:
                want = model_mask(prog, cols, n)
                assert rs.allowed == int(want.sum()), i
                assert np.array_equal(rs.words(), np.packbits(np.concatenate([want, np.zeros(-n % 32, dtype=bool)]), bitorder="little").view(np.uint32)), i


def test_malformed_programs_are_refused(ts):
    from theoremsearch_amd import _ffi
    from theoremsearch_amd.metadata import ANY_IN, IN, RANGE, Atom, code_set
    cols = random_columns(300)
    with ts.MetaTable.from_columns(cols) as table:
        s = code_set([1], 8)
        for prog in ([Atom(RANGE, 0, 5, 4)], [Atom(ANY_IN, 5, negate=1, set=s, set_bits=8)], [Atom(ANY_IN, 0, set=s, set_bits=8)],
                     [Atom(RANGE, 5, 0, 1)], [Atom(IN, 0, set=None, set_bits=8)], [Atom(7, 0)], [Atom(RANGE, 6, 0, 1)],
                     [Atom(RANGE, 0, 0, 1, group=g) for g in range(17)], [Atom(RANGE, 0, 0, 1)] * 33):
            with pytest.raises(_ffi.TSearchError) as e:
                table.eval(prog)
            assert e.value.code == -1, prog


def test_upsert_changes_exactly_the_models_bits(ts):
    from theoremsearch_amd.filters import filter_mask
    data = make_theorems(3000)
    other = make_theorems(100, seed=77)
    states = filter_states()
    with ts.MetaTable.from_theorems(data) as table:
        before = {name: table.eval(f) for name, f in states.items()}
        table.set_rows(1000, other)
        merged = data[:1000] + other + data[1100:]
        for name, f in states.items():
            want = model_mask(table.compile(f), table.columns, table.n)
            assert np.array_equal(want, filter_mask(merged, f)), name
            with table.eval(f) as rs:
                check_rowset(rs, want)
            old = filter_mask(data, f)
            assert np.array_equal(want[:1000], old[:1000]) and np.array_equal(want[1100:], old[1100:])
            check_rowset(before[name], old)                     # a row set made before the upsert keeps its bits
            before[name].close()
        assert any(not np.array_equal(filter_mask(merged, f)[1000:1100], filter_mask(data, f)[1000:1100]) for f in states.values())


# ---- search behind a row set --------------------------------------------------------------------------------------------------
N, NQ, K = 20_000, 32, 10          # above TS_MFMA_MIN_ROWS, a batch the matrix path takes


@functools.lru_cache(maxsize=1)
def library():
    return make_theorems(N)


@functools.lru_cache(maxsize=2)
def embeddings(d):
    return oracle.inputs(N, NQ, d, 500 + d, "ip")


@pytest.fixture(scope="module")
def big(ts):
    with ts.MetaTable.from_theorems(library()) as table:
        yield table


@pytest.fixture(scope="module", params=[("bf16", 768), ("f32", 128)], ids=["bf16-768", "f32-128-general-width"])
def index(ts, request):
    dtype, d = request.param
    q, c = embeddings(d)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
        yield ix, q


def same_answer(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("state", DENSE)
def test_dense_row_set_runs_the_matrix_path_with_the_bool_arrays_answer(ts, big, index, state):
    from theoremsearch_amd.filters import filter_mask
    ix, q = index
    f = filter_states()[state]
    mask = filter_mask(library(), f)
    assert mask.mean() >= 0.1
    with big.eval(f) as rs:
        assert rs.allowed == int(mask.sum())
        want = ix.search(q, K, algo="mfma", mask=mask, return_stats=True)
        assert want[2]["algo"] == MFMA
        for algo in ("mfma", "auto"):
            got = ix.search(q, K, algo=algo, mask=rs, return_stats=True)
            assert got[2]["algo"] == MFMA, algo
            assert same_answer(got[:2], want[:2]), algo
        assert mask[want[1][want[1] >= 0]].all() and (want[1] >= 0).all()


@pytest.mark.parametrize("state", SPARSE)
def test_sparse_row_set_runs_the_scan_and_refuses_mfma(ts, big, index, state):
    from theoremsearch_amd import _ffi
    from theoremsearch_amd.filters import filter_mask
    ix, q = index
    f = filter_states()[state]
    mask = filter_mask(library(), f)
    assert 0 < mask.mean() < 0.1
    with big.eval(f) as rs:
        got = ix.search(q, K, algo="auto", mask=rs, return_stats=True)
        want = ix.search(q, K, algo="auto", mask=mask, return_stats=True)
        assert got[2]["algo"] == SCAN and want[2]["algo"] == SCAN
        assert same_answer(got[:2], want[:2]) and mask[got[1][got[1] >= 0]].all()
        with pytest.raises(_ffi.TSearchError) as e:
            ix.search(q, K, algo="mfma", mask=rs)
        assert e.value.code == -5


def test_row_set_that_allows_nothing(ts, big, index):
    ix, q = index
    with big.eval(filter_states()["nothing"]) as rs:
        assert rs.allowed == 0
        scores, idx = ix.search(q, K, mask=rs)
        assert np.all(np.isneginf(scores)) and np.all(idx == -1)


@pytest.mark.parametrize("algo", ["mfma", "scan"])
def test_biased_search_behind_a_row_set(ts, big, index, algo):
    from theoremsearch_amd.filters import filter_mask
    ix, q = index
    f = filter_states()["authors"]
    mask = filter_mask(library(), f)
    bias = np.log1p(np.array([it["citations"] for it in library()], dtype=np.float32))
    with big.eval(f) as rs:
        want = ix.search_biased(q, K, bias, 0.02, mask=mask, algo=algo, return_stats=True)
        got = ix.search_biased(q, K, bias, 0.02, mask=rs, algo=algo, return_stats=True)
        assert want[3]["algo"] == got[3]["algo"] == (MFMA if algo == "mfma" else SCAN)
        assert same_answer(got[:3], want[:3])
        assert mask[got[2]].all()
        if algo == "scan":                      # algo=None, the scan-only entry point: the same kernel, the same bits
            assert same_answer(ix.search_biased(q, K, bias, 0.02, mask=rs), want[:3])


def test_refusals_keep_the_old_contract(ts, big, showcase, index):
    from theoremsearch_amd import _ffi
    ix, q = index
    lib = _ffi.load()
    with showcase[1].eval(filter_states()["open"]) as small:        # 3,000 rows against an index of 20,000
        with pytest.raises(_ffi.TSearchError) as e:
            ix.search(q, K, mask=small)
        assert e.value.code == -1
        with pytest.raises(_ffi.TSearchError) as e:
            ix.search_biased(q, K, np.zeros(N, dtype=np.float32), 0.02, mask=small, algo="auto")
        assert e.value.code == -1
    # the row set's mask as a bare device pointer: a device mask without a count, the scan only
    with big.eval(filter_states()["authors"]) as rs:
        qq = np.ascontiguousarray(q, dtype=np.float32)
        scores, idx = np.empty((NQ, K), dtype=np.float32), np.empty((NQ, K), dtype=np.int64)
        stats = _ffi.SearchStats()
        args = (ix.handle, _ffi.as_ptr(qq), _ffi.TS_F32, 0, NQ, K, C.c_void_p(rs.mask_ptr), 1, _ffi.as_ptr(scores), _ffi.as_ptr(idx), 0, None)
        assert lib.ts_search_filtered_ex(*args, _ffi.TS_ALGO_MFMA, C.byref(stats)) == -5
        assert lib.ts_search_filtered_ex(*args, _ffi.TS_ALGO_AUTO, C.byref(stats)) == 0 and stats.algo == SCAN
        want = ix.search(q, K, algo="scan", mask=rs)
        assert same_answer((scores, idx), want)
