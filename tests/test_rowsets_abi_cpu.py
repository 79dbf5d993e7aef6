"""ts_search_rowsets without a device (include/tsearch.h): every malformed call is TS_ERR_INVALID with a message - the sizes, the
pointers and which[] are judged before the index handle is read - and a well-formed request fails with the no-device code
where it needs the device, instead of falling back to anything."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, gpu_available
from theoremsearch_amd import _ffi

INVALID, NODEVICE = -1, -4


def last_error():
    return _ffi.load().ts_last_error().decode()


def call(ix=None, nq=2, k=4, nsets=2, which=(0, -1), sets="fake", q_dtype=0, algo=0, nulls=(), stats=True):
    """One ts_search_rowsets call with host buffers; ``sets="fake"``: an array of NULL handles (nobody may read through them
    before the index handle has been refused)."""
    q = np.zeros((max(nq, 1), 8), dtype=np.float32)
    s, i = np.zeros((max(nq, 1), max(k, 1)), dtype=np.float32), np.zeros((max(nq, 1), max(k, 1)), dtype=np.int64)
    w = np.asarray(which, dtype=np.int32)
    handles = (C.c_void_p * max(nsets, 1))() if sets == "fake" else sets
    ptr = {"queries": _ffi.as_ptr(q), "scores": _ffi.as_ptr(s), "idx": _ffi.as_ptr(i), "sets": handles, "which": _ffi.as_ptr(w)}
    for name in nulls:
        ptr[name] = None
    st = _ffi.RowsetsStats()
    st.pass_queries = 77
    rc = _ffi.load().ts_search_rowsets(ix, ptr["queries"], q_dtype, 0, nq, k, ptr["sets"], nsets, ptr["which"], ptr["scores"], ptr["idx"], 0,
                                       None, algo, C.byref(st) if stats else None)
    if stats:
        assert st.pass_queries == 0                      # the counters are reset before anything is judged
    return rc


def test_the_stats_struct_matches_the_header():
    text = open(os.path.join(ROOT, "include", "tsearch.h")).read()
    body = re.search(r"typedef struct ts_rowsets_stats \{(.*?)\} ts_rowsets_stats;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|int64_t)\s+(\w+);", body)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [(n, ctype[t]) for t, n in fields] == list(_ffi.RowsetsStats._fields_)
    assert int(re.search(r"#define\s+TS_MAX_ROWSETS\s+(\d+)", text).group(1)) == _ffi.TS_MAX_ROWSETS == 256
    assert _ffi.load().ts_version() == 100


def test_malformed_sizes_are_refused_with_a_message():
    for bad, text in ((dict(q_dtype=5), "q_dtype"), (dict(nq=-1), "nq is negative"), (dict(k=0), "k outside"), (dict(k=257), "k outside"),
                      (dict(nsets=-1), "nsets outside"), (dict(nsets=257), "nsets outside"), (dict(algo=3), "algo out of range"),
                      (dict(algo=-1), "algo out of range")):
        assert call(**bad) == INVALID, bad
        assert text in last_error() and "ts_search_rowsets" in last_error(), (bad, last_error())
    # the sizes are judged before the pointers
    assert call(k=0, nulls=("queries", "scores", "idx", "sets", "which")) == INVALID and "k outside" in last_error()


def test_null_pointers_are_refused_with_a_message():
    for name in ("queries", "scores", "idx"):
        assert call(nulls=(name,)) == INVALID and "NULL argument" in last_error(), name
    assert call(nulls=("sets",)) == INVALID and "sets is NULL" in last_error()
    assert call(nulls=("which",)) == INVALID and "which is NULL" in last_error()
    assert call(stats=False, nulls=("queries",)) == INVALID          # the stats pointer is optional


def test_which_is_judged_before_any_handle_is_read():
    for which in ((2, 0), (-2, 0), (5, 5), (-1, 2)):
        assert call(which=which) == INVALID and "outside [-1, nsets)" in last_error(), which
    assert call(nsets=0, which=(0, -1), nulls=("sets",)) == INVALID and "outside [-1, nsets)" in last_error()
    # a named entry of sets[] that is NULL
    assert call(which=(0, -1)) == INVALID and "NULL" in last_error()
    # nothing named: the NULL index handle is what is left to refuse
    assert call(which=(-1, -1)) == INVALID and "NULL argument" in last_error()
    assert call(nq=0, which=()) == INVALID and "NULL argument" in last_error()


@pytest.mark.skipif(gpu_available(), reason="checks the no-device behaviour")
def test_a_well_formed_request_fails_with_the_no_device_code():
    import theoremsearch_amd as ts
    assert _ffi.device_count() == 0
    with pytest.raises(_ffi.TSearchError) as e:
        ts.TheoremIndex(64, 128, dtype="bf16", metric="ip")          # no index, so no search behind row sets, without a device
    assert e.value.code == NODEVICE and "no CPU path" in str(e.value)
    with pytest.raises(_ffi.TSearchError) as e:
        ts.MetaTable.from_columns([np.zeros(64, np.int32)])          # ... and no row set
    assert e.value.code == NODEVICE
    # the host-only index has no filters: refused, not answered by another path
    host = ts.TheoremIndex(64, 128, device=-1)
    with pytest.raises(ValueError):
        host.search_rowsets(np.zeros((2, 128), np.float32), 4, [], [-1, -1])
