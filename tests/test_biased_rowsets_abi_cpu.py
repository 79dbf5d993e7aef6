"""ts_search_biased_rowsets without a device (include/tsearch.h): every malformed call is TS_ERR_INVALID with a message that names
the entry - the sizes, the pointers, the bias, the weights and which[] are judged before the index handle is read - and nq == 0
on a live request does nothing."""
import ctypes as C

import numpy as np
import pytest

from theoremsearch_amd import _ffi

INVALID, NODEVICE = -1, -4
ENTRY = "ts_search_biased_rowsets"


def last_error():
    return _ffi.load().ts_last_error().decode()


def call(ix=None, nq=2, k=4, nsets=2, which=(0, -1), weights=(0.25, 0.0), q_dtype=0, algo=0, nulls=(), stats=True, sims=True):
    """One call with host buffers and an array of NULL set handles (nobody may read through them before the index handle has
    been refused)."""
    q = np.zeros((max(nq, 1), 8), dtype=np.float32)
    s, m = np.zeros((max(nq, 1), max(k, 1)), dtype=np.float32), np.zeros((max(nq, 1), max(k, 1)), dtype=np.float32)
    i = np.zeros((max(nq, 1), max(k, 1)), dtype=np.int64)
    w = np.asarray(which, dtype=np.int32)
    wt = np.asarray(weights, dtype=np.float32)
    b = np.zeros(16, dtype=np.float32)
    handles = (C.c_void_p * max(nsets, 1))()
    ptr = {"queries": _ffi.as_ptr(q), "scores": _ffi.as_ptr(s), "idx": _ffi.as_ptr(i), "sets": handles, "which": _ffi.as_ptr(w),
           "bias": _ffi.as_ptr(b), "weights": _ffi.as_ptr(wt), "sims": _ffi.as_ptr(m) if sims else None}
    for name in nulls:
        ptr[name] = None
    st = _ffi.RowsetsStats()
    st.pass_queries = 77
    rc = _ffi.load().ts_search_biased_rowsets(ix, ptr["queries"], q_dtype, 0, nq, k, ptr["bias"], 0, ptr["weights"], ptr["sets"], nsets,
                                              ptr["which"], ptr["scores"], ptr["sims"], ptr["idx"], 0, None, algo, C.byref(st) if stats else None)
    if stats:
        assert st.pass_queries == 0                      # the counters are reset before anything is judged
    return rc


def test_malformed_sizes_are_refused_with_a_message():
    for bad, text in ((dict(q_dtype=5), "q_dtype"), (dict(nq=-1), "nq is negative"), (dict(k=0), "k outside"), (dict(k=257), "k outside"),
                      (dict(nsets=-1), "nsets outside"), (dict(nsets=257), "nsets outside"), (dict(algo=3), "algo out of range"),
                      (dict(algo=-1), "algo out of range")):
        assert call(**bad) == INVALID, bad
        assert text in last_error() and ENTRY in last_error(), (bad, last_error())
    # the sizes are judged before the pointers
    assert call(k=0, nulls=("queries", "scores", "idx", "sets", "which", "bias", "weights")) == INVALID and "k outside" in last_error()


def test_null_pointers_are_refused_with_a_message():
    for name in ("queries", "scores", "idx"):
        assert call(nulls=(name,)) == INVALID and "NULL argument" in last_error() and ENTRY in last_error(), name
    assert call(nulls=("sets",)) == INVALID and "sets is NULL" in last_error() and ENTRY in last_error()
    assert call(nulls=("which",)) == INVALID and "which is NULL" in last_error() and ENTRY in last_error()
    assert call(nulls=("bias",)) == INVALID and "bias is NULL" in last_error() and ENTRY in last_error()
    assert call(nulls=("weights",)) == INVALID and "weights is NULL" in last_error() and ENTRY in last_error()
    assert call(nq=0, which=(), weights=(), nulls=("bias",)) == INVALID and "bias is NULL" in last_error()
    assert call(stats=False, nulls=("queries",)) == INVALID          # the stats pointer is optional
    assert call(sims=False, nulls=("bias",)) == INVALID              # ... and so is out_sims


def test_a_weight_that_is_not_finite_is_refused():
    for bad in (float("nan"), float("inf"), float("-inf")):
        for at in (0, 1):
            weights = [0.25, 0.0]
            weights[at] = bad
            assert call(weights=weights) == INVALID, (bad, at)
            assert "not finite" in last_error() and ENTRY in last_error(), last_error()
    # judged before which[] and the handles
    assert call(weights=(float("nan"), 0.0), which=(7, 7)) == INVALID and "not finite" in last_error()


def test_which_is_judged_before_any_handle_is_read():
    for which in ((2, 0), (-2, 0), (5, 5), (-1, 2)):
        assert call(which=which) == INVALID and "outside [-1, nsets)" in last_error() and ENTRY in last_error(), which
    # a named entry of sets[] that is NULL
    assert call(which=(0, -1)) == INVALID and "NULL" in last_error() and ENTRY in last_error()
    # nothing named: the NULL index handle is what is left to refuse - also for nq == 0, whose weights and which may be NULL
    assert call(which=(-1, -1)) == INVALID and "NULL argument" in last_error() and ENTRY in last_error()
    assert call(nq=0, which=(), weights=(), nulls=("which", "weights")) == INVALID and "NULL argument" in last_error()


def test_the_python_surface_checks_its_arrays_without_a_device():
    import theoremsearch_amd as ts
    host = ts.TheoremIndex(64, 128, device=-1)
    with pytest.raises(ValueError):                                  # the host-only index has no filters: refused, not answered by another path
        host.search_biased_rowsets(np.zeros((2, 128), np.float32), 4, np.zeros(64, np.float32), [0.0, 0.5], [], [-1, -1])
    with pytest.raises(ValueError, match="weights has 3 entries for 2 queries"):
        ts.TheoremIndex._weights_arg([0.0, 0.5, 1.0], 2)


@pytest.mark.gpu
def test_no_queries_is_ts_ok_on_a_live_index():
    import theoremsearch_amd as ts
    ix =ts.TheoremIndex(64, 128, dtype="bf16", metric="ip")
    ix.upload(np.zeros((64, 128), np.float32))
    b = np.zeros(64, dtype=np.float32)
    st = _ffi.RowsetsStats()
    q = np.zeros((1, 128), dtype=np.float32)
    out_s, out_i = np.zeros((1, 4), np.float32), np.zeros((1, 4), np.int64)
    rc = _ffi.load().ts_search_biased_rowsets(ix.handle, _ffi.as_ptr(q), 0, 0, 0, 4, _ffi.as_ptr(b), 0, None, None, 0, None, _ffi.as_ptr(out_s), None,
                                              _ffi.as_ptr(out_i), 0, None, 0, C.byref(st))
    assert rc == 0 and st.pass_queries == 0 and st.scan_queries == 0
