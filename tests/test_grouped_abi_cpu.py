"""The grouped search's entries without a device (include/tsearch.h: ts_search_grouped, ts_collapse_topk, ts_rowset_exclude,
ts_group_depth): malformed arguments are TS_ERR_INVALID with a message, the compute entries fail loudly instead of falling
back, and ts_group_depth answers."""
import ctypes as C

import numpy as np
import pytest

from conftest import gpu_available
from theoremsearch_amd import _ffi

INVALID, NODEVICE = -1, -4


def last_error():
    return _ffi.load().ts_last_error().decode()


def collapse(nq=1, k_in=4, k_out=4, n=8, row_offset=0, nulls=()):
    s = np.zeros((max(nq, 1), max(k_in, 1)), dtype=np.float32)
    i = np.zeros((max(nq, 1), max(k_in, 1)), dtype=np.int64)
    col = np.zeros(max(n, 1), dtype=np.int32)
    os_ = np.zeros((max(nq, 1), max(k_out, 1)), dtype=np.float32)
    oi = np.zeros((max(nq, 1), max(k_out, 1)), dtype=np.int64)
    ptr = {"scores": _ffi.as_ptr(s), "idx": _ffi.as_ptr(i), "column": _ffi.as_ptr(col), "out_scores": _ffi.as_ptr(os_), "out_idx": _ffi.as_ptr(oi)}
    for name in nulls:
        ptr[name] = None
    return _ffi.load().ts_collapse_topk(0, ptr["scores"], ptr["idx"], nq, k_in, k_out, ptr["column"], n, row_offset, ptr["out_scores"],
                                        ptr["out_idx"], None, None, None, 0, None)


def test_group_depth_answers_without_a_device():
    import theoremsearch_amd as ts
    lib = _ffi.load()
    for k in range(1, _ffi.TS_MAX_K + 1):
        first, deep = ts.group_depth(k)
        assert (first, deep) == (min(256, max(2 * k, k + 16)), 256)
    first = C.c_int32(-1)
    assert lib.ts_group_depth(10, C.byref(first), None) == 0 and first.value == 26       # each pointer may be NULL
    assert lib.ts_group_depth(10, None, None) == 0
    for k in (0, -1, 257):
        assert lib.ts_group_depth(k, C.byref(first), None) == INVALID
        assert "k outside" in last_error()
        with pytest.raises(_ffi.TSearchError):
            ts.group_depth(k)


def test_collapse_refuses_malformed_arguments_with_a_message():
    for name in ("scores", "idx", "column", "out_scores", "out_idx"):
        assert collapse(nulls=(name,)) == INVALID and "NULL argument" in last_error()
    for bad, text in ((dict(nq=-1), "nq is negative"), (dict(k_in=0), "k_in outside"), (dict(k_in=257), "k_in outside"),
                      (dict(k_out=0), "k_out is less than 1"), (dict(n=-1), "n is negative"), (dict(row_offset=-5), "row_offset is negative")):
        assert collapse(**bad) == INVALID, bad
        assert text in last_error() and "ts_collapse_topk" in last_error()
    assert collapse(nq=0) == 0                           # nothing to do needs no device


def test_search_grouped_and_exclude_refuse_null_handles_and_bad_sizes():
    lib = _ffi.load()
    q = np.zeros((1, 8), dtype=np.float32)
    s, i = np.zeros((1, 4), dtype=np.float32), np.zeros((1, 4), dtype=np.int64)
    stats = _ffi.GroupedStats()
    assert lib.ts_search_grouped(None, _ffi.as_ptr(q), 0, 0, 1, 4, None, 0, None, _ffi.as_ptr(s), _ffi.as_ptr(i), None, 0, None, 0,
                                 C.byref(stats)) == INVALID
    assert "NULL argument" in last_error() and "ts_search_grouped" in last_error()
    out = C.c_void_p(123)
    codes = np.zeros(300, dtype=np.int32)
    rows = np.zeros(300, dtype=np.int64)
    assert lib.ts_rowset_exclude(None, 0, None, None, 0, None, 0, C.byref(out), None) == INVALID
    assert "NULL argument" in last_error() and out.value is None
    # the sizes are judged before the handles
    assert lib.ts_rowset_exclude(None, 0, None, _ffi.as_ptr(codes), 257, None, 0, C.byref(out), None) == INVALID
    assert "ncodes outside" in last_error()
    assert lib.ts_rowset_exclude(None, 0, None, None, 0, _ffi.as_ptr(rows), -1, C.byref(out), None) == INVALID
    assert "nrows outside" in last_error()
    for k in (0, 257):
        assert lib.ts_search_grouped(None, _ffi.as_ptr(q), 0, 0, 1, k, None, 0, None, _ffi.as_ptr(s), _ffi.as_ptr(i), None, 0, None, 0,
                                     C.byref(stats)) == INVALID
        assert "k outside" in last_error()


@pytest.mark.skipif(gpu_available(), reason="checks the no-device behaviour")
def test_collapse_fails_loudly_without_a_device():
    import theoremsearch_amd as ts
    assert _ffi.device_count() == 0
    assert collapse() == NODEVICE and "no CPU path" in last_error()
    with pytest.raises(_ffi.TSearchError) as e:
        ts.collapse_topk(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int64), np.zeros(4, np.int32), 3)
    assert e.value.code == NODEVICE
    with pytest.raises(_ffi.TSearchError):
        ts.MetaTable.from_columns([np.zeros(4, np.int32)])           # no table, so no exclusion, without a device
