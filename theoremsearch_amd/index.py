"""TheoremIndex: the [N x d] theorem-embedding matrix resident in HBM, and exact top-k search.

Host-side mirror of the two-line search idiom of the reference apps::

    cosine_scores = util.cos_sim(query_emb, embeddings_db)[0]           # app_showcase_model.py:93
    top = torch.topk(cosine_scores, k=min(200, N), sorted=True)          # app_showcase_model.py:96
    top_indices = np.argsort(-cosine_scores.cpu())[:5]                  # app_scratchpad.py:130

and of ``ORDER BY e.embedding <#> q ASC LIMIT k`` (streamlit_app.py:282-283).  All arithmetic
runs in libtsearch.so's HIP kernels; numpy is only the container of host inputs and results.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _ffi
from ._ffi import TS_ALGO_AUTO, TS_ALGO_MFMA, TS_ALGO_SCAN, TS_BF16, TS_F32, TS_METRIC_COS, TS_METRIC_IP
from .metadata import RowSet

_DTYPES = {"f32": TS_F32, "fp32": TS_F32, "float32": TS_F32, "bf16": TS_BF16, "bfloat16": TS_BF16}
_METRICS = {"ip": TS_METRIC_IP, "dot": TS_METRIC_IP, "cos": TS_METRIC_COS, "cosine": TS_METRIC_COS}
_ALGOS = {"auto": TS_ALGO_AUTO, "scan": TS_ALGO_SCAN, "mfma": TS_ALGO_MFMA}


def _host_rows(x) -> np.ndarray:
    """numpy float32 / uint16(bf16 bits) 2-D, C-contiguous; accepts lists and CPU torch tensors."""
    if hasattr(x, "detach") and hasattr(x, "cpu"):          # torch.Tensor without importing torch
        t = x.detach().cpu()
        if str(t.dtype) == "torch.bfloat16":
            x = t.view(dtype=__import__("torch").int16).numpy().view(np.uint16)
        else:
            x = t.float().numpy()
    a = np.asarray(x)
    if a.dtype != np.uint16:
        a = a.astype(np.float32, copy=False)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2:
        raise ValueError("expected a 1-D or 2-D array of embeddings")
    return np.ascontiguousarray(a)


class TheoremIndex:
    """Device-resident embedding matrix with brute-force exact top-k search."""

    _cpu_rows = None          # only the explicit host-only index (device=-1) holds its rows in a numpy array

    def __init__(self, n: int, d: int, dtype: str = "f32", metric: str = "cos", device: int = 0,
                 row_offset: int = 0):
        self._lib = _ffi.load()
        self._h = C.c_void_p()
        self.n, self.d = int(n), int(d)
        self.dtype, self.metric, self.device = dtype, metric, int(device)
        self._cpu_rows = None
        if self.device == -1:
            # The explicit host-only index (BASELINE.json configs[0]: the reference's CPU-runnable plumbing case,
            # compare_embeddings.py:55-92): rows stay in a numpy array, `search` calls ts_search_cpu.  Never chosen by the
            # library itself - a missing GPU still raises for every other device number - and only upload / search / close exist.
            _DTYPES[dtype], _METRICS[metric]                      # validate the names
            self._cpu_rows = np.zeros((self.n, self.d), dtype=np.float32)
            self.row_offset = int(row_offset)
            return
        _ffi.check(self._lib.ts_index_create(self.device, self.n, self.d, _DTYPES[dtype], _METRICS[metric],
                                             C.byref(self._h)))
        self.row_offset = 0
        if row_offset:
            self.set_row_offset(row_offset)

    # -- construction ---------------------------------------------------------------------
    @classmethod
    def from_embeddings(cls, embeddings, dtype: str = "f32", metric: str = "cos", device: int = 0,
                        row_offset: int = 0) -> "TheoremIndex":
        """Build from a host matrix (numpy, list of lists, or the CPU tensor that
        ``torch.load('corpus_embeddings.pt')`` returns, app_showcase_model.py:52)."""
        rows = _host_rows(embeddings)
        ix = cls(rows.shape[0], rows.shape[1], dtype=dtype, metric=metric, device=device, row_offset=row_offset)
        ix.upload(rows, 0)
        return ix

    def view(self) -> "TheoremIndex":
        """A second handle on the same rows (no copy) with its own stream and scratch: searches through the two handles
        can be in flight at once on two streams (serving loops over independent batches).  Read-only; close it before
        the index it views."""
        v = object.__new__(TheoremIndex)
        v._lib, v._h = self._lib, C.c_void_p()
        v.n, v.d, v.dtype, v.metric, v.device, v.row_offset = self.n, self.d, self.dtype, self.metric, self.device, self.row_offset
        v._parent = self                      # keeps the owner of the rows alive
        _ffi.check(self._lib.ts_index_view(self._h, C.byref(v._h)))
        return v

    def subset(self, rows_or_mask) -> "TheoremIndex":
        """A new index over a subset of this one's rows (bool mask of length n, or ascending global row ids).
        Its searches return this index's ids: the filtered search for query batches / long-lived filters."""
        a = np.asarray(rows_or_mask)
        if a.dtype == bool:
            if a.shape[0] != self.n:
                raise ValueError(f"mask has {a.shape[0]} entries, index has {self.n} rows")
            a = np.flatnonzero(a) + self.row_offset
        ids = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
        sub = object.__new__(TheoremIndex)
        sub._lib, sub._h = self._lib, C.c_void_p()
        sub.n, sub.d, sub.dtype, sub.metric, sub.device, sub.row_offset = int(ids.shape[0]), self.d, self.dtype, self.metric, self.device, 0
        _ffi.check(self._lib.ts_index_subset(self._h, _ffi.as_ptr(ids), ids.shape[0], C.byref(sub._h)))
        return sub

    def upload(self, rows, row0: int = 0) -> None:
        rows = _host_rows(rows)
        if rows.shape[1] != self.d:
            raise ValueError(f"rows have d={rows.shape[1]}, index has d={self.d}")
        if self._cpu_rows is not None:
            if row0 < 0 or row0 + rows.shape[0] > self.n:
                raise ValueError("rows outside the index")
            vals = rows if rows.dtype == np.float32 else (rows.astype(np.uint32) << np.uint32(16)).view(np.float32)
            self._cpu_rows[row0:row0 + rows.shape[0]] = vals
            return
        _ffi.check(self._lib.ts_index_upload(self._h, _ffi.as_ptr(rows), _ffi.np_dtype_code(rows), int(row0),
                                             rows.shape[0]))

    def upload_device(self, dev_ptr: int, src_dtype: str, src_ld: int, row0: int, nrows: int, stream: int = 0) -> None:
        """Rows already in device memory (e.g. ``tensor.data_ptr()`` of the encoder output)."""
        _ffi.check(self._lib.ts_index_upload_device(self._h, C.c_void_p(dev_ptr), _DTYPES[src_dtype], int(src_ld),
                                                    int(row0), int(nrows), C.c_void_p(stream)))

    def reserve(self, capacity: int) -> None:
        """Make room for ``capacity`` rows (no change to ``n``): later `append` calls then never move the rows."""
        _ffi.check(self._lib.ts_index_reserve(self._h, int(capacity)))

    def append(self, rows) -> int:
        """Add rows behind the last one (new ``slogan_id``s of the upsert pipeline, ec2/generate_embeddings/__main__.py:85-99);
        returns the global id of the first new row.  The allocation grows 1.5x when it is full."""
        rows = _host_rows(rows)
        if rows.shape[1] != self.d:
            raise ValueError(f"rows have d={rows.shape[1]}, index has d={self.d}")
        first = C.c_int64(-1)
        _ffi.check(self._lib.ts_index_append(self._h, _ffi.as_ptr(rows), _ffi.np_dtype_code(rows), rows.shape[0],
                                             C.byref(first)))
        self.n += rows.shape[0]
        return first.value

    def append_device(self, dev_ptr: int, src_dtype: str, src_ld: int, nrows: int, stream: int = 0) -> int:
        """`append` for rows already in device memory (the encoder output)."""
        first = C.c_int64(-1)
        _ffi.check(self._lib.ts_index_append_device(self._h, C.c_void_p(dev_ptr), _DTYPES[src_dtype], int(src_ld), int(nrows),
                                                    C.c_void_p(stream), C.byref(first)))
        self.n += int(nrows)
        return first.value

    def attach_device(self, dev_ptr: int, capacity_rows: int, keep_alive=None) -> None:
        """Adopt rows already in device memory (zero-copy; e.g. ``tensor.data_ptr()`` of an encoder output in the index's
        dtype with ``capacity_rows >= n`` rounded up to 256).  ``keep_alive``: an object to hold on to (the tensor)."""
        _ffi.check(self._lib.ts_index_attach_device(self._h, C.c_void_p(dev_ptr), int(capacity_rows)))
        self._attached = keep_alive

    def set_row_offset(self, offset: int) -> None:
        _ffi.check(self._lib.ts_index_set_row_offset(self._h, int(offset)))
        self.row_offset = int(offset)

    def set_option(self, name: str, value: Optional[int]) -> None:
        """Tuning / diagnostic knob of this handle (``"TS_MFMA_FIRST_ROWS"`` ...); ``None`` restores the default.
        The knobs' initial values come from the environment when the handle is created."""
        if value is None:
            _ffi.check(self._lib.ts_index_reset_option(self._h, name.encode()))
        else:
            _ffi.check(self._lib.ts_index_set_option(self._h, name.encode(), int(value)))

    def download(self, row0: int = 0, nrows: Optional[int] = None) -> np.ndarray:
        """Stored rows (normalised / bf16-rounded as the kernels see them)."""
        nrows = self.n - row0 if nrows is None else nrows
        out = np.empty((nrows, self.d), dtype=np.uint16 if _DTYPES[self.dtype] == TS_BF16 else np.float32)
        _ffi.check(self._lib.ts_index_download(self._h, _ffi.as_ptr(out), int(row0), int(nrows)))
        return out

    def synchronize(self) -> None:
        """Wait for everything this handle has enqueued (uploads / searches with device buffers return early)."""
        _ffi.check(self._lib.ts_index_synchronize(self._h))

    @property
    def stream(self) -> int:
        s = C.c_void_p()
        _ffi.check(self._lib.ts_index_stream(self._h, C.byref(s)))
        return s.value or 0

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def info(self) -> dict:
        """Shape and placement of the rows as the kernels see them (``ts_index_info``): ``ld`` = row stride in
        elements, ``rows_ptr`` = device address of row 0."""
        n, ld, off = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        d, dt, me = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        rows = C.c_void_p()
        _ffi.check(self._lib.ts_index_info(self._h, C.byref(n), C.byref(d), C.byref(dt), C.byref(me), C.byref(ld), C.byref(off),
                                           C.byref(rows)))
        return {"n": n.value, "d": d.value, "dtype": dt.value, "metric": me.value, "ld": ld.value, "row_offset": off.value,
                "rows_ptr": rows.value or 0}

    # -- search -----------------------------------------------------------------------------
    def search(self, queries, k: int, algo: str = "auto", return_stats: bool = False, mask=None):
        """Exact top-k.  Returns ``(scores [nq x k] float32, indices [nq x k] int64)`` ordered by
        score descending then index ascending; padding is ``(-inf, -1)``.  ``mask`` (bool per row)
        restricts the search to the rows where it is true (metadata filters): the k best allowed rows.
        ``mask`` may also be a `metadata.RowSet` (a mask evaluated on the device, with its count): the same
        answer, and a query batch behind it runs on the matrix path when it allows a tenth of the rows."""
        q = _host_rows(queries)
        if q.shape[1] != self.d:
            raise ValueError(f"queries have d={q.shape[1]}, index has d={self.d}")
        nq, k = q.shape[0], int(k)
        scores = np.empty((nq, k), dtype=np.float32)
        idx = np.empty((nq, k), dtype=np.int64)
        if self._cpu_rows is not None:
            if mask is not None or algo != "auto":
                raise ValueError("the host-only index (device=-1) has one algorithm and no filters")
            _ffi.check(self._lib.ts_search_cpu(_ffi.as_ptr(self._cpu_rows), TS_F32, self.n, self.d, _DTYPES[self.dtype],
                                               _METRICS[self.metric], _ffi.as_ptr(q), _ffi.np_dtype_code(q), nq, k,
                                               _ffi.as_ptr(scores), _ffi.as_ptr(idx), 0))
            if self.row_offset:
                idx[idx >= 0] += self.row_offset
            return (scores, idx, {"algo": 0, "levels": 0, "fallback_queries": 0, "candidates": 0, "screened": 0}) if return_stats else (scores, idx)
        if mask is not None:
            stats = _ffi.SearchStats()
            if isinstance(mask, RowSet):
                _ffi.check(self._lib.ts_search_rowset(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, nq, k, mask.handle,
                                                      _ffi.as_ptr(scores), _ffi.as_ptr(idx), 0, None, _ALGOS[algo],
                                                      C.byref(stats)))
            else:
                m = np.asarray(mask, dtype=bool).reshape(-1)
                if m.shape[0] != self.n:
                    raise ValueError(f"mask has {m.shape[0]} entries, index has {self.n} rows")
                bits = np.packbits(m, bitorder="little")
                words = np.zeros((self.n + 31) // 32 * 4, dtype=np.uint8)
                words[: bits.shape[0]] = bits
                words = words.view(np.uint32)
                _ffi.check(self._lib.ts_search_filtered_ex(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, nq, k,
                                                           _ffi.as_ptr(words), 0, _ffi.as_ptr(scores), _ffi.as_ptr(idx), 0, None,
                                                           _ALGOS[algo], C.byref(stats)))
            if return_stats:
                return scores, idx, {"algo": stats.algo, "levels": stats.levels,
                                     "fallback_queries": stats.fallback_queries, "candidates": stats.candidates,
                                     "screened": stats.screened}
            return scores, idx
        stats = _ffi.SearchStats()
        _ffi.check(self._lib.ts_search_ex(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, nq, k,
                                          _ffi.as_ptr(scores), _ffi.as_ptr(idx), 0, None, _ALGOS[algo],
                                          C.byref(stats)))
        if return_stats:
            return scores, idx, {"algo": stats.algo, "levels": stats.levels,
                                 "fallback_queries": stats.fallback_queries, "candidates": stats.candidates,
                                 "screened": stats.screened}
        return scores, idx

    def search_device(self, q_ptr: int, q_dtype: str, nq: int, k: int, out_scores_ptr: int, out_idx_ptr: int,
                      stream: int = 0, algo: str = "auto", mask_ptr: int = 0, rowset: Optional[RowSet] = None) -> None:
        """Asynchronous search on device buffers (queries [nq x d] dense; outputs [nq x k] f32 / i64),
        enqueued on ``stream`` (0 = the index's own stream).  ``mask_ptr``: device uint32 bitmask
        (ceil(n / 32) words) restricting the rows, see `search` - a bare device mask runs on the scan;
        ``rowset``: a `metadata.RowSet` instead, whose known count lets ``algo`` decide as for a host mask (keep it
        open until the enqueued work has run).
        Queries that already have the form the matrix kernels multiply (the index's dtype, an inner-product index, a
        whole launch's worth: 64 / 128 / 192 / 256 of them) are read in place - keep them unchanged until the enqueued work
        has run (work enqueued later on the same stream is ordered behind it anyway)."""
        if rowset is not None:
            _ffi.check(self._lib.ts_search_rowset(self._h, C.c_void_p(q_ptr), _DTYPES[q_dtype], 1, int(nq), int(k), rowset.handle,
                                                  C.c_void_p(out_scores_ptr), C.c_void_p(out_idx_ptr), 1, C.c_void_p(stream),
                                                  _ALGOS[algo], None))
            return
        if mask_ptr:
            _ffi.check(self._lib.ts_search_filtered(self._h, C.c_void_p(q_ptr), _DTYPES[q_dtype], 1, int(nq), int(k),
                                                    C.c_void_p(mask_ptr), 1, C.c_void_p(out_scores_ptr),
                                                    C.c_void_p(out_idx_ptr), 1, C.c_void_p(stream)))
            return
        _ffi.check(self._lib.ts_search_ex(self._h, C.c_void_p(q_ptr), _DTYPES[q_dtype], 1, int(nq), int(k),
                                          C.c_void_p(out_scores_ptr), C.c_void_p(out_idx_ptr), 1,
                                          C.c_void_p(stream), _ALGOS[algo], None))

    # -- a row set per query ----------------------------------------------------------------
    @staticmethod
    def _rowsets_args(rowsets, which, nq):
        """The handle array and the ``which`` array of ``ts_search_rowsets`` (both must outlive the call)."""
        rowsets = list(rowsets)
        if len(rowsets) > _ffi.TS_MAX_ROWSETS:
            raise ValueError(f"{len(rowsets)} row sets in one call, at most {_ffi.TS_MAX_ROWSETS}")
        for r in rowsets:
            if r is not None and not isinstance(r, RowSet):
                raise TypeError("rowsets holds metadata.RowSet objects (MetaTable.eval / MetaTable.eval_many)")
        w = np.ascontiguousarray(np.asarray(which).reshape(-1), dtype=np.int32)
        if w.shape[0] != nq:
            raise ValueError(f"which has {w.shape[0]} entries for {nq} queries")
        handles = (C.c_void_p * max(len(rowsets), 1))(*[r.handle if r is not None else None for r in rowsets])
        return rowsets, handles, w

    @staticmethod
    def _rowsets_stats(stats) -> dict:
        return {"algo": stats.algo, "sets_used": stats.sets_used, "pass_queries": stats.pass_queries, "scan_queries": stats.scan_queries,
                "scan_calls": stats.scan_calls, "fallback_queries": stats.fallback_queries, "candidates": stats.candidates}

    def search_rowsets(self, queries, k: int, rowsets, which, algo: str = "auto", return_stats: bool = False):
        """`search` with a row set per query (``ts_search_rowsets``): query ``i`` is searched behind ``rowsets[which[i]]``, or
        behind no filter where ``which[i] == -1``.  ``rowsets``: a sequence of `metadata.RowSet` (at most 256); ``which``: an int
        array, one entry per query.  Each output row is what `search` returns for that query alone with ``mask=`` its set; a batch
        with several dense sets crosses the corpus once.  Returns ``(scores, indices)`` and, with ``return_stats``, the routing's
        counters (``algo, sets_used, pass_queries, scan_queries, scan_calls, fallback_queries, candidates``)."""
        if self._cpu_rows is not None:
            raise ValueError("the host-only index (device=-1) has one algorithm and no filters")
        q = _host_rows(queries)
        if q.shape[1] != self.d:
            raise ValueError(f"queries have d={q.shape[1]}, index has d={self.d}")
        nq, k = q.shape[0], int(k)
        rowsets, handles, w = self._rowsets_args(rowsets, which, nq)
        scores = np.empty((nq, max(k, 0)), dtype=np.float32)
        idx = np.empty((nq, max(k, 0)), dtype=np.int64)
        stats = _ffi.RowsetsStats()
        _ffi.check(self._lib.ts_search_rowsets(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, nq, k, handles, len(rowsets),
                                               _ffi.as_ptr(w), _ffi.as_ptr(scores), _ffi.as_ptr(idx), 0, None, _ALGOS[algo], C.byref(stats)))
        return (scores, idx, self._rowsets_stats(stats)) if return_stats else (scores, idx)

    def search_rowsets_device(self, q_ptr: int, q_dtype: str, nq: int, k: int, rowsets, which, out_scores_ptr: int, out_idx_ptr: int,
                              stream: int = 0, algo: str = "auto") -> dict:
        """`search_rowsets` on device buffers (queries [nq x d] dense; outputs [nq x k] f32 / i64) on ``stream`` (0 = the index's
        own); ``which`` stays a host array.  Unlike `search_device` the call WAITS for its pass - the re-run list is read back
        per block of 256 queries - and returns the routing's counters."""
        rowsets, handles, w = self._rowsets_args(rowsets, which, int(nq))
        stats = _ffi.RowsetsStats()
        _ffi.check(self._lib.ts_search_rowsets(self._h, C.c_void_p(q_ptr), _DTYPES[q_dtype], 1, int(nq), int(k), handles, len(rowsets),
                                               _ffi.as_ptr(w), C.c_void_p(out_scores_ptr), C.c_void_p(out_idx_ptr), 1, C.c_void_p(stream),
                                               _ALGOS[algo], C.byref(stats)))
        return self._rowsets_stats(stats)

    # -- a weight and a row set per query ---------------------------------------------------
    @staticmethod
    def _weights_arg(weights, nq):
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
        if w.shape[0] != nq:
            raise ValueError(f"weights has {w.shape[0]} entries for {nq} queries")
        return w

    def search_biased_rowsets(self, queries, k: int, bias, weights, rowsets, which, algo: str = "auto", return_stats: bool = False):
        """`search_biased` with a weight and a row set per query (``ts_search_biased_rowsets``): query ``i`` is ranked by
        ``score + weights[i] * bias[row]`` over the rows ``rowsets[which[i]]`` allows (all rows where ``which[i] == -1``).
        ``bias``: float32 per row of this index, one array for the call; ``weights``: one finite float per query; ``rowsets`` /
        ``which``: as for `search_rowsets`.  Each output row is what `search_biased` returns for that query alone with its weight
        and ``mask=`` its set; a batch whose queries differ in filter or weight crosses the corpus once.  Returns ``(weighted
        scores, raw similarities, indices)`` and, with ``return_stats``, the routing's counters (those of `search_rowsets`)."""
        if self._cpu_rows is not None:
            raise ValueError("the host-only index (device=-1) has one algorithm and no filters")
        q = _host_rows(queries)
        if q.shape[1] != self.d:
            raise ValueError(f"queries have d={q.shape[1]}, index has d={self.d}")
        b = np.ascontiguousarray(np.asarray(bias, dtype=np.float32).reshape(-1))
        if b.shape[0] != self.n:
            raise ValueError(f"bias has {b.shape[0]} entries, index has {self.n} rows")
        nq, k = q.shape[0], int(k)
        rowsets, handles, w = self._rowsets_args(rowsets, which, nq)
        wt = self._weights_arg(weights, nq)
        scores = np.empty((nq, max(k, 0)), dtype=np.float32)
        sims = np.empty((nq, max(k, 0)), dtype=np.float32)
        idx = np.empty((nq, max(k, 0)), dtype=np.int64)
        stats = _ffi.RowsetsStats()
        _ffi.check(self._lib.ts_search_biased_rowsets(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, nq, k, _ffi.as_ptr(b), 0,
                                                      _ffi.as_ptr(wt), handles, len(rowsets), _ffi.as_ptr(w), _ffi.as_ptr(scores),
                                                      _ffi.as_ptr(sims), _ffi.as_ptr(idx), 0, None, _ALGOS[algo], C.byref(stats)))
        return (scores, sims, idx, self._rowsets_stats(stats)) if return_stats else (scores, sims, idx)

    def search_biased_rowsets_device(self, q_ptr: int, q_dtype: str, nq: int, k: int, bias_ptr: int, weights, rowsets, which,
                                     out_scores_ptr: int, out_sims_ptr: int, out_idx_ptr: int, stream: int = 0, algo: str = "auto") -> dict:
        """`search_biased_rowsets` on device buffers (queries [nq x d] dense; bias float32 [n]; outputs [nq x k] f32 / f32 / i64,
        ``out_sims_ptr`` may be 0) on ``stream`` (0 = the index's own); ``weights`` and ``which`` stay host arrays.  Like
        `search_rowsets_device` the call WAITS for its pass and returns the routing's counters."""
        rowsets, handles, w = self._rowsets_args(rowsets, which, int(nq))
        wt = self._weights_arg(weights, int(nq))
        stats = _ffi.RowsetsStats()
        _ffi.check(self._lib.ts_search_biased_rowsets(self._h, C.c_void_p(q_ptr), _DTYPES[q_dtype], 1, int(nq), int(k), C.c_void_p(bias_ptr),
                                                      1, _ffi.as_ptr(wt), handles, len(rowsets), _ffi.as_ptr(w), C.c_void_p(out_scores_ptr),
                                                      C.c_void_p(out_sims_ptr) if out_sims_ptr else None, C.c_void_p(out_idx_ptr), 1,
                                                      C.c_void_p(stream), _ALGOS[algo], C.byref(stats)))
        return self._rowsets_stats(stats)

    # -- grouped search ---------------------------------------------------------------------
    @staticmethod
    def _group_column(meta, column) -> int:
        return meta.col[column] if isinstance(column, str) else int(column)

    def search_grouped(self, queries, k: int, meta, column, mask=None, algo: str = "auto", return_groups: bool = False,
                       return_stats: bool = False):
        """The ``k`` best distinct groups, one row per group (``ts_search_grouped``): ``SELECT DISTINCT ON (group)`` before the
        ranking, exactly, however large a group is.  The group of a row is its value in scalar column ``column`` (a name or a
        number) of the `metadata.MetaTable` ``meta``; a NULL is a group of its own.  ``mask``: a `metadata.RowSet` or None.
        Returns ``(scores, indices)`` shaped and ordered like `search` - each row is its group's best row - then the group codes
        ``int32 [nq x k]`` with ``return_groups`` and the ladder's counters (``algo, depth, deep_queries, excluded_queries,
        exclusion_passes``) with ``return_stats``.  Padding is ``(-inf, -1, NULL)``."""
        if self._cpu_rows is not None:
            raise ValueError("the host-only index (device=-1) has no grouped search")
        if mask is not None and not isinstance(mask, RowSet):
            raise TypeError("search_grouped takes a metadata.RowSet as its mask (MetaTable.eval / MetaTable.exclude), not a bare mask")
        q = _host_rows(queries)
        if q.shape[1] != self.d:
            raise ValueError(f"queries have d={q.shape[1]}, index has d={self.d}")
        nq, k = q.shape[0], int(k)
        scores = np.empty((nq, max(k, 0)), dtype=np.float32)
        idx = np.empty((nq, max(k, 0)), dtype=np.int64)
        groups = np.empty((nq, max(k, 0)), dtype=np.int32)
        stats = _ffi.GroupedStats()
        _ffi.check(self._lib.ts_search_grouped(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, nq, k, meta._h,
                                               self._group_column(meta, column), mask.handle if mask is not None else None,
                                               _ffi.as_ptr(scores), _ffi.as_ptr(idx), _ffi.as_ptr(groups), 0, None, _ALGOS[algo],
                                               C.byref(stats)))
        out = (scores, idx)
        if return_groups:
            out += (groups,)
        if return_stats:
            out += ({"algo": stats.algo, "depth": stats.depth, "deep_queries": stats.deep_queries,
                     "excluded_queries": stats.excluded_queries, "exclusion_passes": stats.exclusion_passes},)
        return out

    def search_grouped_device(self, q_ptr: int, q_dtype: str, nq: int, k: int, meta, column, out_scores_ptr: int, out_idx_ptr: int,
                              out_groups_ptr: int = 0, stream: int = 0, algo: str = "auto", rowset: Optional[RowSet] = None) -> dict:
        """`search_grouped` on device buffers (queries [nq x d] dense; outputs [nq x k] f32 / i64 / i32, ``out_groups_ptr`` may be
        0) on ``stream`` (0 = the index's own).  Unlike `search_device` the call WAITS for its result - the ladder reads its
        certificates back between the stages - and returns the ladder's counters."""
        stats = _ffi.GroupedStats()
        _ffi.check(self._lib.ts_search_grouped(self._h, C.c_void_p(q_ptr), _DTYPES[q_dtype], 1, int(nq), int(k), meta._h,
                                               self._group_column(meta, column), rowset.handle if rowset is not None else None,
                                               C.c_void_p(out_scores_ptr), C.c_void_p(out_idx_ptr),
                                               C.c_void_p(out_groups_ptr) if out_groups_ptr else None, 1, C.c_void_p(stream),
                                               _ALGOS[algo], C.byref(stats)))
        return {"algo": stats.algo, "depth": stats.depth, "deep_queries": stats.deep_queries,
                "excluded_queries": stats.excluded_queries, "exclusion_passes": stats.exclusion_passes}

    def search_biased(self, queries, k: int, bias, weight: float, mask=None, algo: Optional[str] = None,
                      return_stats: bool = False):
        """Top-k of ``score + weight * bias[row]`` over all rows (all rows ``mask`` allows): the citation-weighted
        ranking of streamlit_app.py:348-364 without its candidate pool.  ``bias``: float32 per row of this index.
        Returns ``(weighted scores, raw similarities, indices)``, each ``[nq x k]``.
        ``algo=None`` is ``ts_search_biased`` (the scan); ``"scan" | "mfma" | "auto"`` go through ``ts_search_biased_ex``:
        ``"mfma"`` is the batched matrix search (one corpus pass per 256 queries; refused where it is not served),
        ``"auto"`` takes it for a batch of more than 4 queries (an fp32 index: more than 8).  ``return_stats`` appends the call's counters.
        ``mask`` may be a `metadata.RowSet`: always ``ts_search_biased_rowset`` (``algo=None``: the scan, the same kernel)."""
        q = _host_rows(queries)
        if q.shape[1] != self.d:
            raise ValueError(f"queries have d={q.shape[1]}, index has d={self.d}")
        b = np.ascontiguousarray(np.asarray(bias, dtype=np.float32).reshape(-1))
        if b.shape[0] != self.n:
            raise ValueError(f"bias has {b.shape[0]} entries, index has {self.n} rows")
        nq, k = q.shape[0], int(k)
        scores = np.empty((nq, k), dtype=np.float32)
        sims = np.empty((nq, k), dtype=np.float32)
        idx = np.empty((nq, k), dtype=np.int64)
        words = None
        if isinstance(mask, RowSet):
            stats = _ffi.SearchStats()
            _ffi.check(self._lib.ts_search_biased_rowset(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, nq, k, _ffi.as_ptr(b), 0,
                                                         float(weight), mask.handle, _ffi.as_ptr(scores), _ffi.as_ptr(sims),
                                                         _ffi.as_ptr(idx), 0, None, _ALGOS[algo or "scan"], C.byref(stats)))
            if return_stats:
                return scores, sims, idx, {"algo": stats.algo, "levels": stats.levels, "fallback_queries": stats.fallback_queries,
                                           "candidates": stats.candidates, "screened": stats.screened}
            return scores, sims, idx
        if mask is not None:
            m = np.asarray(mask, dtype=bool).reshape(-1)
            if m.shape[0] != self.n:
                raise ValueError(f"mask has {m.shape[0]} entries, index has {self.n} rows")
            bits = np.packbits(m, bitorder="little")
            words = np.zeros((self.n + 31) // 32 * 4, dtype=np.uint8)
            words[: bits.shape[0]] = bits
        if algo is None:
            _ffi.check(self._lib.ts_search_biased(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, nq, k, _ffi.as_ptr(b), 0,
                                                  float(weight), _ffi.as_ptr(words) if words is not None else None, 0,
                                                  _ffi.as_ptr(scores), _ffi.as_ptr(sims), _ffi.as_ptr(idx), 0, None))
            stats = _ffi.SearchStats()
            stats.algo = _ffi.TS_ALGO_SCAN
        else:
            stats = _ffi.SearchStats()
            _ffi.check(self._lib.ts_search_biased_ex(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, nq, k, _ffi.as_ptr(b), 0,
                                                     float(weight), _ffi.as_ptr(words) if words is not None else None, 0,
                                                     _ffi.as_ptr(scores), _ffi.as_ptr(sims), _ffi.as_ptr(idx), 0, None,
                                                     _ALGOS[algo], C.byref(stats)))
        if return_stats:
            return scores, sims, idx, {"algo": stats.algo, "levels": stats.levels, "fallback_queries": stats.fallback_queries,
                                       "candidates": stats.candidates, "screened": stats.screened}
        return scores, sims, idx

    def search_biased_device(self, q_ptr: int, q_dtype: str, nq: int, k: int, bias_ptr: int, weight: float, out_scores_ptr: int,
                             out_sims_ptr: int, out_idx_ptr: int, stream: int = 0, algo: str = "auto") -> None:
        """Asynchronous `search_biased` on device buffers (queries [nq x d]; bias float32 [n]; outputs [nq x k] f32 / f32 /
        i64; ``out_sims_ptr`` may be 0), enqueued on ``stream`` (0 = the index's own).  Always ``ts_search_biased_ex``:
        ``algo`` defaults to ``"auto"`` as in `search_device` - unlike `search_biased`, whose default ``None`` is the scan.
        Queries of the matrix path's own form are read in place, as by `search_device`."""
        _ffi.check(self._lib.ts_search_biased_ex(self._h, C.c_void_p(q_ptr), _DTYPES[q_dtype], 1, int(nq), int(k),
                                                 C.c_void_p(bias_ptr), 1, float(weight), None, 0, C.c_void_p(out_scores_ptr),
                                                 C.c_void_p(out_sims_ptr) if out_sims_ptr else None, C.c_void_p(out_idx_ptr), 1,
                                                 C.c_void_p(stream), _ALGOS[algo], None))

    def rank_of(self, queries, rows) -> Tuple[np.ndarray, np.ndarray]:
        """0-based rank of ``rows[i]`` among all index rows for query ``i`` (score descending, index ascending)
        and its score: what ``np.flatnonzero(np.argsort(-sim[i]) == rows[i])`` yields on the full score matrix
        (compare_embeddings.py:96-123), computed by one counting pass.  ``-1`` / NaN for rows not in the index."""
        q = _host_rows(queries)
        if q.shape[1] != self.d:
            raise ValueError(f"queries have d={q.shape[1]}, index has d={self.d}")
        t = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        if t.shape[0] != q.shape[0]:
            raise ValueError("one target row per query")
        ranks = np.empty(q.shape[0], dtype=np.int64)
        scores = np.empty(q.shape[0], dtype=np.float32)
        _ffi.check(self._lib.ts_rank_of(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, q.shape[0], _ffi.as_ptr(t),
                                        _ffi.as_ptr(ranks), _ffi.as_ptr(scores), None))
        return ranks, scores

    @staticmethod
    def _ragged(lists, dtype, nq):
        """Per-query sequences -> (offsets int64 [nq + 1], their concatenation as one contiguous array of ``dtype``)."""
        lists = [np.asarray(t, dtype=dtype).reshape(-1) for t in lists]
        if len(lists) != nq:
            raise ValueError(f"{len(lists)} target lists for {nq} queries")
        offsets = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum([t.shape[0] for t in lists], out=offsets[1:])
        return offsets, np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0, dtype=dtype))

    def rank_many(self, queries, targets):
        """Ranks of several rows per query in one matrix pass per block of 256 queries (every width that is a multiple of 64
        from 128 up to a 4,096-byte row, every multiple of 256 with a wider row of up to 16,384 bytes; other widths: one
        `rank_of` pass per target column): ``targets`` holds one integer
        sequence per query (ragged, possibly empty, repeats allowed).  Returns ``(ranks, scores)``, lists of per-query
        int64 / float32 arrays aligned with ``targets``; ``-1`` / NaN for rows not in the index or with a NaN score.
        The ranks are consistent with the returned scores (score descending, row ascending); where the fp64 truth cannot
        separate a target from its neighbours they may differ from `rank_of` by the count of those neighbours."""
        q = _host_rows(queries)
        if q.shape[1] != self.d:
            raise ValueError(f"queries have d={q.shape[1]}, index has d={self.d}")
        offsets, rows = self._ragged(targets, np.int64, q.shape[0])
        ranks = np.empty(max(1, rows.shape[0]), dtype=np.int64)
        scores = np.empty(max(1, rows.shape[0]), dtype=np.float32)
        _ffi.check(self._lib.ts_rank_many(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, q.shape[0], _ffi.as_ptr(offsets),
                                          _ffi.as_ptr(rows), _ffi.as_ptr(ranks), _ffi.as_ptr(scores), None))
        return ([ranks[offsets[i]:offsets[i + 1]] for i in range(q.shape[0])],
                [scores[offsets[i]:offsets[i + 1]] for i in range(q.shape[0])])

    def count_above_many(self, queries, target_scores, target_ids):
        """The many-targets form of `count_above`: ``target_scores`` / ``target_ids`` hold one sequence per query (ragged,
        possibly empty, repeats allowed) of documents given by score and GLOBAL id, wherever they live.  Returns a list of
        per-query int64 arrays: the rows of this index that rank before each document (``-1`` for a NaN score).  Summed
        over the shards of a corpus this is the document's rank, given the score `rank_many` returned on its own shard."""
        q = _host_rows(queries)
        if q.shape[1] != self.d:
            raise ValueError(f"queries have d={q.shape[1]}, index has d={self.d}")
        offsets, sc = self._ragged(target_scores, np.float32, q.shape[0])
        id_offsets, ids = self._ragged(target_ids, np.int64, q.shape[0])
        if not np.array_equal(offsets, id_offsets):
            raise ValueError("one id per target score")
        out = np.empty(max(1, ids.shape[0]), dtype=np.int64)
        _ffi.check(self._lib.ts_count_above_many(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, q.shape[0], _ffi.as_ptr(offsets),
                                                 _ffi.as_ptr(sc), _ffi.as_ptr(ids), _ffi.as_ptr(out), None))
        return [out[offsets[i]:offsets[i + 1]] for i in range(q.shape[0])]

    def count_above(self, queries, target_scores, target_ids) -> np.ndarray:
        """Rows of this index that rank before a document with the given score and GLOBAL id (it may live on another
        shard); summed over the shards of a corpus this is the document's rank (`rank_of` for one index)."""
        q = _host_rows(queries)
        if q.shape[1] != self.d:
            raise ValueError(f"queries have d={q.shape[1]}, index has d={self.d}")
        sc = np.ascontiguousarray(np.asarray(target_scores, dtype=np.float32).reshape(-1))
        ids = np.ascontiguousarray(np.asarray(target_ids, dtype=np.int64).reshape(-1))
        if sc.shape[0] != q.shape[0] or ids.shape[0] != q.shape[0]:
            raise ValueError("one target per query")
        out = np.empty(q.shape[0], dtype=np.int64)
        _ffi.check(self._lib.ts_count_above(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, q.shape[0], _ffi.as_ptr(sc),
                                            _ffi.as_ptr(ids), _ffi.as_ptr(out), None))
        return out

    def scores(self, queries) -> np.ndarray:
        """Full ``[nq x N]`` fp32 score matrix (small N): ``util.cos_sim(q_emb, s_emb)`` of
        compare_embeddings.py:24,61 when the index metric is "cos"."""
        q = _host_rows(queries)
        if q.shape[1] != self.d:
            raise ValueError(f"queries have d={q.shape[1]}, index has d={self.d}")
        out = np.empty((q.shape[0], self.n), dtype=np.float32)
        _ffi.check(self._lib.ts_scores(self._h, _ffi.as_ptr(q), _ffi.np_dtype_code(q), 0, q.shape[0],
                                       _ffi.as_ptr(out), 0, None))
        return out

    # -- moments ----------------------------------------------------------------------------
    def moments(self, rowset: Optional[RowSet] = None, gram=True):
        """``(count, sum float64 [d], gram float64 [d x d])`` of the STORED rows (normalised for "cos", rounded for bf16) - all of
        them, or those ``rowset`` allows - from the rows in HBM (``ts_index_moments``: a sums pass and a Gram pass): what `pca.fit` turns into
        a PCA.  ``gram`` false or None: the sums and the count only, and ``gram`` is returned as None.  The same bits on every call."""
        count = C.c_int64(0)
        s = np.zeros(self.d, dtype=np.float64)
        g = np.zeros((self.d, self.d), dtype=np.float64) if gram else None
        _ffi.check(self._lib.ts_index_moments(self._h, rowset.handle if rowset is not None else None, C.byref(count), _ffi.as_ptr(s),
                                              _ffi.as_ptr(g) if g is not None else None, None))
        return count.value, s, g

    def group_sums(self, meta, column, rowset: Optional[RowSet] = None, ngroups: Optional[int] = None):
        """``(names, counts int64 [G], sums float64 [G x d])``: per code of scalar column ``column`` (a name or a number) of the
        `metadata.MetaTable` ``meta``, the number of (allowed) rows that carry it and the sum of those rows
        (``ts_index_group_sums``).  The groups are the column's dictionary, in code order, and ``names`` its values; a column
        without a dictionary is taken as codes 0 .. max, named by number (``ngroups`` sets their number instead).  NULLs and codes
        outside the range go nowhere."""
        col = meta.col[column] if isinstance(column, str) else int(column)
        name = meta.names[col]
        if ngroups is not None:
            names = list(range(int(ngroups)))
        elif name in meta.dicts and len(meta.dicts[name]):
            names = list(meta.dicts[name].values)
        else:
            codes = np.asarray(meta.columns[col])
            names = list(range(int(codes.max(initial=-1)) + 1)) or [0]
        counts = np.zeros(len(names), dtype=np.int64)
        sums = np.zeros((len(names), self.d), dtype=np.float64)
        _ffi.check(self._lib.ts_index_group_sums(self._h, meta._h, col, len(names), rowset.handle if rowset is not None else None,
                                                 _ffi.as_ptr(counts), _ffi.as_ptr(sums), None))
        return names, counts, sums

    # -- profiling ---------------------------------------------------------------------------
    def profile_enable(self, enable: bool = True) -> None:
        _ffi.check(self._lib.ts_index_profile_enable(self._h, 1 if enable else 0))

    def profile_read(self) -> dict:
        """Launch count and summed hipEvent duration of the dominant kernel since the last read."""
        n, ms, rows = C.c_int64(0), C.c_double(0.0), C.c_int64(0)
        _ffi.check(self._lib.ts_index_profile_read(self._h, C.byref(n), C.byref(ms), C.byref(rows)))
        return {"launches": n.value, "total_ms": ms.value, "rows_per_launch": rows.value}

    def probe_read(self) -> dict:
        """Last in-kernel clock probe of the MFMA full pass (option ``TS_MFMA_VARIANT`` = 3)."""
        g, c, u = C.c_double(0), C.c_double(0), C.c_double(0)
        _ffi.check(self._lib.ts_index_probe_read(self._h, C.byref(g), C.byref(c), C.byref(u)))
        return {"ghz": g.value, "cycles_per_unit": c.value, "units_per_workgroup": u.value}

    # -- lifetime ---------------------------------------------------------------------------
    def close(self) -> None:
        self._cpu_rows = None
        if getattr(self, "_h", None) is not None and self._h.value:
            _ffi.check(self._lib.ts_index_destroy(self._h))      # refused while views of this index are alive
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def merge_topk(scores: np.ndarray, idx: np.ndarray, k_out: int, device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Merge ``[nparts x nq x k_in]`` partial results into the global top-``k_out`` on the device."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    i = np.ascontiguousarray(idx, dtype=np.int64)
    nparts, nq, k_in = s.shape
    os_ = np.empty((nq, k_out), dtype=np.float32)
    oi = np.empty((nq, k_out), dtype=np.int64)
    _ffi.check(_ffi.load().ts_merge_topk(device, _ffi.as_ptr(s), _ffi.as_ptr(i), nparts, nq, k_in, k_out,
                                         _ffi.as_ptr(os_), _ffi.as_ptr(oi), 0, None))
    return os_, oi


def group_depth(k: int) -> Tuple[int, int]:
    """``(first, deep)``: the depths of the grouped search's ladder for ``k`` (``ts_group_depth``; needs no device)."""
    first, deep = C.c_int32(0), C.c_int32(0)
    _ffi.check(_ffi.load().ts_group_depth(int(k), C.byref(first), C.byref(deep)))
    return first.value, deep.value


def collapse_topk(scores: np.ndarray, idx: np.ndarray, column, k_out: int, row_offset: int = 0, device: int = 0):
    """The collapse step of the grouped search alone (``ts_collapse_topk``), for sorted ``[nq x k_in]`` lists from anywhere -
    merged per-shard grouped results, a caller's own: the first ``k_out`` entries of each list that are the first of their group
    (``column[id - row_offset]``; NULL: a group of its own), in order.  Returns ``(scores, indices, groups, found, complete)``:
    ``found [nq]`` counts the group-firsts of the whole list, ``complete [nq]`` is true where ``found >= k_out`` or the list
    held padding."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    i = np.ascontiguousarray(idx, dtype=np.int64)
    col = np.ascontiguousarray(column, dtype=np.int32).reshape(-1)
    if s.ndim != 2 or s.shape != i.shape:
        raise ValueError("scores and idx are [nq x k_in], the same shape")
    nq, k_in = s.shape
    k_out = int(k_out)
    os_ = np.empty((nq, max(k_out, 0)), dtype=np.float32)
    oi = np.empty((nq, max(k_out, 0)), dtype=np.int64)
    og = np.empty((nq, max(k_out, 0)), dtype=np.int32)
    found = np.zeros(nq, dtype=np.int32)
    complete = np.zeros(nq, dtype=np.int32)
    _ffi.check(_ffi.load().ts_collapse_topk(device, _ffi.as_ptr(s), _ffi.as_ptr(i), nq, k_in, k_out, _ffi.as_ptr(col), col.shape[0],
                                            int(row_offset), _ffi.as_ptr(os_), _ffi.as_ptr(oi), _ffi.as_ptr(og), _ffi.as_ptr(found),
                                            _ffi.as_ptr(complete), 0, None))
    return os_, oi, og, found, complete.astype(bool)


class Timer:
    """hipEvent pair on a given stream (ts_timer_*)."""

    def __init__(self, device: int = 0):
        self._lib = _ffi.load()
        self._h = C.c_void_p()
        _ffi.check(self._lib.ts_timer_create(device, C.byref(self._h)))

    def start(self, stream: int = 0):
        _ffi.check(self._lib.ts_timer_start(self._h, C.c_void_p(stream)))

    def stop(self, stream: int = 0):
        _ffi.check(self._lib.ts_timer_stop(self._h, C.c_void_p(stream)))

    def elapsed_ms(self) -> float:
        ms = C.c_float(0)
        _ffi.check(self._lib.ts_timer_elapsed_ms(self._h, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            if self._h.value:
                self._lib.ts_timer_destroy(self._h)
        except Exception:
            pass
