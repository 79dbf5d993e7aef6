"""Bit-exact tests of what enters the index and the query buffers: prep_rows_kernel in all eight instantiations, the padded
storage layout the matrix kernels rely on, and the row copies (unpad_rows_kernel, gather_rows_kernel).  The reference and
the inputs are prep_common.py's (checked on the CPU by test_prep_ref_cpu.py); every assertion is an equality of bits."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import prep_common as pc

pytestmark = pytest.mark.gpu

SOURCES = ("f32", "bf16")
STORAGES = ("f32", "bf16")
METRICS = ("ip", "cos")


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, tag):
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, got.dtype, want.shape, want.dtype)
    bad = bits(got) != bits(want)
    if bad.any():
        first = ", ".join(f"[{r},{c}] got {int(bits(got)[r, c]):#x} want {int(bits(want)[r, c]):#x}" for r, c in np.argwhere(bad)[:4])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.size} elements differ in {int(bad.any(axis=1).sum())} rows: {first}")


def stored(ts, rows, storage, metric):
    with ts.TheoremIndex.from_embeddings(rows, dtype=storage, metric=metric) as ix:
        return ix.download()


# ---- a. every instantiation at the width edges ---------------------------------------------------------------------
@pytest.mark.parametrize("d", pc.WIDTHS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("src", SOURCES)
def test_every_instantiation_at_the_width_edges(ts, src, storage, metric, d):
    rows = pc.width_case(d, src)
    assert rows.shape == (pc.N_FREE + pc.n_special(), d)
    got = stored(ts, rows, storage, metric)
    pc.assert_prepared_equal(got, pc.prepare(rows, metric, storage), rows, metric == "cos", tag=f"{src}->{storage} {metric} d={d}")


@functools.lru_cache(maxsize=None)
def gaussian_reference(src, storage, metric):
    want = pc.prepare(pc.gaussian_case(src), metric, storage)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("src", SOURCES)
def test_gaussian_rows_on_the_decided_rows(ts, src, storage):
    rows, decided = pc.gaussian_case(src), pc.gaussian_decided(src)
    assert (~decided).sum() <= pc.UNDECIDED_CAP * decided.size
    for metric in METRICS:
        got = stored(ts, rows, storage, metric)
        pc.assert_prepared_equal(got, gaussian_reference(src, storage, metric), rows, metric == "cos", rows=decided,
                                 tag=f"gaussian {src}->{storage} {metric}")


# ---- b. grid stride and the widest row -----------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("src", SOURCES)
def test_rows_past_the_grid_stride_point(ts, src, storage):
    """4096 workgroups x 4 waves is the largest launch: rows from 16,384 on take the loop's second trip."""
    n, d = 16_389, 8
    rows = pc.as_source(pc.order_free_rows(n, d, 16389), src)
    for metric in METRICS:
        got = stored(ts, rows, storage, metric)
        pc.assert_prepared_equal(got, pc.prepare(rows, metric, storage), rows, metric == "cos", tag=f"{src}->{storage} {metric} n={n}")


def test_widest_rows_through_two_staging_chunks(ts):
    """d = 16,384: 256 trips of the wave over a row, and 4,096 fp32 rows fill the 256 MiB staging buffer, so the upload
    and the download of 4,100 rows both take two chunks."""
    n, d = 4_100, 16_384
    rows = pc.order_free_rows(n, d, 4100)
    want = pc.prepare(rows, "cos", "f32")
    t0 = time.perf_counter()
    with ts.TheoremIndex.from_embeddings(rows, dtype="f32", metric="cos") as ix:
        assert ix.info()["ld"] == d
        got = ix.download()
        tail = ix.download(4_090, 10)                      # a window across the staging boundary of the upload
    print(f"d={d} n={n}: create + upload + downloads took {time.perf_counter() - t0:.2f} s")
    if not np.array_equal(bits(got), bits(want)):
        pc.assert_prepared_equal(got, want, rows, True, tag=f"d={d} n={n}")
    assert np.array_equal(bits(tail), bits(want[4_090:]))


# ---- c. device sources ---------------------------------------------------------------------------------------------
def device_source(torch, rows, src_ld):
    """The rows in a device buffer with row stride src_ld that starts one element past the allocation's base (a bf16
    source is then only 2-byte aligned); every element outside the rows is a NaN.  Returns (tensor, address of row 0)."""
    n, d = rows.shape
    poison = np.uint16(0x7FC0) if rows.dtype == np.uint16 else np.float32(np.nan)
    host = np.full(1 + n * src_ld, poison, dtype=rows.dtype)
    host[1:].reshape(n, src_ld)[:, :d] = rows
    dev = torch.from_numpy(host.view(np.int16) if rows.dtype == np.uint16 else host).cuda()
    return dev, dev.data_ptr() + host.itemsize


@pytest.mark.parametrize("pad", [0, 1, 37])
@pytest.mark.parametrize("src", SOURCES)
def test_device_sources_match_the_host_upload(ts, src, pad):
    import torch
    d, n0, cut = 100, 500, 7
    rows = pc.width_case(d, src)
    head, tail, src_ld = rows[:n0], rows[n0:], d + pad
    stream = torch.cuda.current_stream().cuda_stream
    for storage in STORAGES:
        for metric in METRICS:
            want = stored(ts, rows, storage, metric)
            with ts.TheoremIndex(n0, d, dtype=storage, metric=metric) as ix:
                a = device_source(torch, head[:cut], src_ld)
                b = device_source(torch, head[cut:], src_ld)
                c = device_source(torch, tail, src_ld)
                ix.upload_device(b[1], src, src_ld, cut, n0 - cut, stream)          # a window with row0 > 0
                ix.upload_device(a[1], src, src_ld, 0, cut, stream)
                assert ix.append_device(c[1], src, src_ld, tail.shape[0], stream) == n0   # past 512 rows: the rows move
                assert ix.n == rows.shape[0]
                ix.synchronize()
                got = ix.download()
            assert_same_bits(got, want, f"{src}->{storage} {metric} src_ld={src_ld}")


# ---- d. windows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("src", SOURCES)
def test_upload_and_download_windows(ts, src, storage):
    d, n, row0, cnt = 100, 1000, 7, 300
    base = pc.order_free_rows(n, d, 31)
    new = pc.width_case(d, src)[-cnt:]                     # ends with the special block
    with ts.TheoremIndex.from_embeddings(base, dtype=storage, metric="cos") as ix:
        before = ix.download()
        ix.upload(new, row0)
        after = ix.download()
        windows = {(r0, nr): ix.download(r0, nr) for r0, nr in [(0, 1), (0, 5), (n - 5, 5), (n - 1, 1), (500, 1), (row0 - 1, cnt + 2)]}
    pc.assert_prepared_equal(before, pc.prepare(base, "cos", storage), base, True, tag="before")
    assert_same_bits(after[:row0], before[:row0], "rows before the window")
    assert_same_bits(after[row0 + cnt:], before[row0 + cnt:], "rows behind the window")
    pc.assert_prepared_equal(after[row0:row0 + cnt], pc.prepare(new, "cos", storage), new, True, tag="the window")
    for (r0, nr), got in windows.items():
        assert_same_bits(got, after[r0:r0 + nr], f"download({r0}, {nr})")


# ---- e. padded storage ---------------------------------------------------------------------------------------------
def read_allocation(ix):
    """The first ceil(n / 256) * 256 rows of the allocation (what ts_index_attach_device's contract promises), ld elements
    each, as the bits of the storage dtype."""
    import torch
    from theoremsearch_amd import _ffi
    info = ix.info()
    assert info["n"] == ix.n and info["d"] == ix.d and info["ld"] % 64 == 0 and info["ld"] - 64 < ix.d <= info["ld"]
    nrows = -(-info["n"] // 256) * 256
    elem = 2 if info["dtype"] == _ffi.TS_BF16 else 4
    nbytes = nrows * info["ld"] * elem
    ix.synchronize()
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _ffi.check(_ffi.load().ts_copy_device(ix.device, C.c_void_p(buf.data_ptr()), C.c_void_p(info["rows_ptr"]), nbytes,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint16 if elem == 2 else np.uint32).reshape(nrows, info["ld"])


def check_padded(ix, tag):
    alloc = read_allocation(ix)
    n, d = ix.n, ix.d
    dirty = np.argwhere(alloc[:, d:] != 0)
    assert dirty.size == 0, f"{tag}: {len(dirty)} non-zero padding columns, first at row {dirty[0][0]} col {d + dirty[0][1]}"
    dirty = np.argwhere(alloc[n:] != 0)
    assert dirty.size == 0, f"{tag}: {len(dirty)} non-zero elements in the padding rows, first at row {n + dirty[0][0]} col {dirty[0][1]}"
    assert_same_bits(alloc[:n, :d], bits(ix.download()), f"{tag}: rows_ptr against download()")


@pytest.mark.parametrize("d", [100, 1000])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("src", SOURCES)
def test_padding_is_zero_after_create_and_overwrite(ts, src, storage, metric, d):
    rows = pc.width_case(d, src, 515 - pc.n_special())
    assert rows.shape[0] == 515
    with ts.TheoremIndex.from_embeddings(rows, dtype=storage, metric=metric) as ix:
        check_padded(ix, "after from_embeddings")
        ix.upload(rows[-300:], 7)                          # NaN, Inf and -0.0 rows over what were plain rows
        check_padded(ix, "after an overwrite")
        ix.upload(rows[:100], 415)                         # and plain rows over the special block, up to the last row
        check_padded(ix, "after an overwrite of the last rows")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("storage", STORAGES)
def test_padding_is_zero_after_appends_that_move_the_rows(ts, storage, metric):
    d = 100
    rows = np.concatenate([pc.width_case(d, "f32")[-200:], pc.order_free_rows(800, d, 41)])
    with ts.TheoremIndex.from_embeddings(rows[:200], dtype=storage, metric=metric) as ix:
        old, where = ix.download(), ix.info()["rows_ptr"]
        for lo, hi in ((200, 300), (300, 1000)):
            assert ix.append(rows[lo:hi]) == lo and ix.n == hi
            assert ix.info()["rows_ptr"] != where, "this append was meant to move the rows"
            where = ix.info()["rows_ptr"]
            check_padded(ix, f"after the append to {hi} rows")
            assert_same_bits(ix.download(0, 200), old, f"the old rows after the append to {hi} rows")
        got = ix.download()
    pc.assert_prepared_equal(got, pc.prepare(rows, metric, storage), rows, metric == "cos", tag="the grown index")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("src", SOURCES)
def test_padding_is_zero_after_append_device(ts, src, storage):
    import torch
    d = 100
    rows = pc.width_case(d, src)[-300:]
    with ts.TheoremIndex.from_embeddings(rows[:200], dtype=storage, metric="cos") as ix:
        dev, ptr = device_source(torch, rows[200:], d + 1)
        assert ix.append_device(ptr, src, d + 1, 100, torch.cuda.current_stream().cuda_stream) == 200
        check_padded(ix, "after append_device")
        got = ix.download()
    pc.assert_prepared_equal(got, pc.prepare(rows, "cos", storage), rows, True, tag="after append_device")


@pytest.mark.parametrize("d", [100, 1000])
@pytest.mark.parametrize("storage", STORAGES)
def test_padding_is_zero_in_a_subset_index(ts, storage, d):
    rows = pc.width_case(d, "f32", 515 - pc.n_special())
    ids = np.r_[0:3, 250:260, 505:515]
    with ts.TheoremIndex.from_embeddings(rows, dtype=storage, metric="cos") as ix:
        full = ix.download()
        for sel in (ids, np.arange(515), ids[-1:]):
            sub = ix.subset(sel)
            try:
                check_padded(sub, f"subset of {len(sel)} rows")
                assert_same_bits(sub.download(), full[sel], f"subset of {len(sel)} rows")
            finally:
                sub.close()


# ---- f. subset copies ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("row_offset", [0, 1000])
def test_subset_rows_are_copies_of_the_parent_rows(ts, row_offset, storage, d):
    rows = pc.width_case(d, "f32")
    n = rows.shape[0]
    local = np.r_[0:4, 63:66, 255:258, 300, n - 12:n]      # first and last row, runs of neighbours, the special block
    mask = np.random.default_rng(d).random(n) < 0.4
    mask[[0, 1, n - 1]] = True
    with ts.TheoremIndex.from_embeddings(rows, dtype=storage, metric="cos", row_offset=row_offset) as ix:
        full = ix.download()
        for name, sel, want in (("ids", local + row_offset, full[local]), ("mask", mask, full[mask]),
                                ("first row", [row_offset], full[:1]), ("last row", [row_offset + n - 1], full[-1:])):
            sub = ix.subset(sel)
            try:
                assert sub.n == want.shape[0]
                assert_same_bits(sub.download(), want, f"subset by {name}")
            finally:
                sub.close()


def test_subset_of_more_rows_than_the_copy_has_waves(ts):
    """gather_rows_kernel runs at most 8192 workgroups x 4 waves: with 32,800 rows the last ones take a second trip."""
    n, d = 33_000, 8
    rows = pc.order_free_rows(n, d, 33)
    ids = np.delete(np.arange(n), np.arange(100, 300))
    assert ids.size > 32_768
    with ts.TheoremIndex.from_embeddings(rows, dtype="f32", metric="ip") as ix:
        full = ix.download()
        sub = ix.subset(ids)
        try:
            assert_same_bits(sub.download(), full[ids], "subset past the grid stride point")
        finally:
            sub.close()
    assert_same_bits(full, rows, "an ip index stores fp32 rows as given")


# ---- g. the query side ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("storage", STORAGES)
def test_scores_against_the_identity_are_the_prepared_queries(ts, storage, metric, d):
    """Against the d x d identity each score is one product by 1.0 plus zeros: ts_scores returns the query buffer that
    prep_rows_kernel wrote (its fp32 copy, 256 rows per block).  Values are compared with ==: -0.0 may return as +0.0."""
    eye = np.eye(d, dtype=np.float32)
    with ts.TheoremIndex.from_embeddings(eye, dtype=storage, metric=metric) as ix:
        assert_same_bits(ix.download(), pc.prepare(eye, "ip", storage), "the identity is stored as 1.0 and +0.0")
        for qsrc in SOURCES:
            for nq in (1, 3, 257):                          # 257: the second block holds one query
                q = pc.as_source(pc.query_rows(nq, d, 100 * d + nq), qsrc)
                want = pc.widen(pc.prepare(q, metric, storage))
                assert np.isfinite(want).all()
                got = ix.scores(q)
                assert got.shape == (nq, d)
                bad = got != want
                if bad.any():
                    r, c = np.argwhere(bad)[0]
                    raise AssertionError(f"{qsrc} queries, nq={nq}: {int(bad.sum())} of {bad.size} scores differ from the prepared "
                                         f"queries; first at [{r},{c}]: got {got[r, c]!r} want {want[r, c]!r} query {pc.widen(q)[r, c]!r}")
