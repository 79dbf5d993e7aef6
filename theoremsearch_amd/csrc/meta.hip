// libtsearch.so - C ABI (include/tsearch.h), part 6: the rows' metadata as columns in HBM (ts_meta_*), a filter program
// evaluated to a row set (ts_meta_eval, kernels_meta.h) and the row set itself (ts_rowset_*).  The searches that take a row
// set are search.hip's (ts_search_rowset, ts_search_biased_rowset).
#include "host.h"
#include "kernels_meta.h"

extern "C" int ts_meta_create(int device, int64_t n, int32_t ncols, ts_meta** out) {
    if (!out) return fail(TS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 0 || n > 0xFFFFFFF0ll) return fail(TS_ERR_INVALID, "n = %lld out of range", (long long)n);
    if (ncols < 1 || ncols > TS_META_MAX_COLS) return fail(TS_ERR_INVALID, "ncols = %d outside [1, %d]", ncols, TS_META_MAX_COLS);
    TS_TRY(check_device(device));
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<ts_meta> m(new (std::nothrow) ts_meta());
    if (!m) return fail(TS_ERR_NOMEM, "host allocation failed");
    m->device = device;
    m->n = n;
    m->ncols = ncols;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) == hipSuccess) m->cu_count = p.multiProcessorCount;
    *out = m.release();
    return TS_OK;
}

extern "C" int ts_meta_destroy(ts_meta* m) {
    if (!m) return TS_OK;
    hipSetDevice(m->device);
    delete m;       // every ts_meta_eval has waited for its own work: nothing is in flight
    return TS_OK;
}

extern "C" int ts_meta_set_column(ts_meta* m, int32_t col, const int32_t* values, int64_t row0, int64_t nrows) {
    if (!m || !values) return fail(TS_ERR_INVALID, "NULL argument");
    if (col < 0 || col >= m->ncols) return fail(TS_ERR_INVALID, "column %d outside [0, %d)", col, m->ncols);
    if (row0 < 0 || nrows < 0 || row0 > m->n || nrows > m->n - row0)
        return fail(TS_ERR_INVALID, "rows [%lld, %lld + %lld) outside the table's %lld", (long long)row0, (long long)row0, (long long)nrows, (long long)m->n);
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->kind[col] == kMetaColList) return fail(TS_ERR_INVALID, "column %d is a list column", col);
    HIP_TRY(hipSetDevice(m->device));
    if (m->kind[col] == kMetaColUnset) {
        // rows that are never uploaded are NULL
        DEV_TRY(m->values[col].need(std::max<size_t>((size_t)m->n * 4, 4)));
        const hipError_t e = m->n ? hipMemsetD32(m->values[col].as<void>(), TS_META_NULL, (size_t)m->n) : hipSuccess;
        if (e != hipSuccess) {
            m->values[col].reset();
            return fail(TS_ERR_HIP, "hipMemsetD32 of a column failed: %s", hipGetErrorString(e));
        }
        m->kind[col] = kMetaColScalar;
    }
    if (nrows) HIP_TRY(hipMemcpy(m->values[col] + row0, values, (size_t)nrows * 4, hipMemcpyHostToDevice));
    return TS_OK;
}

extern "C" int ts_meta_set_lists(ts_meta* m, int32_t col, const int64_t* offsets, const int32_t* codes) {
    if (!m || !offsets) return fail(TS_ERR_INVALID, "NULL argument");
    if (col < 0 || col >= m->ncols) return fail(TS_ERR_INVALID, "column %d outside [0, %d)", col, m->ncols);
    // the kernel walks codes[offsets[row] .. offsets[row + 1]): every bound it relies on is checked here
    if (offsets[0] != 0) return fail(TS_ERR_INVALID, "offsets[0] = %lld, not 0", (long long)offsets[0]);
    for (int64_t r = 0; r < m->n; ++r)
        if (offsets[r + 1] < offsets[r]) return fail(TS_ERR_INVALID, "offsets descend at row %lld", (long long)r);
    const int64_t total = offsets[m->n];
    if (total > 0 && !codes) return fail(TS_ERR_INVALID, "codes is NULL");
    for (int64_t j = 0; j < total; ++j)
        if (codes[j] < 0) return fail(TS_ERR_INVALID, "codes[%lld] = %d is negative", (long long)j, codes[j]);
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->kind[col] == kMetaColScalar) return fail(TS_ERR_INVALID, "column %d is a scalar column", col);
    HIP_TRY(hipSetDevice(m->device));
    m->kind[col] = kMetaColUnset;       // until both halves are in place
    DEV_TRY(m->offsets[col].need((size_t)(m->n + 1) * 8));
    DEV_TRY(m->values[col].need(std::max<size_t>((size_t)total * 4, 4)));
    HIP_TRY(hipMemcpy(m->offsets[col], offsets, (size_t)(m->n + 1) * 8, hipMemcpyHostToDevice));
    if (total) HIP_TRY(hipMemcpy(m->values[col], codes, (size_t)total * 4, hipMemcpyHostToDevice));
    m->kind[col] = kMetaColList;
    return TS_OK;
}

// everything ts_meta_eval enqueues on `st`; the caller waits for the stream whatever this returns
static int meta_eval_enqueue(ts_meta* m, const MetaProgram& p, const std::vector<u32>& sets, ts_rowset* r, u64* allowed_host, hipStream_t st) {
    if (!sets.empty()) HIP_TRY(hipMemcpyAsync(m->sets, sets.data(), sets.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(m->allowed, 0, 8, st));
    MetaArgs a;
    memset(&a, 0, sizeof(a));
    a.n = m->n;
    a.nblocks = mask_blocks(m->n);
    a.natoms = p.natoms;
    a.all_groups = meta_all_groups(p.ngroups);
    a.mask = r->mask;
    a.allowed = m->allowed;
    for (int i = 0; i < p.natoms; ++i) {
        const MetaAtom& s = p.atom[i];
        MetaKAtom& t = a.atom[i];
        t.kind = s.kind;
        t.lo = s.lo;
        t.hi = s.hi;
        t.negate = s.negate;
        t.slot = s.slot;
        t.set_bits = s.set_bits;
        t.values = m->values[s.col];
        t.offsets = m->offsets[s.col];
        t.set = m->sets.as<u32>() + s.set_off;
    }
    meta_eval_kernel<<<meta_grid(m->cu_count, m->n), kMetaThreads, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(allowed_host, m->allowed, 8, hipMemcpyDeviceToHost, st));
    return TS_OK;
}

extern "C" int ts_meta_eval(ts_meta* m, const ts_atom* atoms, int32_t natoms, ts_rowset** out, void* stream) {
    if (!out) return fail(TS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!m) return fail(TS_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(m->mu);
    const MetaProgram p = meta_plan(m->kind, m->ncols, atoms, natoms);
    if (p.invalid) {
        if (p.bad_atom < 0) return fail(TS_ERR_INVALID, "%s", p.invalid);
        return fail(TS_ERR_INVALID, "atom %d (column %d): %s", p.bad_atom, atoms[p.bad_atom].col, p.invalid);
    }
    HIP_TRY(hipSetDevice(m->device));
    std::vector<u32> sets((size_t)p.set_words);
    meta_pack_sets(p, atoms, sets.data());
    std::unique_ptr<ts_rowset> r(new (std::nothrow) ts_rowset());
    if (!r) return fail(TS_ERR_NOMEM, "host allocation failed");
    r->device = m->device;
    r->n = m->n;
    DEV_TRY(r->mask.need((size_t)mask_alloc_words(m->n) * 4));
    DEV_TRY(m->sets.need(std::max<size_t>(sets.size() * 4, 4)));
    DEV_TRY(m->allowed.need(8));
    hipStream_t st = (hipStream_t)stream;
    u64 allowed = 0;
    const int rc = meta_eval_enqueue(m, p, sets, r.get(), &allowed, st);
    // `sets`, `allowed` and (on failure) the row set's mask go out of scope behind this: the stream is drained first, always
    const hipError_t e = hipStreamSynchronize(st);
    TS_TRY(rc);
    if (e != hipSuccess) return fail(TS_ERR_HIP, "the filter evaluation failed: %s", hipGetErrorString(e));
    r->allowed = (int64_t)allowed;
    *out = r.release();
    return TS_OK;
}

extern "C" int ts_rowset_info(const ts_rowset* r, int64_t* n, int64_t* allowed, void** device_mask) {
    if (!r) return fail(TS_ERR_INVALID, "row set is NULL");
    if (n) *n = r->n;
    if (allowed) *allowed = r->allowed;
    if (device_mask) *device_mask = r->mask.as<void>();
    return TS_OK;
}

extern "C" int ts_rowset_download(ts_rowset* r, uint32_t* host_words) {
    if (!r || !host_words) return fail(TS_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(r->device));
    if (r->n) HIP_TRY(hipMemcpy(host_words, r->mask, (size_t)mask_words(r->n) * 4, hipMemcpyDeviceToHost));
    return TS_OK;
}

extern "C" int ts_rowset_destroy(ts_rowset* r) {
    if (!r) return TS_OK;
    hipSetDevice(r->device);
    // a search that reads the mask may still be in flight on a caller's stream: hipFree waits for the device
    delete r;
    return TS_OK;
}
