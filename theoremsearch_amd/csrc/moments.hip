// libtsearch.so - C ABI (include/tsearch.h), part 7: moments of the stored rows taken on the device - count, column sums and Gram
// matrix (ts_index_moments), count and column sums per code of a metadata column (ts_index_group_sums).  The plan is
// moments_plan.h, the kernels kernels_moments.h; the host side of a PCA over the whole table (theoremsearch_amd/pca.py).
#include "host.h"
#include "moments_plan.h"
#include "kernels_moments.h"

static_assert(mom_lds_bytes(TS_F32, true) <= kMomLdsLimit && mom_lds_bytes(TS_BF16, true) <= kMomLdsLimit, "the staged panels fit the CU's LDS");
static_assert(kMomTileRows <= kRowPad && kRowPad % kMomTileRows == 0, "a tile never leaves the padded allocation");
static_assert(kMetaBlockRows % kMomTileRows == 0, "a tile's mask words lie inside the row set's allocation");
static_assert(kMomThreads == 4 * 64 && kMomPanel == 2 * 64, "four waves: the 64 x 64 quadrants of a pair's tile");
static_assert(kMomPairAccRegs == 4 * 4 * 4 && kMomGroupAccRegs == 4 * 2 * 4, "the accumulator blocks of moments_kernel");

extern "C" int ts_moments_plan(int32_t dtype, int32_t d, int64_t n, int32_t cu_count, int32_t* flush_rows, int32_t* panel,
                               int32_t* ranges, int64_t* partial_bytes) {
    if (flush_rows) *flush_rows = kMomFlushRows;
    if (panel) *panel = kMomPanel;
    if (!mom_served(dtype, d)) return fail(TS_ERR_UNSUPPORTED, "moments: no kernel for dtype %d, d = %d (bf16 / fp32, d a multiple of 64 in [%d, %d])", dtype, d, kMomMinD, kMomMaxD);
    if (n < 0) return fail(TS_ERR_INVALID, "n = %lld", (long long)n);
    const int r = mom_ranges(n, cu_count, mom_pairs(d), mom_pair_tile_bytes());
    if (ranges) *ranges = r;
    if (partial_bytes) *partial_bytes = mom_partial_bytes(r, mom_pairs(d), mom_pair_tile_bytes());
    return TS_OK;
}

// the index and the row set of a call: the rules and the wording of ts_search_rowset
static int mom_check(const ts_index* ix, const ts_rowset* rows) {
    if (!mom_served(ix->dtype, ix->d) || ix->ld != ix->d)
        return fail(TS_ERR_UNSUPPORTED, "moments: no kernel for d = %d (bf16 / fp32 indexes, d a multiple of 64 in [%d, %d])", ix->d, kMomMinD, kMomMaxD);
    if (rows) {
        if (rows->n != ix->n) return fail(TS_ERR_INVALID, "the row set has %lld rows, the index %lld", (long long)rows->n, (long long)ix->n);
        if (rows->device != ix->device) return fail(TS_ERR_INVALID, "the row set lives on device %d, the index on device %d", rows->device, ix->device);
    }
    return TS_OK;
}

template <bool IND>
static int mom_launch(const ts_index* ix, int units, int ranges, hipStream_t st, const MomArgs& a) {
    const MomGrid g = mom_grid(units, ranges);
    const int lds = mom_lds_bytes(ix->dtype, !IND);
    if (ix->dtype == TS_F32) return launch_lds<moments_kernel<true, IND>>(ix->device, dim3(g.x, g.y), kMomThreads, lds, st, a);
    return launch_lds<moments_kernel<false, IND>>(ix->device, dim3(g.x, g.y), kMomThreads, lds, st, a);
}

// counts [ngroups] u64 and sums [ngroups][d] doubles of the indicator pass into `out` (device), `partial` sized by the caller
static int mom_group_pass(const ts_index* ix, const u32* mask, const int32_t* codes, int ngroups, double* partial, int ranges,
                          u64* counts, double* sums, hipStream_t st) {
    const int units = mom_panels(ix->d) * mom_group_chunks(ngroups);
    MomArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = ix->rows;
    a.mask = mask;
    a.codes = codes;
    a.partial = partial;
    a.n = ix->n;
    a.d = ix->d;
    a.ngroups = ngroups;
    TS_TRY(mom_launch<true>(ix, units, ranges, st, a));
    moments_finish_groups<<<dim3(kMomGroupChunk * kMomPanel / 256, units), 256, 0, st>>>(partial, sums, ix->d, ngroups, ranges);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(counts, 0, (size_t)ngroups * 8, st));
    const int grid = (int)std::min<int64_t>(((ix->n + 31) / 32 + 255) / 256, (int64_t)ix->cu_count * 8);
    moments_count_kernel<<<std::max(grid, 1), 256, 0, st>>>(mask, codes, ix->n, ngroups, counts);
    HIP_TRY(hipGetLastError());
    return TS_OK;
}

static int mom_group_ranges(const ts_index* ix, int ngroups) {
    return mom_ranges(ix->n, ix->cu_count, mom_panels(ix->d) * mom_group_chunks(ngroups), mom_group_tile_bytes());
}
static size_t mom_group_partial(const ts_index* ix, int ngroups) {
    return (size_t)mom_partial_bytes(mom_group_ranges(ix, ngroups), mom_panels(ix->d) * mom_group_chunks(ngroups), mom_group_tile_bytes());
}

extern "C" int ts_index_moments(ts_index* ix, const ts_rowset* rows, int64_t* out_count, double* out_sum, double* out_gram, void* stream) {
    if (!ix || !out_count || !out_sum) return fail(TS_ERR_INVALID, "NULL argument");
    TS_TRY(mom_check(ix, rows));
    const int d = ix->d;
    *out_count = 0;
    memset(out_sum, 0, (size_t)d * 8);
    if (out_gram) memset(out_gram, 0, (size_t)d * d * 8);
    if (ix->n == 0 || (rows && rows->allowed == 0)) return TS_OK;
    std::lock_guard<std::mutex> lock(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st;
    StreamScope scope;
    TS_TRY(enter_stream(ix, stream, &st, &scope));
    const int pairs = mom_pairs(d);
    const int pranges = mom_ranges(ix->n, ix->cu_count, pairs, mom_pair_tile_bytes());
    const size_t pbytes = out_gram ? (size_t)mom_partial_bytes(pranges, pairs, mom_pair_tile_bytes()) : 0;
    DevBuf partial, out;
    DEV_TRY(partial.need(std::max(pbytes, mom_group_partial(ix, 1))));
    const size_t gram_doubles = out_gram ? (size_t)d * d : 0;
    DEV_TRY(out.need((gram_doubles + d + 1) * 8));
    double* dgram = out.as<double>();
    double* dsum = dgram + gram_doubles;
    u64* dcount = (u64*)(dsum + d);
    const u32* mask = rows ? rows->mask.as<u32>() : nullptr;
    // from here on every path drains the stream before the temporaries are freed: failures are kept in rc, not returned
    int rc = mom_group_pass(ix, mask, nullptr, 1, partial.as<double>(), mom_group_ranges(ix, 1), dcount, dsum, st);
    if (rc == TS_OK && out_gram) {
        MomArgs a;
        memset(&a, 0, sizeof(a));
        a.rows = ix->rows;
        a.mask = mask;
        a.partial = partial.as<double>();
        a.n = ix->n;
        a.d = d;
        hipEvent_t stop = prof_begin(ix, st, ix->n);
        rc = mom_launch<false>(ix, pairs, pranges, st, a);
        prof_end(stop, st);
        if (rc == TS_OK) {
            moments_finish_gram<<<dim3(kMomPanel * kMomPanel / 256, pairs), 256, 0, st>>>(partial.as<double>(), dgram, d, pranges);
            if (hipGetLastError() != hipSuccess) rc = fail(TS_ERR_HIP, "launch of the Gram finish failed");
        }
    }
    uint64_t count = 0;
    if (rc == TS_OK) {
        hipError_t e = hipMemcpyAsync(&count, dcount, 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_sum, dsum, (size_t)d * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && out_gram) e = hipMemcpyAsync(out_gram, dgram, gram_doubles * 8, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = fail(TS_ERR_HIP, "copy of the moments failed: %s", hipGetErrorString(e));
    }
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess && rc == TS_OK) rc = fail(TS_ERR_HIP, "the moments pass failed: %s", hipGetErrorString(e));
    if (rc == TS_OK) *out_count = (int64_t)count;
    return rc;
}

extern "C" int ts_index_group_sums(ts_index* ix, const ts_meta* m, int32_t col, int32_t ngroups, const ts_rowset* rows,
                                   int64_t* out_counts, double* out_sums, void* stream) {
    if (!ix || !m || !out_counts || !out_sums) return fail(TS_ERR_INVALID, "NULL argument");
    TS_TRY(mom_check(ix, rows));
    if (ngroups < 1 || ngroups > kMomMaxGroups) return fail(TS_ERR_UNSUPPORTED, "group sums: ngroups = %d outside [1, %d]", ngroups, kMomMaxGroups);
    if (m->n != ix->n) return fail(TS_ERR_INVALID, "the meta table has %lld rows, the index %lld", (long long)m->n, (long long)ix->n);
    if (m->device != ix->device) return fail(TS_ERR_INVALID, "the meta table lives on device %d, the index on device %d", m->device, ix->device);
    if (col < 0 || col >= m->ncols) return fail(TS_ERR_INVALID, "column %d outside [0, %d)", col, m->ncols);
    const int d = ix->d;
    std::lock_guard<std::mutex> lock(ix->mu);
    std::lock_guard<std::mutex> mlock(const_cast<ts_meta*>(m)->mu);
    if (m->kind[col] == kMetaColList) return fail(TS_ERR_INVALID, "column %d is a list column", col);
    if (m->kind[col] != kMetaColScalar) return fail(TS_ERR_INVALID, "column %d was never set", col);
    memset(out_counts, 0, (size_t)ngroups * 8);
    memset(out_sums, 0, (size_t)ngroups * d * 8);
    if (ix->n == 0 || (rows && rows->allowed == 0)) return TS_OK;
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st;
    StreamScope scope;
    TS_TRY(enter_stream(ix, stream, &st, &scope));
    DevBuf partial, out;
    DEV_TRY(partial.need(mom_group_partial(ix, ngroups)));
    DEV_TRY(out.need(((size_t)ngroups * d + ngroups) * 8));
    double* dsums = out.as<double>();
    u64* dcounts = (u64*)(dsums + (size_t)ngroups * d);
    int rc = mom_group_pass(ix, rows ? rows->mask.as<u32>() : nullptr, m->values[col].as<int32_t>(), ngroups, partial.as<double>(),
                            mom_group_ranges(ix, ngroups), dcounts, dsums, st);
    if (rc == TS_OK) {
        hipError_t e = hipMemcpyAsync(out_counts, dcounts, (size_t)ngroups * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_sums, dsums, (size_t)ngroups * d * 8, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = fail(TS_ERR_HIP, "copy of the group sums failed: %s", hipGetErrorString(e));
    }
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess && rc == TS_OK) rc = fail(TS_ERR_HIP, "the group-sums pass failed: %s", hipGetErrorString(e));
    return rc;
}
