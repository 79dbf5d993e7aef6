// libtsearch.so - C ABI (include/tsearch.h), part 8: grouped search - the k best distinct groups, one row per group
// (ts_search_grouped), its collapse step alone (ts_collapse_topk) and the exclusion row set (ts_rowset_exclude).  The ladder's
// rules are group_plan.h, the kernels kernels_group.h; every search it runs is search.hip's search_core, untouched.
#include "host.h"
#include "group_plan.h"
#include "kernels_group.h"

extern "C" int ts_group_depth(int32_t k, int32_t* first, int32_t* deep) {
    if (const char* bad = group_depth_invalid(k)) return fail(TS_ERR_INVALID, "k = %d: %s", k, bad);
    if (first) *first = group_first_depth(k);
    if (deep) *deep = group_deep_depth();
    return TS_OK;
}

// one workgroup per list: one wave up to 64 entries, four above (the sizes of merge_kernel's variants)
static int collapse_launch(const CollapseArgs& a, int nq, hipStream_t st) {
    if (nq == 0) return TS_OK;
    if (a.k_in <= kWave) collapse_kernel<kWave><<<nq, kWave, 0, st>>>(a);
    else collapse_kernel<TS_MAX_K><<<nq, TS_MAX_K, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    return TS_OK;
}

extern "C" int ts_collapse_topk(int device, const float* scores, const int64_t* idx, int32_t nq, int32_t k_in, int32_t k_out,
                                const int32_t* column, int64_t n, int64_t row_offset, float* out_scores, int64_t* out_idx,
                                int32_t* out_groups, int32_t* out_found, int32_t* out_complete, int on_device, void* stream) {
    if (const char* bad = collapse_args_invalid(scores, idx, column, out_scores, out_idx, nq, k_in, k_out, n, row_offset))
        return fail(TS_ERR_INVALID, "ts_collapse_topk (nq = %d, k_in = %d, k_out = %d): %s", nq, k_in, k_out, bad);
    if (nq == 0) return TS_OK;
    TS_TRY(check_device(device));
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    CollapseArgs a;
    memset(&a, 0, sizeof(a));
    a.k_in = k_in;
    a.k_out = k_out;
    a.n = n;
    a.row_offset = row_offset;
    const size_t nin = (size_t)nq * k_in, nout = (size_t)nq * k_out;
    DevBuf tmp;     // host form: ids in | ids out | scores in | scores out | groups | found | complete | column
    if (on_device) {
        a.scores = scores;
        a.idx = idx;
        a.column = column;
        a.out_scores = out_scores;
        a.out_idx = out_idx;
        a.out_groups = out_groups;
        a.out_found = out_found;
        a.out_complete = out_complete;
        if (!out_groups) {      // the kernel writes the groups unconditionally
            DEV_TRY(tmp.need(nout * 4));
            a.out_groups = tmp.as<int32_t>();
        }
        TS_TRY(collapse_launch(a, nq, st));
        if (!out_groups) HIP_TRY(hipStreamSynchronize(st));      // `tmp` goes out of scope
        return TS_OK;
    }
    DEV_TRY(tmp.need(nin * 12 + nout * 16 + (size_t)nq * 8 + (size_t)std::max<int64_t>(n, 1) * 4));
    int64_t* di = tmp.as<int64_t>();
    int64_t* doi = di + nin;
    float* ds = (float*)(doi + nout);
    float* dos = ds + nin;
    int32_t* dg = (int32_t*)(dos + nout);
    int32_t* dfound = dg + nout;
    int32_t* dcomplete = dfound + nq;
    int32_t* dcol = dcomplete + nq;
    a.scores = ds;
    a.idx = di;
    a.column = dcol;
    a.out_scores = dos;
    a.out_idx = doi;
    a.out_groups = dg;
    a.out_found = dfound;
    a.out_complete = dcomplete;
    // from here on every path drains the stream before `tmp` is freed: failures are kept in rc, not returned
    auto enqueue = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(ds, scores, nin * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(di, idx, nin * 8, hipMemcpyHostToDevice, st));
        if (n) HIP_TRY(hipMemcpyAsync(dcol, column, (size_t)n * 4, hipMemcpyHostToDevice, st));
        TS_TRY(collapse_launch(a, nq, st));
        HIP_TRY(hipMemcpyAsync(out_scores, dos, nout * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_idx, doi, nout * 8, hipMemcpyDeviceToHost, st));
        if (out_groups) HIP_TRY(hipMemcpyAsync(out_groups, dg, nout * 4, hipMemcpyDeviceToHost, st));
        if (out_found) HIP_TRY(hipMemcpyAsync(out_found, dfound, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
        if (out_complete) HIP_TRY(hipMemcpyAsync(out_complete, dcomplete, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
        return TS_OK;
    };
    const int rc = enqueue();
    const hipError_t e = hipStreamSynchronize(st);
    TS_TRY(rc);
    if (e != hipSuccess) return fail(TS_ERR_HIP, "the collapse failed: %s", hipGetErrorString(e));
    return TS_OK;
}

// ---- the exclusion mask ---------------------------------------------------------------------------------------------------
// The lists of one exclusion on the device, and its count: codes [256] | rows [256] | count.  `codes` / `rows` are sorted.
struct ExcludeLists {
    DevBuf buf;
    int64_t* rows() { return buf.as<int64_t>(); }
    u64* count() { return (u64*)(rows() + kGroupMaxList); }
    int32_t* codes() { return (int32_t*)(count() + 1); }
    int ensure() { return (int)buf.need((size_t)kGroupMaxList * 12 + 8); }
};

// everything one exclusion enqueues on `st`: the lists' upload, the kernel, the count's way back.  The host arrays must
// stay alive until the stream has run that far (both callers wait for the count).
static int exclude_enqueue(int cu_count, int64_t n, const u32* base, const int32_t* column, const int32_t* codes, int ncodes,
                           const int64_t* rows, int nrows, ExcludeLists* lists, u32* mask, u64* count_host, hipStream_t st) {
    if (ncodes) HIP_TRY(hipMemcpyAsync(lists->codes(), codes, (size_t)ncodes * 4, hipMemcpyHostToDevice, st));
    if (nrows) HIP_TRY(hipMemcpyAsync(lists->rows(), rows, (size_t)nrows * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(lists->count(), 0, 8, st));
    GroupExcludeArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.nblocks = mask_blocks(n);
    a.base = base;
    a.column = column;
    a.codes = lists->codes();
    a.rows = lists->rows();
    a.ncodes = ncodes;
    a.nrows = nrows;
    a.mask = mask;
    a.allowed = lists->count();
    group_exclude_kernel<<<meta_grid(cu_count, n), kMetaThreads, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(count_host, lists->count(), 8, hipMemcpyDeviceToHost, st));
    return TS_OK;
}

// the scalar column `col` of `m` as the kernels read it; the wording of ts_index_group_sums
static int group_column(const ts_meta* m, int32_t col, const int32_t** column) {
    if (col < 0 || col >= m->ncols) return fail(TS_ERR_INVALID, "column %d outside [0, %d)", col, m->ncols);
    std::lock_guard<std::mutex> lock(const_cast<ts_meta*>(m)->mu);
    if (m->kind[col] == kMetaColList) return fail(TS_ERR_INVALID, "column %d is a list column", col);
    if (m->kind[col] != kMetaColScalar) return fail(TS_ERR_INVALID, "column %d was never set", col);
    *column = m->values[col].as<int32_t>();
    return TS_OK;
}

extern "C" int ts_rowset_exclude(ts_meta* m, int32_t col, const ts_rowset* base, const int32_t* codes, int32_t ncodes,
                                 const int64_t* local_rows, int32_t nrows, ts_rowset** out, void* stream) {
    if (out) *out = nullptr;
    if (const char* bad = exclude_args_invalid(m, out, codes, ncodes, local_rows, nrows, m ? m->n : 0))
        return fail(TS_ERR_INVALID, "ts_rowset_exclude (ncodes = %d, nrows = %d): %s", ncodes, nrows, bad);
    if (base && base->n != m->n) return fail(TS_ERR_INVALID, "the row set has %lld rows, the meta table %lld", (long long)base->n, (long long)m->n);
    if (base && base->device != m->device) return fail(TS_ERR_INVALID, "the row set lives on device %d, the meta table on device %d", base->device, m->device);
    const int32_t* column = nullptr;
    TS_TRY(group_column(m, col, &column));
    std::vector<int32_t> scodes(codes, codes + ncodes);
    std::vector<int64_t> srows(local_rows, local_rows + nrows);
    const int nc = sort_unique(scodes.data(), ncodes), nr = sort_unique(srows.data(), nrows);
    HIP_TRY(hipSetDevice(m->device));
    std::unique_ptr<ts_rowset> r(new (std::nothrow) ts_rowset());
    if (!r) return fail(TS_ERR_NOMEM, "host allocation failed");
    r->device = m->device;
    r->n = m->n;
    DEV_TRY(r->mask.need((size_t)mask_alloc_words(m->n) * 4));
    ExcludeLists lists;
    DEV_TRY(lists.ensure());
    hipStream_t st = (hipStream_t)stream;
    u64 allowed = 0;
    const int rc = exclude_enqueue(m->cu_count, m->n, base ? base->mask.as<u32>() : nullptr, column, scodes.data(), nc, srows.data(), nr,
                                   &lists, r->mask, &allowed, st);
    // the lists, `allowed` and (on failure) the row set's mask go out of scope behind this: the stream is drained first, always
    const hipError_t e = hipStreamSynchronize(st);
    TS_TRY(rc);
    if (e != hipSuccess) return fail(TS_ERR_HIP, "the exclusion failed: %s", hipGetErrorString(e));
    r->allowed = (int64_t)allowed;
    *out = r.release();
    return TS_OK;
}

// ---- the grouped search ---------------------------------------------------------------------------------------------------
namespace {

struct GroupedCall {
    ts_index* ix;
    const char* queries;
    size_t q_row_bytes;
    int q_dtype, q_on_device, k;
    const int32_t* column;
    const u32* base_mask;           // the row set's, or NULL
    int64_t base_allowed;           // ... and its count (-1 without one)
    void* stream;                   // as the caller gave it: what the searches take
    hipStream_t st;                 // the stream that means
    // device scratch of the call
    DevArray<float> list_s;   DevArray<int64_t> list_i;          // [nq x deep] the lists the searches write
    DevArray<float> res_s;    DevArray<int64_t> res_i;   DevArray<int32_t> res_g;   // [nq x k] the answer
    DevArray<int32_t> cert;                                     // [nq] found | [nq] complete | [nq] qmap
};

// one search of `nq` queries at depth `depth` into the call's lists (device results: enqueued, not waited for)
int grouped_search(GroupedCall& c, const void* queries, int q_on_device, int nq, int depth, int algo, const u32* mask, int64_t allowed,
                   ts_search_stats* stats) {
    return search_core(c.ix, queries, c.q_dtype, q_on_device, nq, depth, c.list_s, c.list_i, 1, c.stream, algo, stats, mask, allowed);
}

// collapse the first `nq` lists of depth k_in into k_out slots per query of (out_s, out_i, out_g); certificates to cert
int grouped_collapse(GroupedCall& c, int nq, int k_in, int k_out, const int32_t* qmap, float* out_s, int64_t* out_i, int32_t* out_g,
                     int32_t* found, int32_t* complete) {
    CollapseArgs a;
    memset(&a, 0, sizeof(a));
    a.scores = c.list_s;
    a.idx = c.list_i;
    a.k_in = k_in;
    a.k_out = k_out;
    a.column = c.column;
    a.n = c.ix->n;
    a.row_offset = c.ix->row_offset;
    a.qmap = qmap;
    a.out_scores = out_s;
    a.out_idx = out_i;
    a.out_groups = out_g;
    a.out_found = found;
    a.out_complete = complete;
    return collapse_launch(a, nq, c.st);
}

// Stage 3 for query q: scan passes behind the base mask without the groups found so far, until k groups or no rows are
// left.  The first pass excludes nothing and replaces what the earlier stages found: every score of the query then comes
// from passes of one call shape, and the mask only gates whether a key is made (kernels_scan.h), so appended entries
// keep the canonical order.
int grouped_exclude_query(GroupedCall& c, int q, const ts_meta* m, ExcludeLists& lists, DevArray<u32>& xmask, int* passes) {
    const int k = c.k, deep = group_deep_depth();
    std::vector<float> hs((size_t)k, -INFINITY), rs((size_t)k);         // the answer so far; what a round found
    std::vector<int64_t> hi((size_t)k, -1), ri((size_t)k);
    std::vector<int32_t> hg((size_t)k, TS_META_NULL), rg((size_t)k);
    std::vector<int32_t> codes;
    std::vector<int64_t> rows;
    int32_t* d_found = c.cert;      // a round's found | complete: the earlier stages' certificates are read already
    float* tmp_s = c.res_s.as<float>() + (size_t)q * k;       // a round collapses into the query's own slots: list 0 -> row q
    int64_t* tmp_i = c.res_i.as<int64_t>() + (size_t)q * k;
    int32_t* tmp_g = c.res_g.as<int32_t>() + (size_t)q * k;
    int have = 0;
    for (int round = 0;; ++round) {
        if (round > k) return fail(TS_ERR_INTERNAL, "grouped search: query %d found no new group in an exclusion pass", q);
        u64 allowed = 0;
        TS_TRY(exclude_enqueue(m->cu_count, c.ix->n, c.base_mask, c.column, codes.data(), (int)codes.size(), rows.data(), (int)rows.size(),
                               &lists, xmask, &allowed, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
        const void* qsrc = c.queries + (size_t)q * c.q_row_bytes;
        TS_TRY(grouped_search(c, qsrc, c.q_on_device, 1, deep, TS_ALGO_SCAN, xmask, (int64_t)allowed, nullptr));
        ++*passes;
        const int want = k - have;
        TS_TRY(grouped_collapse(c, 1, deep, want, nullptr, tmp_s, tmp_i, tmp_g, d_found, d_found + 1));
        int32_t cert[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(rs.data(), tmp_s, (size_t)want * 4, hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipMemcpyAsync(ri.data(), tmp_i, (size_t)want * 8, hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipMemcpyAsync(rg.data(), tmp_g, (size_t)want * 4, hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipMemcpyAsync(cert, d_found, 8, hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
        const int fresh = std::min<int>(cert[0], want);
        for (int j = 0; j < fresh; ++j) {
            hs[have + j] = rs[j];
            hi[have + j] = ri[j];
            hg[have + j] = rg[j];
            if (rg[j] == TS_META_NULL) rows.push_back(ri[j] - c.ix->row_offset);
            else codes.push_back(rg[j]);
        }
        have += fresh;
        if (cert[1]) break;
        std::sort(codes.begin(), codes.end());
        std::sort(rows.begin(), rows.end());
    }
    HIP_TRY(hipMemcpyAsync(tmp_s, hs.data(), (size_t)k * 4, hipMemcpyHostToDevice, c.st));
    HIP_TRY(hipMemcpyAsync(tmp_i, hi.data(), (size_t)k * 8, hipMemcpyHostToDevice, c.st));
    HIP_TRY(hipMemcpyAsync(tmp_g, hg.data(), (size_t)k * 4, hipMemcpyHostToDevice, c.st));
    HIP_TRY(hipStreamSynchronize(c.st));     // the host arrays go out of scope
    return TS_OK;
}

// the ladder; everything it enqueues may still be in flight when it returns with an error (the caller drains the stream)
int grouped_ladder(GroupedCall& c, const ts_meta* m, int nq, int algo, ts_grouped_stats* gs) {
    const int k = c.k, first = group_first_depth(k), deep = group_deep_depth();
    int32_t* d_found = c.cert;
    int32_t* d_complete = d_found + nq;
    int32_t* d_qmap = d_complete + nq;
    // stage 1: the ordinary search, over-fetched
    ts_search_stats ss;
    TS_TRY(grouped_search(c, c.queries, c.q_on_device, nq, first, algo, c.base_mask, c.base_allowed, &ss));
    gs->algo = ss.algo;
    TS_TRY(grouped_collapse(c, nq, first, k, nullptr, c.res_s, c.res_i, c.res_g, d_found, d_complete));
    std::vector<int32_t> complete((size_t)nq);
    HIP_TRY(hipMemcpyAsync(complete.data(), d_complete, (size_t)nq * 4, hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    std::vector<int32_t> open;
    for (int q = 0; q < nq; ++q)
        if (!complete[q]) open.push_back(q);
    // stage 2: the open queries, gathered, at the library's depth
    DevBuf gathered;
    std::vector<char> gathered_host;
    if (!open.empty() && group_has_deep_stage(k)) {
        const int no = (int)open.size();
        gs->deep_queries = no;
        const void* gq = nullptr;
        if (c.q_on_device) {
            DEV_TRY(gathered.need((size_t)no * c.q_row_bytes));
            for (int i = 0; i < no; ++i)
                HIP_TRY(hipMemcpyAsync(gathered.as<char>() + (size_t)i * c.q_row_bytes, c.queries + (size_t)open[i] * c.q_row_bytes, c.q_row_bytes,
                                       hipMemcpyDeviceToDevice, c.st));
            gq = gathered.as<char>();
        } else {
            gathered_host.resize((size_t)no * c.q_row_bytes);
            for (int i = 0; i < no; ++i)
                memcpy(gathered_host.data() + (size_t)i * c.q_row_bytes, c.queries + (size_t)open[i] * c.q_row_bytes, c.q_row_bytes);
            gq = gathered_host.data();
        }
        TS_TRY(grouped_search(c, gq, c.q_on_device, no, deep, algo == TS_ALGO_SCAN ? TS_ALGO_SCAN : TS_ALGO_AUTO, c.base_mask, c.base_allowed, nullptr));
        HIP_TRY(hipMemcpyAsync(d_qmap, open.data(), (size_t)no * 4, hipMemcpyHostToDevice, c.st));
        TS_TRY(grouped_collapse(c, no, deep, k, d_qmap, c.res_s, c.res_i, c.res_g, d_found, d_complete));
        HIP_TRY(hipMemcpyAsync(complete.data(), d_complete, (size_t)nq * 4, hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
        std::vector<int32_t> still;
        for (int q : open)
            if (!complete[q]) still.push_back(q);
        open.swap(still);
    }
    // stage 3: the exact backstop, one query at a time
    if (!open.empty()) {
        ExcludeLists lists;
        DEV_TRY(lists.ensure());
        DevArray<u32> xmask;
        DEV_TRY(xmask.need((size_t)mask_alloc_words(c.ix->n) * 4));
        gs->excluded_queries = (int)open.size();
        for (int q : open) TS_TRY(grouped_exclude_query(c, q, m, lists, xmask, &gs->exclusion_passes));
    }
    return TS_OK;
}

}  // namespace

extern "C" int ts_search_grouped(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k, ts_meta* m,
                                 int32_t col, const ts_rowset* rows, float* out_scores, int64_t* out_idx, int32_t* out_groups,
                                 int out_on_device, void* stream, int algo, ts_grouped_stats* stats) {
    ts_grouped_stats gs;
    memset(&gs, 0, sizeof(gs));
    if (stats) *stats = gs;
    if (const char* bad = grouped_args_invalid(ix, queries, m, out_scores, out_idx, q_dtype, nq, k, algo))
        return fail(TS_ERR_INVALID, "ts_search_grouped (nq = %d, k = %d): %s", nq, k, bad);
    if (ix->id_map) return fail(TS_ERR_UNSUPPORTED, "grouped search on a subset index");
    if (m->n != ix->n) return fail(TS_ERR_INVALID, "the meta table has %lld rows, the index %lld", (long long)m->n, (long long)ix->n);
    if (m->device != ix->device) return fail(TS_ERR_INVALID, "the meta table lives on device %d, the index on device %d", m->device, ix->device);
    if (rows && rows->n != ix->n) return fail(TS_ERR_INVALID, "the row set has %lld rows, the index %lld", (long long)rows->n, (long long)ix->n);
    if (rows && rows->device != ix->device) return fail(TS_ERR_INVALID, "the row set lives on device %d, the index on device %d", rows->device, ix->device);
    GroupedCall c;
    TS_TRY(group_column(m, col, &c.column));
    gs.depth = group_first_depth(k);
    if (stats) *stats = gs;
    if (nq == 0) return TS_OK;
    HIP_TRY(hipSetDevice(ix->device));
    c.ix = ix;
    c.queries = (const char*)queries;
    c.q_row_bytes = (size_t)ix->d * (q_dtype == TS_BF16 ? 2 : 4);
    c.q_dtype = q_dtype;
    c.q_on_device = q_on_device;
    c.k = k;
    c.base_mask = rows ? rows->mask.as<u32>() : nullptr;
    c.base_allowed = rows ? rows->allowed : -1;
    c.stream = stream;
    c.st = stream ? (hipStream_t)stream : ix->stream;
    const size_t nlist = (size_t)nq * group_deep_depth(), nres = (size_t)nq * k;
    DEV_TRY(c.list_s.need(nlist * 4));
    DEV_TRY(c.list_i.need(nlist * 8));
    DEV_TRY(c.res_s.need(nres * 4));
    DEV_TRY(c.res_i.need(nres * 8));
    DEV_TRY(c.res_g.need(nres * 4));
    DEV_TRY(c.cert.need((size_t)std::max(nq, 1) * 12 + 8));
    int rc = grouped_ladder(c, m, nq, algo, &gs);
    if (rc == TS_OK) {
        const hipMemcpyKind kind = out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        hipError_t e = hipMemcpyAsync(out_scores, c.res_s, nres * 4, kind, c.st);
        if (e == hipSuccess) e = hipMemcpyAsync(out_idx, c.res_i, nres * 8, kind, c.st);
        if (e == hipSuccess && out_groups) e = hipMemcpyAsync(out_groups, c.res_g, nres * 4, kind, c.st);
        if (e != hipSuccess) rc = fail(TS_ERR_HIP, "copy of the grouped results failed: %s", hipGetErrorString(e));
    }
    // the call's scratch goes out of scope behind this: the stream is drained first, always
    const hipError_t e = hipStreamSynchronize(c.st);
    TS_TRY(rc);
    if (e != hipSuccess) return fail(TS_ERR_HIP, "the grouped search failed: %s", hipGetErrorString(e));
    if (stats) *stats = gs;
    return TS_OK;
}
