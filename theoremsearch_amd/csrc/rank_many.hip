// libtsearch.so - C ABI (include/tsearch.h), part 5: ts_rank_many, the ranks of many target rows per query, and
// ts_count_above_many, its form for documents that live on other shards: one matrix pass per block of 256 queries and per
// kRankT targets at every width of rank_many_served (rank_plan.h; kernels_rank_mfma.h, whole rows in LDS) and of rank_wide_served
// (rank_wide_plan.h; kernels_rank_wide.h, rows staged k-chunk by k-chunk).  Other widths fall back to ts_rank_of /
// ts_count_above, one streaming pass per target column: correct and slow.
#include <algorithm>
#include <vector>

#include "host.h"
#include "kernels_rank_mfma.h"
#include "kernels_rank_wide.h"

static_assert(kRankQueries == kQBlock, "one launch holds one block of the query feed");
static_assert(kRowPad % rank_wide_tile_rows() == 0, "whole 64-row tiles inside the padded allocation");

static inline bool rank_many_width(const ts_index* ix) { return rank_many_served(ix->dtype, ix->d) && ix->ld == ix->d; }
// the k-chunked widths: whatever TS_MFMA_F32 says and whatever the index size, as the narrower rank pass
static inline bool rank_wide_width(const ts_index* ix) { return rank_wide_served(ix->dtype, ix->d) && ix->ld == ix->d; }
static inline bool rank_matrix_width(const ts_index* ix) { return rank_many_width(ix) || rank_wide_width(ix); }

static u64 host_key(float s, int64_t row) {
    return ((u64)host_ord_f32(s) << 32) | (u64)(0xFFFFFFFFu - (u32)row);
}

template <bool F32, int RB, bool TAIL>
static int launch_rank_many_t(int dev, bool gather, int grid, int lds, hipStream_t st, const RankManyArgs& a) {
    if (gather) return launch_lds<rank_many_kernel<F32, RB, true, TAIL>, rank_lds_max(RB)>(dev, grid, kRankThreads, lds, st, a);
    return launch_lds<rank_many_kernel<F32, RB, false, TAIL>, rank_lds_max(RB)>(dev, grid, kRankThreads, lds, st, a);
}

// every served width has its kernel: storage type x RB (rank_rb) x tail group (rank_tail, bf16 only) x mode
static int launch_rank_many(const ts_index* ix, bool gather, int grid, hipStream_t st, const RankManyArgs& a) {
    if (rank_wide_width(ix)) {
        // the k-chunked form: storage type x mode, the two chunk buffers whatever the width
        constexpr int lds = rank_wide_lds_bytes();
        if (ix->dtype == TS_F32)
            return gather ? launch_lds<rank_wide_kernel<true, true>, lds>(ix->device, grid, kWideThreads, lds, st, a)
                          : launch_lds<rank_wide_kernel<true, false>, lds>(ix->device, grid, kWideThreads, lds, st, a);
        return gather ? launch_lds<rank_wide_kernel<false, true>, lds>(ix->device, grid, kWideThreads, lds, st, a)
                      : launch_lds<rank_wide_kernel<false, false>, lds>(ix->device, grid, kWideThreads, lds, st, a);
    }
    const int row_bytes = (int)ix->ld * ix->elem();
    const int rb = rank_rb(row_bytes);
    const int lds = rank_lds_bytes(rb, row_bytes);
    if (ix->dtype == TS_F32)
        return rb == 4 ? launch_rank_many_t<true, 4, false>(ix->device, gather, grid, lds, st, a) : launch_rank_many_t<true, 2, false>(ix->device, gather, grid, lds, st, a);
    if (rank_tail(ix->dtype, (int)ix->ld))
        return rb == 4 ? launch_rank_many_t<false, 4, true>(ix->device, gather, grid, lds, st, a) : launch_rank_many_t<false, 2, true>(ix->device, gather, grid, lds, st, a);
    return rb == 4 ? launch_rank_many_t<false, 4, false>(ix->device, gather, grid, lds, st, a) : launch_rank_many_t<false, 2, false>(ix->device, gather, grid, lds, st, a);
}

// the argument checks both entries share; *empty: nothing to do
static int rank_many_check(const ts_index* ix, const void* queries, int q_dtype, int32_t nq, const int64_t* off, const void* out,
                           bool* empty) {
    if (!ix || !queries || !off || !out) return fail(TS_ERR_INVALID, "NULL argument");
    if (q_dtype != TS_F32 && q_dtype != TS_BF16) return fail(TS_ERR_INVALID, "q_dtype %d", q_dtype);
    if (nq < 0) return fail(TS_ERR_INVALID, "nq = %d", nq);
    if (off[0] != 0) return fail(TS_ERR_INVALID, "target_offsets[0] = %lld, not 0", (long long)off[0]);
    for (int i = 0; i < nq; ++i)
        if (off[i + 1] < off[i]) return fail(TS_ERR_INVALID, "target_offsets decrease at query %d", i);
    *empty = nq == 0 || off[nq] == 0;
    return TS_OK;
}

// rows of a tile of this index's pass (gather: slots), and the workgroups of its counting launch: one per CU; the k-chunked form
// takes TS_MFMA_GRID where set, clamped as the search's pass
static int64_t rank_tile_rows_of(const ts_index* ix) {
    return rank_wide_width(ix) ? rank_wide_tile_rows() : rank_tile_rows((int)ix->ld * (int)ix->elem());
}
static int rank_count_grid(const ts_index* ix) { return rank_wide_width(ix) ? mfma_grid(ix) : ix->cu_count; }

// One pass (kRankT targets of every query of one block) on the device and on the host.  A slot is one target of the pass:
// gquery = its query within the block, tslot = its index in the caller's target arrays, skey = its key in this index's key
// space (~0: a NaN score, which ranks nowhere).
struct RankPass {
    static constexpr int kSlots = kQBlock * kRankT;
    int64_t* d_grow;
    u64* d_tkeys;
    float* d_gscore;
    int* d_gquery;
    u32* d_counts;
    int* d_tcount;
    float* d_tworst;
    std::vector<int64_t> grow, tslot;
    std::vector<int> gquery, tcount;
    std::vector<float> gscore, tworst;
    std::vector<u64> skey, tkeys;
    std::vector<u32> counts;
    RankPass() : grow(kSlots), tslot(kSlots), gquery(kSlots), tcount(kQBlock), gscore(kSlots), tworst(kQBlock), skey(kSlots), tkeys(kSlots), counts(kSlots) {}
    int open(ts_index* ix) {
        DEV_TRY(ix->rank_many_buf.need((size_t)kSlots * (8 + 8 + 4 + 4 + 4) + (size_t)kQBlock * 8));
        d_grow = ix->rank_many_buf.as<int64_t>();
        d_tkeys = (u64*)(d_grow + kSlots);
        d_gscore = (float*)(d_tkeys + kSlots);
        d_gquery = (int*)(d_gscore + kSlots);
        d_counts = (u32*)(d_gquery + kSlots);
        d_tcount = (int*)(d_counts + kSlots);
        d_tworst = (float*)(d_tcount + kQBlock);
        return TS_OK;
    }
};

static RankManyArgs rank_many_args(const ts_index* ix, int nb) {
    RankManyArgs a;
    memset(&a, 0, sizeof(a));
    a.corpus = ix->rows;
    a.n = ix->n;
    a.ld = (int)ix->ld;
    a.q = ix->qstore;
    a.nq = nb;
    return a;
}

// The counting half of a pass, for ns slots whose keys are known: out[tslot[s]] = the rows of this index whose key beats
// skey[s] (-1 for a NaN key).  Slots of one query that share a key share the count.
static int count_pass(ts_index* ix, hipStream_t st, RankPass& w, int nb, int64_t ns, int64_t* out) {
    // per query: the target keys best first, padded with a key nothing beats, and the score of the worst one
    std::fill(w.tkeys.begin(), w.tkeys.begin() + (size_t)nb * kRankT, ~0ull);
    std::fill(w.tcount.begin(), w.tcount.begin() + nb, 0);
    std::fill(w.tworst.begin(), w.tworst.begin() + nb, __builtin_nanf(""));
    for (int64_t s = 0; s < ns; ++s)
        if (w.skey[s] != ~0ull) w.tkeys[(size_t)w.gquery[s] * kRankT + w.tcount[w.gquery[s]]++] = w.skey[s];
    bool any = false;
    for (int i = 0; i < nb; ++i) {
        if (w.tcount[i] == 0) continue;
        any = true;
        u64* k = w.tkeys.data() + (size_t)i * kRankT;
        std::sort(k, k + w.tcount[i], [](u64 x, u64 y) { return x > y; });
        const u32 hi = (u32)(k[w.tcount[i] - 1] >> 32);
        const u32 u = (hi & 0x80000000u) ? (hi & 0x7FFFFFFFu) : ~hi;
        memcpy(&w.tworst[i], &u, 4);
    }
    // the counting pass: rows whose key beats each target key
    if (any) {
        HIP_TRY(hipMemcpyAsync(w.d_tkeys, w.tkeys.data(), (size_t)nb * kRankT * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(w.d_tcount, w.tcount.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(w.d_tworst, w.tworst.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(w.d_counts, 0, (size_t)nb * kRankT * 4, st));
        const int64_t tile_rows = rank_tile_rows_of(ix);
        RankManyArgs a = rank_many_args(ix, nb);
        a.ntiles = (ix->n + tile_rows - 1) / tile_rows;
        a.tkeys = w.d_tkeys;
        a.tcount = w.d_tcount;
        a.tworst = w.d_tworst;
        a.counts = w.d_counts;
        hipEvent_t stop = prof_begin(ix, st, ix->n);
        const int rc = launch_rank_many(ix, false, rank_count_grid(ix), st, a);
        prof_end(stop, st);
        TS_TRY(rc);
        HIP_TRY(hipMemcpyAsync(w.counts.data(), w.d_counts, (size_t)nb * kRankT * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    // each slot's count: the count of its key
    for (int64_t s = 0; s < ns; ++s) {
        const int64_t t = w.tslot[s];
        out[t] = -1;
        if (w.skey[s] == ~0ull) continue;
        const int i = w.gquery[s];
        const u64* k = w.tkeys.data() + (size_t)i * kRankT;
        for (int j = 0; j < w.tcount[i]; ++j)
            if (k[j] == w.skey[s]) {
                out[t] = (int64_t)w.counts[(size_t)i * kRankT + j];
                break;
            }
    }
    return TS_OK;
}

// Other widths: one ts_rank_of per target column (column c = the c-th target of every query that has one)
static int rank_many_fallback(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq,
                              const int64_t* off, const int64_t* rows, int64_t* out_rank, float* out_score, void* stream) {
    int64_t cols = 0;
    for (int i = 0; i < nq; ++i) cols = std::max(cols, off[i + 1] - off[i]);
    std::vector<int64_t> tgt(nq), rk(nq);
    std::vector<float> sc(nq);
    for (int64_t c = 0; c < cols; ++c) {
        for (int i = 0; i < nq; ++i) tgt[i] = (c < off[i + 1] - off[i]) ? rows[off[i] + c] : -1 - ix->row_offset;   // not a row: rank -1
        TS_TRY(ts_rank_of(ix, queries, q_dtype, q_on_device, nq, tgt.data(), rk.data(), sc.data(), stream));
        for (int i = 0; i < nq; ++i)
            if (c < off[i + 1] - off[i]) {
                out_rank[off[i] + c] = rk[i];
                if (out_score) out_score[off[i] + c] = sc[i];
            }
    }
    return TS_OK;
}

// ... and one ts_count_above per target column (a query without a c-th target hands in a NaN score: nothing counts)
static int count_above_many_fallback(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, const int64_t* off,
                                     const float* scores, const int64_t* ids, int64_t* out_counts, void* stream) {
    int64_t cols = 0;
    for (int i = 0; i < nq; ++i) cols = std::max(cols, off[i + 1] - off[i]);
    std::vector<int64_t> id(nq), cnt(nq);
    std::vector<float> sc(nq);
    for (int64_t c = 0; c < cols; ++c) {
        for (int i = 0; i < nq; ++i) {
            const bool has = c < off[i + 1] - off[i];
            sc[i] = has ? scores[off[i] + c] : __builtin_nanf("");
            id[i] = has ? ids[off[i] + c] : 0;
        }
        TS_TRY(ts_count_above(ix, queries, q_dtype, q_on_device, nq, sc.data(), id.data(), cnt.data(), stream));
        for (int i = 0; i < nq; ++i)
            if (c < off[i + 1] - off[i]) out_counts[off[i] + c] = cnt[i];
    }
    return TS_OK;
}

extern "C" int ts_rank_many(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq,
                            const int64_t* target_offsets, const int64_t* target_rows, int64_t* out_rank, float* out_score,
                            void* stream) {
    bool empty = false;
    TS_TRY(rank_many_check(ix, queries, q_dtype, nq, target_offsets, out_rank, &empty));
    if (empty) return TS_OK;
    if (!target_rows) return fail(TS_ERR_INVALID, "target_rows is NULL");
    if (ix->id_map) return fail(TS_ERR_UNSUPPORTED, "rank / count on a subset index");
    if (!rank_matrix_width(ix))
        return rank_many_fallback(ix, queries, q_dtype, q_on_device, nq, target_offsets, target_rows, out_rank, out_score, stream);

    std::lock_guard<std::mutex> lock(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st;
    StreamScope scope;
    TS_TRY(enter_stream(ix, stream, &st, &scope));
    QueryFeed feed;
    TS_TRY(query_feed_open(&feed, ix, queries, q_dtype, q_on_device, nq, false, st));
    RankPass w;
    TS_TRY(w.open(ix));
    const float nan = __builtin_nanf("");
    const int64_t tile_rows = rank_tile_rows_of(ix);

    for (int q0 = 0; q0 < nq; q0 += kQBlock) {
        const int nb = std::min(kQBlock, nq - q0);
        int64_t longest = 0;
        for (int i = 0; i < nb; ++i) longest = std::max(longest, target_offsets[q0 + i + 1] - target_offsets[q0 + i]);
        if (longest == 0) continue;
        TS_TRY(query_feed_block(feed, q0, nb));
        // pass p: targets p * kRankT .. p * kRankT + kRankT - 1 of every query
        for (int64_t p0 = 0; p0 < longest; p0 += kRankT) {
            // 1. slots: the targets of this pass that are rows of this index
            int64_t ns = 0;
            for (int i = 0; i < nb; ++i) {
                const int64_t b = target_offsets[q0 + i] + p0, e = std::min(target_offsets[q0 + i + 1], b + kRankT);
                for (int64_t t = b; t < e; ++t) {
                    const int64_t r = target_rows[t] - ix->row_offset;
                    if (r >= 0 && r < ix->n) {
                        w.grow[ns] = r;
                        w.gquery[ns] = i;
                        w.tslot[ns] = t;
                        ++ns;
                    } else {
                        out_rank[t] = -1;
                        if (out_score) out_score[t] = nan;
                    }
                }
            }
            if (ns == 0) continue;
            // 2. gather: the targets' scores, by the same arithmetic as the counting pass
            HIP_TRY(hipMemcpyAsync(w.d_grow, w.grow.data(), (size_t)ns * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.d_gquery, w.gquery.data(), (size_t)ns * 4, hipMemcpyHostToDevice, st));
            RankManyArgs a = rank_many_args(ix, nb);
            a.grow = w.d_grow;
            a.gquery = w.d_gquery;
            a.nslots = ns;
            a.gscore = w.d_gscore;
            TS_TRY(launch_rank_many(ix, true, (int)((ns + tile_rows - 1) / tile_rows), st, a));
            HIP_TRY(hipMemcpyAsync(w.gscore.data(), w.d_gscore, (size_t)ns * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            // 3. - 5. the keys (NaN scores rank nowhere), the counting pass, each target's rank: the count of its key (a
            // repeated row shares its key and its rank)
            for (int64_t s = 0; s < ns; ++s) {
                const float sc = w.gscore[s];
                w.skey[s] = sc == sc ? host_key(sc, w.grow[s]) : ~0ull;
                if (out_score) out_score[w.tslot[s]] = sc;
            }
            TS_TRY(count_pass(ix, st, w, nb, ns, out_rank));
        }
    }
    return TS_OK;
}

extern "C" int ts_count_above_many(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq,
                                   const int64_t* target_offsets, const float* target_scores, const int64_t* target_ids,
                                   int64_t* out_counts, void* stream) {
    bool empty = false;
    TS_TRY(rank_many_check(ix, queries, q_dtype, nq, target_offsets, out_counts, &empty));
    if (empty) return TS_OK;
    if (!target_scores || !target_ids) return fail(TS_ERR_INVALID, "target_scores or target_ids is NULL");
    if (ix->id_map) return fail(TS_ERR_UNSUPPORTED, "rank / count on a subset index");
    if (!rank_matrix_width(ix))
        return count_above_many_fallback(ix, queries, q_dtype, q_on_device, nq, target_offsets, target_scores, target_ids, out_counts, stream);

    std::lock_guard<std::mutex> lock(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st;
    StreamScope scope;
    TS_TRY(enter_stream(ix, stream, &st, &scope));
    QueryFeed feed;
    TS_TRY(query_feed_open(&feed, ix, queries, q_dtype, q_on_device, nq, false, st));
    RankPass w;
    TS_TRY(w.open(ix));

    for (int q0 = 0; q0 < nq; q0 += kQBlock) {
        const int nb = std::min(kQBlock, nq - q0);
        int64_t longest = 0;
        for (int i = 0; i < nb; ++i) longest = std::max(longest, target_offsets[q0 + i + 1] - target_offsets[q0 + i]);
        if (longest == 0) continue;
        TS_TRY(query_feed_block(feed, q0, nb));
        for (int64_t p0 = 0; p0 < longest; p0 += kRankT) {
            // every target of the pass is a slot: its key says where the document lies (in, before or behind this index)
            int64_t ns = 0;
            for (int i = 0; i < nb; ++i) {
                const int64_t b = target_offsets[q0 + i] + p0, e = std::min(target_offsets[q0 + i + 1], b + kRankT);
                for (int64_t t = b; t < e; ++t) {
                    w.gquery[ns] = i;
                    w.tslot[ns] = t;
                    w.skey[ns] = count_above_key(target_scores[t], target_ids[t] - ix->row_offset, ix->n);
                    ++ns;
                }
            }
            if (ns) TS_TRY(count_pass(ix, st, w, nb, ns, out_counts));
        }
    }
    return TS_OK;
}
