// libtsearch.so - C ABI (include/tsearch.h), part 5: ts_rank_many, the ranks of many target rows per query in one matrix
// pass per block of 256 queries and per kRankT targets (kernels_rank_mfma.h).  Other widths fall back to ts_rank_of, one
// streaming pass per target column: correct and slow.
#include <algorithm>
#include <vector>

#include "host.h"
#include "kernels_rank_mfma.h"

static inline bool rank_many_width(const ts_index* ix) {
    return (ix->dtype == TS_BF16 || ix->dtype == TS_F32) && mfma_dim(ix->d) && ix->ld == ix->d;
}

static u64 host_key(float s, int64_t row) {
    return ((u64)host_ord_f32(s) << 32) | (u64)(0xFFFFFFFFu - (u32)row);
}

template <bool F32, int RB, bool GATHER>
static int launch_rank_many_t(int dev, int grid, int lds, hipStream_t st, const RankManyArgs& a) {
    // the largest row of its RB (rank_rb): 2,048 bytes at RB = 4, 4,096 (fp32 at d = 1024) at RB = 2
    constexpr int kMaxLds = rank_lds_bytes(RB, RB == 4 ? 2048 : 4096);
    static_assert(kMaxLds <= 160 * 1024, "a tile must fit the CU's LDS");
    return launch_lds<rank_many_kernel<F32, RB, GATHER>, kMaxLds>(dev, grid, kRankThreads, lds, st, a);
}

static int launch_rank_many(const ts_index* ix, bool gather, int grid, hipStream_t st, const RankManyArgs& a) {
    const int row_bytes = (int)ix->ld * ix->elem();
    const int rb = rank_rb(row_bytes);
    const int lds = rank_lds_bytes(rb, row_bytes);
    const bool f32 = ix->dtype == TS_F32;
    if (f32 && rb == 4) return gather ? launch_rank_many_t<true, 4, true>(ix->device, grid, lds, st, a) : launch_rank_many_t<true, 4, false>(ix->device, grid, lds, st, a);
    if (f32) return gather ? launch_rank_many_t<true, 2, true>(ix->device, grid, lds, st, a) : launch_rank_many_t<true, 2, false>(ix->device, grid, lds, st, a);
    if (rb == 4) return gather ? launch_rank_many_t<false, 4, true>(ix->device, grid, lds, st, a) : launch_rank_many_t<false, 4, false>(ix->device, grid, lds, st, a);
    return fail(TS_ERR_INTERNAL, "no rank_many kernel for a bf16 row of %d bytes", row_bytes);
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

extern "C" int ts_rank_many(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq,
                            const int64_t* target_offsets, const int64_t* target_rows, int64_t* out_rank, float* out_score,
                            void* stream) {
    if (!ix || !queries || !target_offsets || !out_rank) return fail(TS_ERR_INVALID, "NULL argument");
    if (q_dtype != TS_F32 && q_dtype != TS_BF16) return fail(TS_ERR_INVALID, "q_dtype %d", q_dtype);
    if (nq < 0) return fail(TS_ERR_INVALID, "nq = %d", nq);
    if (target_offsets[0] != 0) return fail(TS_ERR_INVALID, "target_offsets[0] = %lld, not 0", (long long)target_offsets[0]);
    for (int i = 0; i < nq; ++i)
        if (target_offsets[i + 1] < target_offsets[i])
            return fail(TS_ERR_INVALID, "target_offsets decrease at query %d", i);
    if (nq == 0 || target_offsets[nq] == 0) return TS_OK;
    if (!target_rows) return fail(TS_ERR_INVALID, "target_rows is NULL");
    if (ix->id_map) return fail(TS_ERR_UNSUPPORTED, "rank / count on a subset index");
    if (!rank_many_width(ix))
        return rank_many_fallback(ix, queries, q_dtype, q_on_device, nq, target_offsets, target_rows, out_rank, out_score, stream);

    std::lock_guard<std::mutex> lock(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st;
    StreamScope scope;
    TS_TRY(enter_stream(ix, stream, &st, &scope));
    QueryFeed feed;
    TS_TRY(query_feed_open(&feed, ix, queries, q_dtype, q_on_device, nq, false, st));
    constexpr int kSlots = kQBlock * kRankT;
    DEV_TRY(ix->rank_many_buf.need((size_t)kSlots * (8 + 8 + 4 + 4 + 4) + (size_t)kQBlock * 8));
    int64_t* d_grow = ix->rank_many_buf.as<int64_t>();
    u64* d_tkeys = (u64*)(d_grow + kSlots);
    float* d_gscore = (float*)(d_tkeys + kSlots);
    int* d_gquery = (int*)(d_gscore + kSlots);
    u32* d_counts = (u32*)(d_gquery + kSlots);
    int* d_tcount = (int*)(d_counts + kSlots);
    float* d_tworst = (float*)(d_tcount + kQBlock);

    std::vector<int64_t> grow(kSlots), tslot(kSlots);   // tslot: index of the slot's target in target_rows
    std::vector<int> gquery(kSlots), tcount(kQBlock);
    std::vector<float> gscore(kSlots), tworst(kQBlock);
    std::vector<u64> tkeys(kSlots);
    std::vector<u32> counts(kSlots);
    const float nan = __builtin_nanf("");
    const int64_t tile_rows = 16 * rank_rb((int)ix->ld * ix->elem());

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
                        grow[ns] = r;
                        gquery[ns] = i;
                        tslot[ns] = t;
                        ++ns;
                    } else {
                        out_rank[t] = -1;
                        if (out_score) out_score[t] = nan;
                    }
                }
            }
            if (ns == 0) continue;
            // 2. gather: the targets' scores, by the same arithmetic as the counting pass
            HIP_TRY(hipMemcpyAsync(d_grow, grow.data(), (size_t)ns * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_gquery, gquery.data(), (size_t)ns * 4, hipMemcpyHostToDevice, st));
            RankManyArgs a;
            memset(&a, 0, sizeof(a));
            a.corpus = ix->rows;
            a.n = ix->n;
            a.ld = (int)ix->ld;
            a.q = ix->qstore;
            a.nq = nb;
            a.grow = d_grow;
            a.gquery = d_gquery;
            a.nslots = ns;
            a.gscore = d_gscore;
            TS_TRY(launch_rank_many(ix, true, (int)((ns + tile_rows - 1) / tile_rows), st, a));
            HIP_TRY(hipMemcpyAsync(gscore.data(), d_gscore, (size_t)ns * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            // 3. per query: the target keys best first (NaN scores rank nowhere), padded with a key nothing beats
            std::fill(tkeys.begin(), tkeys.begin() + (size_t)nb * kRankT, ~0ull);
            std::fill(tcount.begin(), tcount.begin() + nb, 0);
            std::fill(tworst.begin(), tworst.begin() + nb, nan);
            for (int64_t s = 0; s < ns; ++s) {
                const float sc = gscore[s];
                if (sc == sc) tkeys[(size_t)gquery[s] * kRankT + tcount[gquery[s]]++] = host_key(sc, grow[s]);
            }
            bool any = false;
            for (int i = 0; i < nb; ++i) {
                if (tcount[i] == 0) continue;
                any = true;
                u64* k = tkeys.data() + (size_t)i * kRankT;
                std::sort(k, k + tcount[i], [](u64 x, u64 y) { return x > y; });
                const u32 hi = (u32)(k[tcount[i] - 1] >> 32);
                const u32 u = (hi & 0x80000000u) ? (hi & 0x7FFFFFFFu) : ~hi;
                memcpy(&tworst[i], &u, 4);
            }
            // 4. the counting pass: rows whose key beats each target key
            if (any) {
                HIP_TRY(hipMemcpyAsync(d_tkeys, tkeys.data(), (size_t)nb * kRankT * 8, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(d_tcount, tcount.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(d_tworst, tworst.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)nb * kRankT * 4, st));
                a.ntiles = (ix->n + tile_rows - 1) / tile_rows;
                a.tkeys = d_tkeys;
                a.tcount = d_tcount;
                a.tworst = d_tworst;
                a.counts = d_counts;
                hipEvent_t stop = prof_begin(ix, st, ix->n);
                TS_TRY(launch_rank_many(ix, false, ix->cu_count, st, a));
                prof_end(stop, st);
                HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, (size_t)nb * kRankT * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
            }
            // 5. each target's rank: the count of its key (a repeated row shares its key and its rank)
            for (int64_t s = 0; s < ns; ++s) {
                const int64_t t = tslot[s];
                const float sc = gscore[s];
                if (out_score) out_score[t] = sc;
                out_rank[t] = -1;
                if (sc != sc) continue;
                const int i = gquery[s];
                const u64 key = host_key(sc, grow[s]);
                const u64* k = tkeys.data() + (size_t)i * kRankT;
                for (int j = 0; j < tcount[i]; ++j)
                    if (k[j] == key) {
                        out_rank[t] = (int64_t)counts[(size_t)i * kRankT + j];
                        break;
                    }
            }
        }
    }
    return TS_OK;
}
