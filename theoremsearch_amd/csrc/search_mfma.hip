// The matrix path of a search: planning of the threshold levels, the dense threshold sample and its
// select, the full pass (launch_mfma*.hip hold the kernel instantiations), the final select, the exact re-run.
// mfma_search runs the stages in order: mfma_plan (what this search is), mfma_scratch (the handle's buffers), then per level
// mfma_sample (level 0 as the dense sample) or mfma_level (a matrix kernel + its select).  A biased search (ts_search_biased_ex)
// is the general-width form of all this at any served width, with its own sample select (kernels_sample_biased.h).  A search with
// a row set per query (ts_search_rowsets: ix->active_rowsets) is that form too, with the row-set kernels of
// launch_mfma_anyd_rowsets.hip, a table per block of queries (rowsets_table) and a re-run per set (rowsets_rerun).  Both at once
// (ts_search_biased_rowsets: a weight per query in the block's table) is that form with the biased row-set pass, a histogram of the
// raw bias per set (biased_rowsets_histograms), the sample select that reads it through the query's weight, and a re-run per class.
//
// What the plan fixes, as tests/threshold_common.py restates it and tests/test_threshold_gpu.py observes it: level i visits
// tiles j * stride_i, so the sample is the rows 32 j stride + r (r < 32) below n - a partial last tile gives its real rows
// only, and only when its index is a multiple of the stride; ceil(n / 32) * 32 <= first_rows is ONE unthresholded level
// (every live row a candidate of the final select); pop = the rows a host mask allows.  A host mask reaches this path in
// batches only (scan_plan.h: choose_algo).  ts_search_stats' candidates and fallback_queries describe the LAST launch
// block of a call (mfma_block_queries), not the whole batch.
#include "host.h"
#include "kernels_mfma.h"
#include "kernels_mfma16.h"
#include "mfma16_variants.h"
#include "kernels_mfma_f32.h"
#include "kernels_sample.h"
#include "kernels_sample_biased.h"
#include "kernels_biased_rowsets.h"
#include "kernels_level.h"

struct Level { int64_t stride, ntiles; int run; };

// Threshold levels of the MFMA path, sparsest first.  Level i visits runs of `run` consecutive tiles
// every run * stride tiles (stride 1 = every tile = the full pass) and passes on to level i+1 the
// kk-th best score it saw as that level's pass threshold: a lower bound of the final kk-th best, so
// nothing that belongs to the answer is ever dropped.  Expected candidates per query in level i+1 =
// kk * rows(i+1) / rows(i): the full pass is planned for `target` candidates (few trips through
// the append path), the sparser levels for up to kCandCap / 4 (they are short anyway); the first
// level is small enough to run unthresholded.
// (normal_tail_z, the inverse of the standard normal CDF the estimates use: rowsets_plan.h, which restates them per query)
static int mfma_target_cands(const Knobs& kn, int64_t n, int kk) {
    // Cost model fitted on 10M / 1.25M x 768, batch 256: a sample row costs ~0.4 ns, a candidate of the next
    // level ~0.27 us per query (the append path is ~1 us of wave time).  Minimising kk * N * c_row / F + c_cand * F
    // gives F ~ 512 * sqrt(N / 1e7) candidates per query for the full pass.
    int target = (int)(512.0 * std::sqrt(std::max<double>((double)n, 1.0) / 1e7));
    target = std::max(target, 8 * kk);  // large k: keep the level ratio >= 8, or the sparse levels cost as much as the pass
    return std::min(2048, std::max(64, kn.get(K_MFMA_TARGET_CANDS, target)));
}

// Rows the sparsest level may hold (it runs unthresholded: every score becomes a candidate, so at most kLevelSortMax rows -
// what one select sorts - and one tile per workgroup, 16 entries per private list).
// sample size: 8192 rows for large corpora; below 4M rows half of that estimates the threshold as well (the
// guaranteed bound k * N / sample stays small) and its pass + select are 13 us shorter - 2 % of a 1.25M-row shard
static int64_t first_level_rows(const Knobs& kn, int64_t n, bool statistical) {
    const int first_default = (statistical && n < 4000000) ? kLevelSortMax / 2 : kLevelSortMax;
    return std::min<int64_t>(kLevelSortMax, (int64_t)kn.get(K_MFMA_FIRST_ROWS, first_default));
}
// The full pass of a search on this handle sits behind a threshold: the corpus is more than the sparsest level may hold, so
// plan_levels makes at least two levels (whatever k is).
static bool thresholded_pass(const ts_index* ix) {
    const int64_t T = (ix->n + kTileRows - 1) / kTileRows;
    return T * kTileRows > first_level_rows(ix->knobs, ix->n, ix->knobs.get(K_MFMA_STAT, 1) != 0);
}

static std::vector<Level> plan_levels(const Knobs& kn, int64_t n, int kk, bool statistical) {
    const int64_t T = (n + kTileRows - 1) / kTileRows;
    const int target = mfma_target_cands(kn, n, kk);
    auto pow2_ratio = [&](int cands) { int64_t r = 2; while (r * 2 * kk <= cands) r *= 2; return r; };
    const int64_t r_last = pow2_ratio(target);
    const int64_t first_rows = first_level_rows(kn, n, statistical);
    const int64_t r_cap = std::max<int64_t>(2, pow2_ratio(kn.get(K_MFMA_TARGET_SPARSE, 1280)));
    std::vector<Level> lv;
    int64_t stride = 1;
    for (;;) {
        const int64_t nt = (T + stride - 1) / stride;
        // sampling in runs of consecutive tiles (shared DRAM pages / TLB entries) measured no different from
        // single tiles; kept as a knob
        const int run = (stride > 1 && nt >= 8 * 256) ? kn.get(K_MFMA_RUN, 1) : 1;
        lv.push_back({stride, nt, run});
        if (nt * kTileRows <= first_rows) break;  // every score of this level fits: it can run unthresholded
        if (statistical) {
            // one unthresholded sample of up to first_rows rows; its select extrapolates the threshold of the full pass
            int64_t need = 2;
            while (((T + need - 1) / need) * kTileRows > first_rows) need *= 2;
            stride = need;
        } else if (lv.size() == 1) {
            stride *= r_last;
        } else {
            // smallest ratio that reaches the unthresholded size in one step, if the cap allows it
            int64_t need = 2;
            while (need < r_cap && ((T + stride * need - 1) / (stride * need)) * kTileRows > first_rows) need *= 2;
            stride *= need;
        }
    }
    std::reverse(lv.begin(), lv.end());
    return lv;
}

// Queries one launch of the MFMA kernel serves for this index / batch: d = 768 holds two query groups per wave
// (256 queries; one group = half the matrix work when the batch is <= 128), d = 1024 one (128 queries).
// bf16 x 1024 (the production table, rds_schema.sql:50-56: vector(1024)) holds 3 blocks of 16 queries per wave: 192 per
// workgroup.  A batch of 193 .. 256 queries runs as ONE launch of workgroup PAIRS (MfmaArgs::pair): both workgroups of a pair
// walk the same tiles with 128 queries each, two blocks per wave, so the corpus crosses HBM once for the whole batch (the
// pair's second read of a tile is served by the XCD's L2 / the memory-side cache) instead of once per 128 queries.
// (mfma_grid, kMfmaMaxGrid: host.h - the k-chunked rank pass takes the same grid)
// The search in progress is a biased one on the matrix path: whatever the width, its pass is the general-width kernel (256
// queries per launch, full pass only, shared lists only; no screen, pairs, balancing or private lists).
static bool biased_search(const ts_index* ix) { return ix->active_bias_matrix; }
// (the k-chunked kernel of the wider rows is the same form of search: kernels_mfma_wide.h)
// ... or the shared pass of ts_search_rowsets (a row set per query): the general-width kernel again, at the biased search's widths
static bool rowsets_search(const ts_index* ix) { return ix->active_rowsets != nullptr; }
static bool general_width(const ts_index* ix) { return anyd_index(ix) || wide_index(ix) || biased_search(ix) || rowsets_search(ix); }
static bool mfma_pairs(const ts_index* ix, int nq) {
    return !biased_search(ix) && !rowsets_search(ix) && ix->dtype == TS_BF16 && ix->d == 1024 && nq > 192 && use_shape16(ix) && two_level_search(ix) &&
           ix->knobs.get(K_MFMA_PAIR, 1) != 0 && mfma_grid(ix) % 16 == 0;
}

// TS_MFMA_VARIANT names a timing-only form of the int8 screen (diagnostic build only; launch_screen8*.hip)
static bool screen_diag_variant(int variant) {
#ifdef TS_DIAG
    return variant_screen_diag(variant);
#else
    return false;
#endif
}
// This handle's searches run their full pass as the int8 screen + exact rescore (kernels_screen8.h): an index the screen serves
// (screen_usable), the product kernel (or a timing form of the screen), a full pass behind a threshold.  One predicate for the
// pass (mfma_plan) and for the queries a launch holds (mfma_block_queries).
static bool mfma_screened(const ts_index* ix) {
    const int variant = ix->knobs.get(K_MFMA_VARIANT, 0);
    return !biased_search(ix) && !rowsets_search(ix) && use_shape16(ix) && (variant == kVariantProduct || screen_diag_variant(variant)) && thresholded_pass(ix) && screen_usable(ix);
}

int mfma_block_queries(const ts_index* ix, int nq) {
    if (general_width(ix)) return kAnydQueries;
    if (mfma_pairs(ix, nq)) return 256;
    if (ix->dtype == TS_F32) {
        // screened (TS_MFMA_SCREEN_F32): the int8 kernel holds up to four blocks of 16 queries per wave at either width, so the
        // image crosses HBM once for up to 256 queries; the rescore computes every score as the fp32 pass would have.  Only the
        // two-level search is screened (screen_usable): its other launch is the dense sample, which takes any batch - no fp32
        // matrix kernel ever sees more than its one or two blocks
        if (mfma_screened(ix)) return 64 * std::max(1, (std::min(nq, 256) + 63) / 64);
        if (ix->d == 1024) return 64;                          // one block of 16 queries x 4 waves
        if (use_shape16(ix)) return nq <= 64 ? 64 : 128;       // one or two blocks per wave (d = 384, 512, 768)
        return kMfmaF32Queries;                                // 32x32x2 kernel: 32 queries x 4 waves
    }
    if (use_shape16(ix)) {
        // 16 queries x NB blocks x 4 waves; d = 1024 has registers for 3 blocks per wave, and a batch of more than 192
        // queries is cut into equal launches (two of 128 for 256: both then stream at the HBM rate)
        const int max_nb = ix->d == 1024 ? 3 : 4;
        const int blocks = (std::min(nq, 256) + 63) / 64;
        if (blocks <= max_nb) return 64 * std::max(1, blocks);
        return 64 * ((blocks + 1) / 2);
    }
    if (ix->d == 1024) return 128;
    return nq <= 128 && ix->knobs.get(K_MFMA_GROUPS, 0) != 2 ? 128 : 256;
}

// Once per biased matrix search, before its first block of queries: the histogram of w * bias[row] over every row the call may
// return (kernels_sample_biased.h) - two short passes over the bias array and the mask, n * 4 bytes each.
int bias_histogram(ts_index* ix, hipStream_t st) {
    DEV_TRY(ix->bias_hist.need((size_t)kBiasHistWords * 4));
    HIP_TRY(hipMemsetAsync(ix->bias_hist, 0, (size_t)kBiasHistWords * 4, st));
    BiasHistArgs a;
    a.bias = ix->active_bias;
    a.w = ix->active_bias_w;
    a.n = ix->n;
    a.row_mask = ix->active_mask;
    a.out = ix->bias_hist;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)ix->cu_count * 4, (ix->n + 255) / 256));
    bias_range_kernel<<<grid, 256, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    bias_hist_kernel<<<grid, 256, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    return TS_OK;
}

// ts_search_biased_rowsets (a weight and a row set per query; kernels_biased_rowsets.h).
// Once per call: the range of the raw bias over all rows, then one histogram per entry of `masks` (NULL = every row) into
// ix->bias_sets_hist: [nhists][kBiasBins] counts, then the two range words.
int biased_rowsets_histograms(ts_index* ix, const uint32_t* const* masks, int nhists, hipStream_t st) {
    if (nhists < 1 || nhists > kRowsetsBlock + 1) return fail(TS_ERR_INTERNAL, "%d histograms of the raw bias", nhists);
    if (!ix->active_bias) return fail(TS_ERR_INTERNAL, "the histograms need the call's bias on the device");
    const size_t words = (size_t)nhists * kBiasBins + 2;
    DEV_TRY(ix->bias_sets_hist.need(words * 4));
    HIP_TRY(hipMemsetAsync(ix->bias_sets_hist, 0, words * 4, st));
    u32* hists = ix->bias_sets_hist;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)ix->cu_count * 4, (ix->n + 255) / 256));
    // bias_range_kernel writes its two words behind kBiasBins counters: handed the LAST histogram, they land behind them all
    BiasHistArgs ra;
    ra.bias = ix->active_bias;
    ra.w = 1.0f;
    ra.n = ix->n;
    ra.row_mask = nullptr;
    ra.out = hists + (size_t)(nhists - 1) * kBiasBins;
    bias_range_kernel<<<grid, 256, 0, st>>>(ra);
    HIP_TRY(hipGetLastError());
    for (int h0 = 0; h0 < nhists; h0 += kBiasedRowsetsHistGroup) {
        BiasHistSetsArgs a;
        memset(&a, 0, sizeof(a));
        a.bias = ix->active_bias;
        a.n = ix->n;
        a.nsets = std::min(kBiasedRowsetsHistGroup, nhists - h0);
        for (int s = 0; s < a.nsets; ++s) a.mask[s] = masks[h0 + s];
        a.range = hists + (size_t)nhists * kBiasBins;
        a.out = hists + (size_t)h0 * kBiasBins;
        TS_TRY((launch_lds<bias_hist_sets_kernel, kBiasedRowsetsHistGroup * kBiasBins * 4>(ix->device, grid, 256, a.nsets * kBiasBins * 4, st, a)));
    }
    return TS_OK;
}

int launch_sample_select_biased_rowsets(const ts_index* ix, int nq, int kk, int nhists, double target, const float* scores, int row_stride,
                                        int64_t ntiles, int64_t tile_stride, int run, hipStream_t st) {
    if (!ix->rowsets_dev || ix->rowsets_dev.bytes() < sizeof(BiasedRowsetsTable) || !ix->active_bias)
        return fail(TS_ERR_INTERNAL, "the biased row-set sample select needs the block's table and the call's bias on the device");
    if (nq > kRowsetsBlock) return fail(TS_ERR_INTERNAL, "a block of the biased row-set pass holds %d queries", kRowsetsBlock);
    if (nhists < 1 || !ix->bias_sets_hist || ix->bias_sets_hist.bytes() < ((size_t)nhists * kBiasBins + 2) * 4)
        return fail(TS_ERR_INTERNAL, "the biased row-set sample select needs the call's %d histograms", nhists);
    BiasRowsetsSelectArgs b;
    memset(&b, 0, sizeof(b));
    b.scores = scores;
    b.row_stride = row_stride;
    b.ntiles = ntiles;
    b.tile_stride = tile_stride;
    b.run = run;
    b.bias = ix->active_bias;
    b.table = ix->rowsets_dev.as<const BiasedRowsetsTable>();
    b.kk = kk;
    b.hists = ix->bias_sets_hist;
    b.range = ix->bias_sets_hist.as<const u32>() + (size_t)nhists * kBiasBins;
    b.target = target;
    b.thr = ix->thr;
    b.count = ix->count;
    if (kk <= 64) return launch_lds<sample_select_biased_rowsets_kernel<1>>(ix->device, nq, kLevelThreads, kBiasSelectLds, st, b);
    return launch_lds<sample_select_biased_rowsets_kernel<4>>(ix->device, nq, kLevelThreads, kBiasSelectLds, st, b);
}

int launch_unbias_rows(const ts_index* ix, const float* scores, const int64_t* idx, const float* bias, const float* weights, int k, float* sims,
                       int64_t count, hipStream_t st) {
    if (count <= 0) return TS_OK;
    unbias_rows_kernel<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(scores, idx, bias, weights, k, ix->row_offset, sims, count);
    HIP_TRY(hipGetLastError());
    return TS_OK;
}

// What one search of `nq` queries for `k` results on this handle is: every decision, made once (mfma_plan) and read by the
// stages below.
struct MfmaPlan {
    std::vector<Level> lv;      // threshold levels, sparsest first; the last one is the full pass
    int kk, variant;
    bool anyd;                  // the general-width kernel (kernels_mfma_anyd.h): full pass only, shared lists only, no screen / pairs / balancing
    bool wide;                  // ... at a width of wide_plan.h: the k-chunked pass and sample (kernels_mfma_wide.h), biased or not
    bool biased;                // ... with the call's bias term in its epilogue, and the biased sample select (any served width)
    bool rowsets;               // ... with a row set per query (ts_search_rowsets): pop, z_tail, tail_p and min_fill come per query from the block's table
    bool shape16, statistical, dense_sample, dense0;
    bool screen_diag, screen, screen_rider, ksplit_form, pair;
    int nq_launch, groups, nb16;
    int grid, wgs, nwriters, priv_cap, pair_lag;
    int stat_cands;
    int64_t pop;
    float z_tail, tail_p;
    double sample_rows;
    bool balance;
};

static MfmaPlan mfma_plan(const ts_index* ix, int nq, int k) {
    MfmaPlan p;
    // threshold rank: the k-th best of a sample is already a valid lower bound of the final k-th best; private
    // lists + spill absorb the run-to-run spread of the candidate count, so no safety margin in the rank
    p.kk = std::max(k, ix->knobs.get(K_MFMA_MIN_RANK, 1));
    p.variant = ix->knobs.get(K_MFMA_VARIANT, 0);
    p.biased = biased_search(ix);
    p.rowsets = rowsets_search(ix);
    p.anyd = general_width(ix);
    p.wide = wide_index(ix) && !p.rowsets;                // (the routing keeps the k-chunked widths off the shared pass)
    p.shape16 = !p.anyd && use_shape16(ix);               // (false for the general-width form, and with it screen, pair and balance)
    p.nq_launch = mfma_block_queries(ix, nq);
    p.groups = p.shape16 ? 0 : p.nq_launch / 128;
    // Threshold of the full pass: by default extrapolated from ONE unthresholded sample (Gaussian tail of the
    // sample's scores, verified afterwards by the candidate count); TS_MFMA_STAT=0 selects the chain of
    // guaranteed lower bounds (more sample rows to scan, no re-runs ever).
    p.statistical = ix->knobs.get(K_MFMA_STAT, 1) != 0;
    p.lv = plan_levels(ix->knobs, ix->n, p.kk, p.statistical);
    const std::vector<Level>& lv = p.lv;
    // TS_MFMA_VARIANT kVariantScreenNoEpilogue .. kVariantScreenTestOnly: the timing-only forms of the int8 screen (diagnostic build only; launch_screen8*.hip)
    p.screen_diag = screen_diag_variant(p.variant);
    // bf16 at d = 768 (or, with TS_MFMA_SCREEN_WIDE, d = 1024) and, with TS_MFMA_SCREEN_F32, fp32 at d = 768 / 1024, behind a
    // threshold: the full pass runs as the int8 screen + exact rescore (kernels_screen8.h), the same candidates >= thr for the
    // final select
    p.screen = mfma_screened(ix) && lv.size() >= 2 && lv.back().stride == 1 && lv.back().run == 1;
    // an fp32 search: the threshold sample carries no rider row for the screen's queries, they get a launch of their own
    p.screen_rider = p.screen && ix->dtype != TS_F32;
    // d = 1024, 193 .. 256 queries: the unscreened pass is a launch of workgroup pairs, in the k-split form unless TS_MFMA_PAIR=1.
    // The screen holds all 256 queries in ONE unpaired launch (four blocks per wave: an int8 query fragment is half the
    // registers); its rescore adds every score in the form the pairs would have (plain chain or two half-chains), bit for bit.
    const bool pair_form = mfma_pairs(ix, nq);
    p.ksplit_form = pair_form && ix->knobs.get(K_MFMA_PAIR, 2) != 1;
    p.pair = pair_form && !p.screen;
    p.pair_lag = p.pair ? std::max(0, ix->knobs.get(K_MFMA_PAIR_LAG, 1)) : 0;
    p.nb16 = p.pair ? 2 : (p.shape16 ? p.nq_launch / 64 : 0);
    // The sparsest level (every score a candidate, at most kLevelSortMax rows) runs as a dense score matrix + one select per
    // query (kernels_sample.h) instead of the full-pass kernel over the sample + a gather from lane-private lists; the
    // latter stays selectable (TS_MFMA_SAMPLE=0) as the A/B partner and serves the thresholded sparse levels of the
    // guaranteed chain (TS_MFMA_STAT=0).
    p.dense_sample = ix->knobs.get(K_MFMA_SAMPLE, 1) != 0;
    // the sparsest level as the dense sample (below): its launch also makes the screen's image of the queries
    p.dense0 = lv.size() >= 2 && p.dense_sample && lv[0].ntiles * kTileRows <= kLevelSortMax;
    p.grid = mfma_grid(ix);
    p.wgs = p.pair ? p.grid / 2 : p.grid;                 // tile ranges of the full pass: one per workgroup, or one per pair
    // lane-private candidate lists: 2 writers x 32 entries per workgroup and query (32x32 shape) or 4 x 16 (16x16 shape)
    p.nwriters = (p.shape16 ? 4 : 2) * p.grid;
    p.priv_cap = p.shape16 ? kMfma16PrivCap : kMfmaPrivCap;
    // Expected candidates per query of the full pass under the estimate.  Every candidate costs the pass ~0.3 us of one
    // CU's time (the appending wave holds the other three at the next barrier), whatever N: 160 per query were 10 % of
    // a 1.25M-row shard's pass and 1 % of the 10M pass; an under-filled query (fewer than k back) costs an exact scan
    // pass.  6 k (at least 64) keeps the under-fill probability negligible for Gaussian-like scores (Poisson mean 64
    // against k = 10, estimate error e^+-0.15) - measured on 10M / 1.25M x 768: 160 / 96 / 64 / 40 expected candidates
    // -> 0 re-runs, 24 -> 5-7 re-runs per 256 queries; full pass 0.459 / 0.447 / 0.438 / 0.424 ms on the shard.
    p.stat_cands = std::min(2048, std::max(2 * p.kk, ix->knobs.get(K_MFMA_STAT_CANDS, std::max(64, 6 * p.kk))));
    // rows the candidates are drawn from: all of them, or the rows a filter allows (the sample sees only those too)
    p.pop = ix->active_mask ? ix->active_allowed : ix->n;
    p.z_tail = (p.statistical && lv.size() == 2)
                   ? (float)normal_tail_z(std::min(0.25, (double)p.stat_cands / (double)std::max<int64_t>(p.pop, 1)))
                   : 0.0f;
    // Second estimate (exponential tail fit of the sample's order statistics, level_threshold in kernels_level.h), for score distributions
    // with heavier tails than a Gaussian.  Only where it is needed: when the guaranteed bound alone (the kk-th best of
    // the sample admits ~kk * N / sample rows) would swamp the candidate buffer - large corpora; it aims at
    // max(2048, 8 kk) expected candidates, a quarter of the buffer.
    p.sample_rows = (double)std::max<int64_t>(1, lv[0].ntiles * kTileRows);
    const bool bound_swamps = (double)p.kk * (double)ix->n / p.sample_rows > 0.5 * kCandCap;
    p.tail_p = (p.z_tail > 0.0f && bound_swamps && ix->knobs.get(K_MFMA_TAIL_FIT, 1))
                   ? (float)std::min(0.25, (double)std::max(2048, 8 * p.kk) / (double)std::max<int64_t>(p.pop, 1))
                   : 0.0f;
    // Feedback partition of the full pass (16x16 kernel): the final select moves the workgroups' tile boundaries towards
    // equal finishing times for the next search (common.h, rebalance_tiles).  The table starts as equal shares and
    // is re-made whenever the grid or the number of tiles changes.
    p.balance = p.shape16 && ix->knobs.get(K_MFMA_BALANCE, 1) != 0 && p.wgs >= 8 && p.wgs <= 256 && lv.back().stride == 1 &&
                lv.back().run == 1 && lv.back().ntiles >= 32 * (int64_t)p.wgs && (p.variant == kVariantProduct || p.variant == kVariantClockProbe || p.screen_diag);
    return p;
}

// The per-handle scratch this plan needs: made on first use, re-made when the grid outgrows it.
static int mfma_scratch(ts_index* ix, const MfmaPlan& p, hipStream_t st) {
    if (p.dense_sample) DEV_TRY(ix->sample.need((size_t)kMfmaQ * kLevelSortMax * 4));
    if (!p.anyd && ix->priv_writers < 4 * p.grid) {            // (the general-width pass writes the shared lists only)
        ix->priv_writers = 0;
        static_assert(4 * kMfma16PrivCap == 2 * kMfmaPrivCap, "both shapes use the same list bytes per workgroup");
        DEV_TRY(remake(ix->priv, (size_t)kMfmaQ * 4 * p.grid * kMfma16PrivCap * 8, ix->pcount, (size_t)kMfmaQ * 4 * p.grid * 4));
        ix->priv_writers = 4 * p.grid;
    }
    const int wgs = p.wgs;
    const int64_t full_tiles = p.lv.back().ntiles;
    if (p.balance && (ix->part_g != wgs || ix->part_ntiles != full_tiles)) {
        if (ix->part_g != wgs) {
            ix->part_g = 0; ix->part_ntiles = -1;
            DEV_TRY(remake(ix->part, (size_t)(wgs + 1) * 8, ix->wg_ticks, (size_t)wgs * 4));
            ix->part_g = wgs;
        }
        std::vector<int64_t> equal((size_t)wgs + 1);
        for (int w = 0; w <= wgs; ++w) equal[w] = full_tiles * (int64_t)w / wgs;
        HIP_TRY(hipMemcpyAsync(ix->part, equal.data(), equal.size() * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(ix->wg_ticks, 0, (size_t)wgs * 4, st));
        HIP_TRY(hipStreamSynchronize(st));          // `equal` is a local; this happens once per (grid, size)
        ix->part_ntiles = full_tiles;
    }
    if (p.pair_lag > 0 && !ix->pair_pos) {
        // one word per workgroup of the pass (index 2 * pair + half < grid): sized for the largest grid the option allows
        DEV_TRY(ix->pair_pos.need(kMfmaMaxGrid * sizeof(unsigned)));
        HIP_TRY(hipMemsetAsync(ix->pair_pos, 0, kMfmaMaxGrid * sizeof(unsigned), st));
    }
#ifdef TS_DIAG
    if (variant_gets_dbg(p.variant)) DEV_TRY(ix->dbg.need(2048 * 4 * 4 * 8));
#endif
    return TS_OK;
}

// Level 0 as the dense threshold sample: the score matrix (with the riders its launch has room for: last search's rebalance,
// the screen's image of the queries) and one select per query.
static int mfma_sample(ts_index* ix, const MfmaPlan& p, int nq, const void* qmat, hipStream_t st) {
    const Level& lv0 = p.lv[0];
    SampleArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.corpus = ix->rows;
    sa.n = ix->n;
    sa.ld = (int)ix->ld;
    sa.ntiles = lv0.ntiles;
    sa.tile_stride = lv0.stride;
    sa.run = lv0.run;
    sa.q = qmat;
    sa.nq = nq;
    sa.row_mask = ix->active_mask;
    sa.scores = ix->sample;
    sa.row_stride = (int)((lv0.ntiles * kTileRows + 63) / 64 * 64);
    sa.fb_count = ix->fb_count;
    // 32 rows per workgroup and one 64-query chunk: 512 workgroups of 50 KB LDS at 4,096 rows x 256 queries, two to
    // a CU (64-row workgroups serving two chunks each measured the same: 15.2 / 25.0 us against 14.9 / 24.3 us at
    // 4,096 / 8,192 rows - the launch is latency, not work)
    const bool f32 = ix->dtype == TS_F32;
    const int nchunks = (nq + 63) / 64;
    const int wg_rows = 32;
    // the previous search's full pass left its workgroups' times: one extra workgroup of this launch moves the
    // tile boundaries before this search's pass reads them
    if (ix->rebalance_pending && p.balance && ix->rebalance_grid == p.wgs && ix->rebalance_grid <= 256) {
        sa.part = ix->part;
        sa.wg_ticks = ix->wg_ticks;
        sa.part_g = ix->rebalance_grid;
        const int b = ix->knobs.get(K_MFMA_BALANCE, 1);      // TS_MFMA_BALANCE = n > 1: gain n / 10 (default 0.7)
        sa.part_gain = (b >= 2 && b <= 10) ? 0.1f * (float)b : 0.7f;
    }
    ix->rebalance_pending = false;
    if (p.screen_rider) {
        sa.scr_qimg = ix->scr_q.as<signed char>();
        sa.scr_qmeta = ix->scr_qmeta.as<float4>();
        sa.scr_count = ix->scr_count;
        sa.scr_nrows = std::min(p.nq_launch, kMfmaQ);
    }
    const dim3 sgrid((unsigned)(sa.row_stride / wg_rows), (unsigned)(nchunks + ((sa.part || sa.scr_qimg) ? 1 : 0)));
    const int slds = sample_lds_bytes(wg_rows, (int)(ix->ld * ix->elem()));
    constexpr int kSampleLdsMax = 144 * 1024;   // dynamic part; the kernel also has a few hundred static bytes (rebalance_tiles)
    static_assert(kSampleLdsMax == kWideSampleLdsLimit, "wide_plan.h restates the sample's limit");
    if (p.rowsets) TS_TRY(launch_sample_rowsets(ix, sgrid, slds, st, sa));          // liveness per (sample position, query): no riders
    else if (p.wide) TS_TRY(launch_sample_wide(ix, sgrid, st, sa));       // rows staged k-chunk by k-chunk: its LDS does not follow the width
    else if (slds > kSampleLdsMax) return fail(TS_ERR_INTERNAL, "threshold sample: rows of %lld bytes do not fit the LDS", (long long)(ix->ld * ix->elem()));
    else if (f32) TS_TRY((launch_lds<sample_scores_kernel<true, 2>, kSampleLdsMax>(ix->device, sgrid, 256, slds, st, sa)));
    else TS_TRY((launch_lds<sample_scores_kernel<false, 2>, kSampleLdsMax>(ix->device, sgrid, 256, slds, st, sa)));
    LevelArgs l;
    memset(&l, 0, sizeof(l));
    l.count = ix->count;
    l.kk = p.kk;
    l.thr = ix->thr;
    l.z_tail = p.z_tail;
    l.tail_p = p.tail_p;
    l.tail_z = (float)normal_tail_z(std::min(0.25, 32.0 / p.sample_rows));
    l.nq = nq;
    // where the select cuts first: ~2 kl of the sample's live rows above it on Gaussian-like scores
    const int kl = p.tail_p > 0.0f ? std::max(p.kk, 32) : p.kk;
    const double live = p.sample_rows * (double)p.pop / (double)std::max<int64_t>(ix->n, 1);
    const float z_sel = (float)normal_tail_z(std::min(0.25, 2.0 * kl / std::max(live, 1.0)));
    if (p.biased && p.rowsets)           // ... with the query's own weight and its set's histogram of the raw bias
        return launch_sample_select_biased_rowsets(ix, nq, p.kk, ix->active_rowsets->nhists, (double)p.stat_cands, ix->sample, sa.row_stride,
                                                   lv0.ntiles, lv0.stride, lv0.run, st);
    if (p.biased) {
        // the weighted scores are not Gaussian: the select models the similarities and the known term apart (bias_plan.h)
        BiasSelectArgs b;
        memset(&b, 0, sizeof(b));
        b.scores = ix->sample;
        b.row_stride = sa.row_stride;
        b.ntiles = lv0.ntiles;
        b.tile_stride = lv0.stride;
        b.run = lv0.run;
        b.bias = ix->active_bias;
        b.w = ix->active_bias_w;
        b.kk = p.kk;
        b.ghist = ix->bias_hist;
        b.target = (double)p.stat_cands;
        b.thr = ix->thr;
        b.count = ix->count;
        if (p.kk <= 64) return launch_lds<sample_select_biased_kernel<1>>(ix->device, nq, kLevelThreads, kBiasSelectLds, st, b);
        return launch_lds<sample_select_biased_kernel<4>>(ix->device, nq, kLevelThreads, kBiasSelectLds, st, b);
    }
    if (p.rowsets) return launch_sample_select_rowsets(ix, nq, st, l, ix->sample, sa.row_stride);     // z_tail, tail_p, z_sel: the table's
    sample_select_fast_kernel<kSelThreads><<<nq, kSelThreads, 0, st>>>(l, ix->sample, sa.row_stride, z_sel);
    HIP_TRY(hipGetLastError());
    return TS_OK;
}

#ifdef TS_DIAG
// What a timing variant's full pass left in MfmaArgs::dbg, read back and printed (or kept in the handle: the clock probe).
static int mfma_diag_readout(ts_index* ix, const MfmaPlan& p, const unsigned long long* dbg, hipStream_t st) {
    const int grid = p.grid, variant = p.variant;
    if (p.shape16 && (variant == kVariantClockProbe || (p.screen && variant == kVariantScreenClockProbe))) {
        // clock probe (MI355X_MICROARCH.md "DVFS give-back" item 6): shader cycles / 100 MHz ticks around the tile loop,
        // median over workgroups
        std::vector<unsigned long long> h((size_t)grid * 4);
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost));
        std::vector<double> ghz, cpu_;
        for (int w = 0; w < grid; ++w)
            if (h[w * 4 + 1] > 0 && h[w * 4 + 2] > 0) {
                ghz.push_back((double)h[w * 4] / (double)h[w * 4 + 1] * 0.1);
                cpu_.push_back((double)h[w * 4] / (double)h[w * 4 + 2]);
            }
        if (!ghz.empty()) {
            std::sort(ghz.begin(), ghz.end());
            std::sort(cpu_.begin(), cpu_.end());
            ix->probe_ghz = ghz[ghz.size() / 2];
            ix->probe_cycles_per_unit = cpu_[cpu_.size() / 2];
            ix->probe_units = (double)h[2];
            if (ix->knobs.get(K_PROBE_SPREAD, 0)) {
                // the launch ends with its slowest workgroup: time inside the tile loop per workgroup (100 MHz ticks),
                // and its mean by workgroup id % 8 (the XCD under round-robin dispatch)
                std::vector<double> us;
                double xm[8] = {0}, xn[8] = {0};
                for (int w = 0; w < grid; ++w)
                    if (h[w * 4 + 1] > 0) {
                        us.push_back((double)h[w * 4 + 1] * 0.01);
                        xm[w & 7] += us.back();
                        xn[w & 7] += 1;
                    }
                std::sort(us.begin(), us.end());
                fprintf(stderr, "[tsearch probe] tile loop per workgroup: min %.1f us, median %.1f, max %.1f; mean by id %% 8:", us.front(),
                        us[us.size() / 2], us.back());
                for (int x = 0; x < 8; ++x) fprintf(stderr, " %.1f", xm[x] / std::max(1.0, xn[x]));
                fprintf(stderr, "\n");
            }
        }
    } else if (p.shape16 && (variant == kVariantStamps || (p.screen && variant == kVariantScreenStamps))) {
        std::vector<unsigned long long> h((size_t)grid * 16);
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost));
        const double units = (double)(p.lv.back().ntiles * (variant == kVariantScreenStamps ? (ix->d == 1024 ? Mfma16Dims<512>::kUnits : Mfma16Dims<384>::kUnits) : MfmaDims<768>::kUnits)) / grid;
        for (int wv = 0; wv < 4; ++wv) {
            double tot = 0, vm = 0, bar = 0, dma = 0;
            for (int w = wv; w < grid * 4; w += 4) { tot += h[w * 4]; vm += h[w * 4 + 1]; bar += h[w * 4 + 2]; dma += h[w * 4 + 3]; }
            if (variant == kVariantScreenStamps)
                fprintf(stderr, "[tsearch stamps8] wave %d per tile: total %.0f cycles, vmcnt wait %.0f, barrier wait %.0f, tile tail %.0f (drain to end of epilogue; stamp cost ~40 each included)\n",
                        wv, tot / grid / units, vm / grid / units, bar / grid / units, dma / grid / units);
            else
                fprintf(stderr, "[tsearch stamps16] wave %d per unit: total %.0f cycles, vmcnt wait %.0f, barrier wait %.0f, DMA issue %.0f (6 pieces; stamp cost ~40 each included)\n",
                        wv, tot / grid / units, vm / grid / units, bar / grid / units, dma / grid / units);
        }
    } else if (!p.shape16) {
        std::vector<unsigned long long> h((size_t)grid * 16);
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost));
        for (int wv = 0; wv < 4; ++wv) {  // by wave of the workgroup: with small batches the waves differ
            double tot = 0, vm = 0, bar = 0, units = 0;
            for (int w = wv; w < grid * 4; w += 4) { tot += h[w * 4]; vm += h[w * 4 + 1]; bar += h[w * 4 + 2]; units += h[w * 4 + 3]; }
            fprintf(stderr, "[tsearch stamps] wave %d per unit: total %.0f cycles, vmcnt wait %.0f, barrier wait %.0f (units/wave %.0f)\n",
                    wv, tot / units, vm / units, bar / units, units / grid);
        }
    }
    return TS_OK;
}
#endif

// Level `i` on a matrix kernel (the full pass, or a sparse level of the guaranteed chain / of TS_MFMA_SAMPLE=0) and its select.
static int mfma_level(ts_index* ix, const MfmaPlan& p, size_t i, int nq, int k, float* out_scores, int64_t* out_idx, const void* qmat,
                      hipStream_t st) {
    const Level& lv = p.lv[i];
    const bool full_pass = (i + 1 == p.lv.size());
    MfmaArgs a;
    a.corpus = ix->rows.as<const unsigned short>();
    a.n = ix->n;
    a.ntiles = lv.ntiles;
    a.tile_stride = lv.stride;
    a.run = lv.run;
    a.q = (const unsigned short*)qmat;
    a.thr = ix->thr;
    a.nq = ix->knobs.get(K_MFMA_NO_IDLE, 0) ? 256 : nq;
    a.row_mask = ix->active_mask;
    a.ahead = ix->knobs.get(K_MFMA_AHEAD, 0);
    a.priv = ix->priv;
    a.pcount = ix->pcount;
    a.cand = ix->cand;
    a.count = ix->count;
    a.cap = kCandCap;
    a.first_level = (i == 0) ? 1 : 0;      // thresholds and per-search counters are initialised inside the first launch of a search
    a.nq_real = nq;
    a.fb_count = ix->fb_count;
    a.part = (p.balance && full_pass) ? ix->part : nullptr;
    a.wg_ticks = (p.balance && full_pass) ? ix->wg_ticks : nullptr;
    a.pair = (p.pair && full_pass) ? (p.ksplit_form ? 2 : 1) : 0;      // 2: the k-split form (TS_MFMA_PAIR=1: two blocks per wave over the whole row)
    const bool paced = a.pair && p.pair_lag > 0;
    a.pair_pos = paced ? ix->pair_pos : nullptr;
    a.pair_lag = paced ? p.pair_lag : 0;
    a.dbg = nullptr;
    a.scr_tile = nullptr;
    a.scr_q = nullptr;
#ifdef TS_DIAG
    if (variant_gets_dbg(p.variant) && !p.anyd) a.dbg = ix->dbg;
#endif
    if (p.anyd && !full_pass) return fail(TS_ERR_INTERNAL, "the general-width matrix kernel has no sparse level");
    hipEvent_t stop = full_pass ? prof_begin(ix, st, ix->n) : nullptr;  // only the full pass is bracketed
    int rc;
    if (p.rowsets && p.biased) rc = launch_pass_mfma_anyd_biased_rowsets(ix, p.grid, st, a);
    else if (p.rowsets) rc = launch_pass_mfma_anyd_rowsets(ix, p.grid, st, a);
    else if (p.wide) rc = p.biased ? launch_pass_mfma_wide_biased(ix, p.grid, st, a) : launch_pass_mfma_wide(ix, p.grid, st, a);
    else if (p.biased) rc = launch_pass_mfma_anyd_biased(ix, p.grid, st, a);
    else if (p.anyd) rc = launch_pass_mfma_anyd(ix, p.grid, st, a);
    else if (p.screen && full_pass) rc = screen_full_pass(ix, p.nb16, nq, p.grid, p.screen_diag ? p.variant : kVariantProduct, p.ksplit_form, st, a);
    else if (ix->dtype == TS_F32 && p.shape16) rc = launch_pass_mfma16_f32(ix->device, ix->d, p.nb16, full_pass, p.grid, st, a);
    else if (ix->dtype == TS_F32) rc = launch_pass_mfma32_f32(ix->device, full_pass, p.variant, p.grid, st, a);
    else if (p.shape16) rc = launch_pass_mfma16(ix->device, ix->d, p.nb16, full_pass, p.variant, p.grid, st, a);
    else rc = launch_pass_mfma32(ix->device, ix->d, p.groups, full_pass, p.variant, p.grid, st, a);
    prof_end(stop, st);
    TS_TRY(rc);
#ifdef TS_DIAG
    if (a.dbg && full_pass) TS_TRY(mfma_diag_readout(ix, p, a.dbg, st));
#endif
    LevelArgs l;
    memset(&l, 0, sizeof(l));
    l.priv = ix->priv;
    l.pcount = ix->pcount;
    // the 16x16 full pass stages its candidates in LDS, the general-width one appends them directly: shared lists only
    l.nwriters = ((p.shape16 || p.anyd) && full_pass) ? 0 : p.nwriters;
    l.priv_cap = p.priv_cap;
    l.cand = ix->cand;
    l.count = ix->count;
    l.cap = kCandCap;
    l.kk = p.kk;
    l.thr = ix->thr;
    l.final_level = full_pass;
    l.z_tail = full_pass ? 0.0f : p.z_tail;
    l.tail_p = full_pass ? 0.0f : p.tail_p;
    l.tail_z = (float)normal_tail_z(std::min(0.25, 32.0 / p.sample_rows));
    // fewer candidates back than there are answers = the threshold was too high (an estimate that overshot, or a sample
    // score that differs from the pass's in the last bit): exact re-run
    l.min_fill = (int)std::min<int64_t>(k, p.pop);
    l.out_scores = out_scores;
    l.out_idx = out_idx;
    l.k_user = k;
    l.row_offset = ix->row_offset;
    l.id_map = ix->id_map;
    l.fb_list = ix->fb_list;
    l.fb_count = ix->fb_count;
    l.stat_q = ix->stat;
    l.nq = nq;
    if (p.rowsets) return launch_level_select_rowsets(ix, nq, st, l);      // min_fill: the table's, per query
    if (p.kk <= 64) return launch_lds<level_select_kernel<1>>(ix->device, nq, kLevelThreads, kLevelLds, st, l);
    return launch_lds<level_select_kernel<4>>(ix->device, nq, kLevelThreads, kLevelLds, st, l);
}

// ts_search_rowsets: the block's table (rowsets_plan.h: RowsetsTable) from the call's sets and this plan, made on the host and
// uploaded before the block's first launch.  The host copy is the handle's: the previous block's upload has run (every block
// ends by waiting for its re-run list).
// (one layout for both entries: the table of ts_search_biased_rowsets begins with ts_search_rowsets' and adds the weights)
constexpr size_t kRowsetsTableBytes = sizeof(BiasedRowsetsTable);
static_assert(offsetof(BiasedRowsetsTable, r) == 0, "the row-set kernels read the biased table's first member");
static int rowsets_table(ts_index* ix, const MfmaPlan& p, int nq, int k, hipStream_t st) {
    const RowsetsCall& call = *ix->active_rowsets;
    constexpr size_t kBytes = kRowsetsTableBytes + 2 * kRowsetsBlock * sizeof(int);
    DEV_TRY(ix->rowsets_dev.need(kBytes));
    ix->rowsets_host.resize(kBytes);
    BiasedRowsetsTable* bt = reinterpret_cast<BiasedRowsetsTable*>(ix->rowsets_host.data());
    RowsetsTable* t = &bt->r;
    const bool estimate = p.statistical && p.lv.size() == 2;
    const bool tail_fit = ix->knobs.get(K_MFMA_TAIL_FIT, 1) != 0;
    for (int s = 0; s < kRowsetsBlock; ++s) t->mask[s] = nullptr;
    for (int q = 0; q < kRowsetsBlock; ++q) {
        const int32_t s = q < nq ? call.which[q] : -1;
        const int64_t pop = s < 0 ? ix->n : call.sets[s]->allowed;
        if (s >= 0) t->mask[s] = call.sets[s]->mask;
        const RowsetsNumbers num = rowsets_numbers(pop, ix->n, k, p.kk, p.stat_cands, p.sample_rows, kCandCap, estimate, tail_fit);
        t->z_tail[q] = num.z_tail;
        t->tail_p[q] = num.tail_p;
        t->min_fill[q] = num.min_fill;
        t->z_sel[q] = rowsets_z_sel(pop, ix->n, p.kk, num.tail_p, p.sample_rows);
        t->set[q] = s;
        bt->weight[q] = (call.weights && q < nq) ? call.weights[q] : 0.0f;
        bt->hist[q] = (call.hist_of && q < nq) ? call.hist_of[q] : 0;
    }
    HIP_TRY(hipMemcpyAsync(ix->rowsets_dev, bt, kRowsetsTableBytes, hipMemcpyHostToDevice, st));
    return TS_OK;
}

// ... and its exact re-run: the final select's list is read back, grouped by set on the host, and each group runs through the scan
// behind its own set (one launch per set that has a query to re-run; none in the usual case).  Waits for the stream.
static int rowsets_rerun(ts_index* ix, int nq, int k, float* out_scores, int64_t* out_idx, hipStream_t st, const void* qmat, bool in_place) {
    RowsetsCall& call = *ix->active_rowsets;
    int fb = 0;
    std::vector<int> list((size_t)kRowsetsBlock);
    std::vector<u32> cands((size_t)nq);
    HIP_TRY(hipMemcpyAsync(&fb, ix->fb_count, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(list.data(), ix->fb_list, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cands.data(), ix->stat, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (u32 c : cands) call.candidates += c;
    if (fb < 0 || fb > nq) return fail(TS_ERR_INTERNAL, "the re-run list of a row-set pass holds %d of %d queries", fb, nq);
    call.fallback_queries += fb;
    if (fb == 0) return TS_OK;
    for (int i = 0; i < fb; ++i)
        if (list[i] < 0 || list[i] >= nq) return fail(TS_ERR_INTERNAL, "the re-run list of a row-set pass names query %d of %d", list[i], nq);
    // (under a weight per query: by class, set then weight - the scan's weight is one per launch)
    auto weight_of = [&](int q) { return call.weights ? call.weights[q] : 0.0f; };
    auto same_class = [&](int x, int y) { return biased_rowsets_same_class(call.which[x], weight_of(x), call.which[y], weight_of(y)); };
    std::stable_sort(list.begin(), list.begin() + fb, [&](int x, int y) {
        return call.which[x] != call.which[y] ? call.which[x] < call.which[y] : weight_of(x) < weight_of(y);
    });
    // lists [256] | counts [256] behind the table, both in the handle's host copy
    int* hl = reinterpret_cast<int*>(ix->rowsets_host.data() + kRowsetsTableBytes);
    int* hc = hl + kRowsetsBlock;
    int* dl = reinterpret_cast<int*>(ix->rowsets_dev.as<unsigned char>() + kRowsetsTableBytes);
    int* dc = dl + kRowsetsBlock;
    int ngroups = 0;
    for (int i = 0; i < fb; ++i) {
        hl[i] = list[i];
        if (i == 0 || !same_class(list[i], list[i - 1])) hc[ngroups++] = 0;
        ++hc[ngroups - 1];
    }
    HIP_TRY(hipMemcpyAsync(dl, hl, (size_t)fb * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dc, hc, (size_t)ngroups * 4, hipMemcpyHostToDevice, st));
    int rc = TS_OK;
    for (int g = 0, at = 0; g < ngroups && rc == TS_OK; at += hc[g], ++g) {
        const int32_t s = call.which[hl[at]];
        ix->active_mask = s < 0 ? nullptr : (const u32*)call.sets[s]->mask;
        if (call.weights) ix->active_bias_w = call.weights[hl[at]];
        if (!in_place) rc = scan_search(ix, nq, k, out_scores, out_idx, dl + at, dc + g, st);
        else if (ix->dtype == TS_F32) rc = scan_search(ix, nq, k, out_scores, out_idx, dl + at, dc + g, st, (const float*)qmat);
        else rc = scan_search(ix, nq, k, out_scores, out_idx, dl + at, dc + g, st, nullptr, (const unsigned short*)qmat);
    }
    ix->active_mask = nullptr;
    TS_TRY(rc);
    HIP_TRY(hipStreamSynchronize(st));       // the lists are the handle's: the next block writes them
    return TS_OK;
}

// `qmat`: the queries as the kernels multiply them (storage dtype, row stride d = ld, a whole launch's worth of rows):
// the prepared copy, or the caller's own device matrix when it already has that form (`in_place`).
int mfma_search(ts_index* ix, int nq, int k, float* out_scores, int64_t* out_idx, hipStream_t st, ts_search_stats* stats,
                       const void* qmat, bool in_place) {
    const MfmaPlan p = mfma_plan(ix, nq, k);
    TS_TRY(mfma_scratch(ix, p, st));
    if (p.rowsets) TS_TRY(rowsets_table(ix, p, nq, k, st));
    if (p.screen) TS_TRY(screen_prepare(ix, qmat, p.nq_launch, !(p.dense0 && p.screen_rider), st));
    for (size_t i = 0; i < p.lv.size(); ++i) {
        if (i == 0 && p.dense0) TS_TRY(mfma_sample(ix, p, nq, qmat, st));
        else TS_TRY(mfma_level(ix, p, i, nq, k, out_scores, out_idx, qmat, st));
    }
    // the pass just finished left its workgroups' times: the next search's sample launch moves the tile boundaries (without
    // a dense sample: block 0 of the re-run launch below)
    ix->rebalance_pending = p.balance;
    ix->rebalance_grid = p.wgs;
    ix->rebalance_in_rerun = !(p.dense_sample && p.lv.size() == 2);
    if (stats) {
        stats->levels = (int)p.lv.size();
        stats->screened = p.screen ? 1 : 0;
    }
    if (p.rowsets) return rowsets_rerun(ix, nq, k, out_scores, out_idx, st, qmat, in_place);
    // exact fall-back for queries that lost candidates (device-side count; one empty launch when 0)
    if (!in_place) TS_TRY(scan_search(ix, nq, k, out_scores, out_idx, ix->fb_list, ix->fb_count, st));
    else if (ix->dtype == TS_F32) TS_TRY(scan_search(ix, nq, k, out_scores, out_idx, ix->fb_list, ix->fb_count, st, (const float*)qmat));
    else TS_TRY(scan_search(ix, nq, k, out_scores, out_idx, ix->fb_list, ix->fb_count, st, nullptr, (const unsigned short*)qmat));
    return TS_OK;
}
