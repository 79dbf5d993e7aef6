// The kernels of ts_search_biased_rowsets beside the full pass (mfma_anyd_biased_rowsets_kernel, kernels_mfma_anyd.h): the
// citation-weighted search with a weight and a row set per query.  The threshold sample (sample_scores_rowsets_kernel: raw
// scores, -inf where the query's set filters the row out) and the final select (level_select_rowsets_kernel) are the row-set
// search's own; what is new:
//   * bias_hist_sets_kernel, once per call: the histogram of the RAW bias (finite values only) over the rows of each distinct
//     set the pass's queries name - not of w * bias, which would be one histogram per query.  One range (lo, hi) over all rows
//     (bias_range_kernel with w = 1 and no mask).  A workgroup keeps the histograms of up to kBiasedRowsetsHistGroup sets in its
//     LDS, so `bias` is read once per group of sets and each mask once (biased_rowsets_plan.h: biased_rowsets_hist_bytes);
//   * sample_select_biased_rowsets_kernel, one workgroup per query: sample_select_biased_kernel's rule with the query's own
//     weight - the kk-th best weighted sample score as the guaranteed bound, the estimate of biased_rowsets_solve_threshold from
//     the query's mu / sigma, its set's histogram and its weight; thr[q] = max(bound, estimate), count[q] = 0;
//   * unbias_rows_kernel: unbias_kernel with the weight of row i / k.
#pragma once
#include "biased_rowsets_plan.h"
#include "kernels_level.h"
#include "kernels_sample_biased.h"

namespace ts {

struct BiasHistSetsArgs {
    const float* bias;                               // [n]
    int64_t n;
    const u32* mask[kBiasedRowsetsHistGroup];        // this launch's sets: NULL = every row
    int nsets;                                       // 1 .. kBiasedRowsetsHistGroup
    const u32* range;                                // [2]: ~ord_f32(lo), ord_f32(hi) of all rows (bias_range_kernel); both 0: no finite value
    u32* out;                                        // [nsets][kBiasBins], zeroed
};

// dynamic LDS: nsets * kBiasBins counters
__global__ void __launch_bounds__(256) bias_hist_sets_kernel(BiasHistSetsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char hist_smem[];
    u32* h = (u32*)hist_smem;
    if (a.range[1] == 0u) return;                    // no row with a finite bias (uniform)
    const float lo = unord_f32(~a.range[0]), hi = unord_f32(a.range[1]);
    const float width = hi > lo ? (hi - lo) / (float)kBiasBins : 0.0f;
    const int bins = a.nsets * kBiasBins;
    for (int i = threadIdx.x; i < bins; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += (int64_t)gridDim.x * blockDim.x) {
        const float v = a.bias[r];
        if (!(fabsf(v) < INFINITY)) continue;
        const int b = bias_bin(v, lo, width);
        for (int s = 0; s < a.nsets; ++s) {          // uniform trip count; mask[s] is a kernel argument
            const u32* m = a.mask[s];
            if (!m || ((m[r >> 5] >> (r & 31)) & 1u)) atomicAdd(&h[s * kBiasBins + b], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += blockDim.x)
        if (h[i]) atomicAdd(&a.out[i], h[i]);
}

struct BiasRowsetsSelectArgs {
    const float* scores;      // [nq][row_stride] raw sample scores (-inf: no such row / filtered out for this query)
    int row_stride;
    int64_t ntiles;           // sample tiles; position p = 32 * tile + row (positions >= 32 * ntiles hold -inf)
    int64_t tile_stride;      // sample tile j is global tile (j / run) * run * tile_stride + j % run
    int run;
    const float* bias;        // [n]
    const BiasedRowsetsTable* table;
    int kk;                   // threshold rank
    const u32* hists;         // [histograms][kBiasBins] raw-bias counts per set (bias_hist_sets_kernel)
    const u32* range;         // [2] as BiasHistSetsArgs::range
    double target;            // expected candidates per query the estimate aims at
    float* thr;               // [256]
    u32* count;               // [256]
};

template <int KR>   // 1: kk <= 64, 4: kk <= 256 (as level_select_kernel)
__global__ void __launch_bounds__(kLevelThreads) sample_select_biased_rowsets_kernel(BiasRowsetsSelectArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NW = kLevelThreads / 64;
    const SelectLds lds = SelectLds::carve(smem, kLevelSortMax);   // keys: weighted sample scores keyed by position
    u32* bhist = (u32*)(smem + kLevelLds);                    // the query's set's histogram of the raw bias
    double* red = (double*)(bhist + kBiasBins);               // [2][NW] sums of the bisection
    double* stat = red + 2 * NW;                              // [NW][4]: sum, sum of squares, live rows, -
    const int q = blockIdx.x;                                 // < kRowsetsBlock (the launcher checks)
    const float w = a.table->weight[q];
    const u32* ghist = a.hists + (int64_t)a.table->hist[q] * kBiasBins;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int npos = (int)min(a.ntiles * (int64_t)kTileRows, (int64_t)kLevelSortMax);
    if (threadIdx.x == 0) {
        a.count[q] = 0;
        lds.ctr[kSelFill] = 0;                                // keys made
        lds.ctr[kSelShort] = 0;
    }
    for (int i = threadIdx.x; i < kLevelBins; i += blockDim.x) lds.hist[i] = 0;
    for (int i = threadIdx.x; i < kBiasBins; i += blockDim.x) bhist[i] = ghist[i];
    __syncthreads();
    auto row_of = [&](int p) -> int64_t {
        const int64_t j = min((int64_t)(p >> 5), a.ntiles - 1);
        const int64_t gt = (a.run == 1) ? j * a.tile_stride : (j / a.run) * a.run * a.tile_stride + j % a.run;
        return gt * kTileRows + (p & 31);
    };
    const float* src = a.scores + (int64_t)q * a.row_stride;

    // statistics of the raw scores, the weighted keys
    double s1 = 0.0, s2 = 0.0;
    u32 nl = 0;
    for (int i0 = wave * 64; i0 < npos; i0 += NW * 64) {
        const int i = i0 + lane;
        const float raw = i < npos ? src[i] : -INFINITY;
        const bool live = raw == raw && raw > -INFINITY;      // a live position's row is a real row (< n) of the query's set
        u64 key = 0ull;
        if (live) {
            const float ws = fmaf(w, a.bias[row_of(i)], raw);
            s1 += (double)raw;
            s2 += (double)raw * (double)raw;
            ++nl;
            if (ws == ws) key = make_key(ws, (u32)i);
        }
        const u64 made = __ballot(key != 0ull);
        u32 base = 0;
        if (lane == 0 && made) base = atomicAdd(&lds.ctr[kSelFill], (u32)__popcll(made));
        base = (u32)__shfl((int)base, 0, 64);
        if (key != 0ull) lds.keys[base + __popcll(made & ((1ull << lane) - 1ull))] = key;
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    const double dn = wave_sum_f64((double)nl);
    if (lane == 0) {
        stat[4 * wave] = s1;
        stat[4 * wave + 1] = s2;
        stat[4 * wave + 2] = dn;
    }
    __syncthreads();
    double t1 = 0.0, t2 = 0.0, live_rows = 0.0;
#pragma unroll
    for (int v = 0; v < NW; ++v) {
        t1 += stat[4 * v];
        t2 += stat[4 * v + 1];
        live_rows += stat[4 * v + 2];
    }
    const double mu = live_rows > 0.0 ? t1 / live_rows : 0.0;
    const double sigma = live_rows > 0.0 ? sqrt(fmax(t2 / live_rows - mu * mu, 0.0)) : 0.0;
    // the call's range (no row with a finite bias: hi < lo, and the solver has nothing to estimate from)
    const bool any_term = a.range[1] != 0u;
    const float lo = any_term ? unord_f32(~a.range[0]) : INFINITY, hi = any_term ? unord_f32(a.range[1]) : -INFINITY;
    const float width = hi > lo ? (hi - lo) / (float)kBiasBins : 0.0f;
    const int cnt = (int)lds.ctr[kSelFill];

    // the guaranteed bound: the kk-th best weighted score of the query's sample
    double m_unused, sd_unused;
    const u64* best = lds_select_top<KR>(lds, cnt, a.kk, false, m_unused, sd_unused);
    const u64 kth = best[a.kk - 1];
    const float bound = kth ? key_score(kth) : -INFINITY;

    // the estimate (as level_threshold: from 256 live rows on)
    float est = -INFINITY;
    if (live_rows >= 256.0) {
        int flip = 0;
        auto total = [&](double x) -> double {
            x = wave_sum_f64(x);
            if (lane == 0) red[flip * NW + wave] = x;
            __syncthreads();
            double t = 0.0;
#pragma unroll
            for (int v = 0; v < NW; ++v) t += red[flip * NW + v];
            flip ^= 1;
            return t;
        };
        est = biased_rowsets_solve_threshold(bhist, lo, width, hi, w, mu, sigma, a.target, (int)threadIdx.x, (int)blockDim.x, total);
    }
    if (threadIdx.x == 0) a.thr[q] = fmaxf(bound, est);
}

// ts_search_biased_rowsets' out_sims: entry i belongs to query i / k, whose weight is weights[i / k]
__global__ void unbias_rows_kernel(const float* scores, const int64_t* idx, const float* bias, const float* weights, int k, int64_t row_offset,
                                   float* sims, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int64_t id = idx[i];
    sims[i] = id < 0 ? -INFINITY : fmaf(-weights[i / k], bias[id - row_offset], scores[i]);
}

}  // namespace ts
