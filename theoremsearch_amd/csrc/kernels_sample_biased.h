// The threshold of the biased matrix search (ts_search_biased_ex), in two parts.
//
// Once per call, bias_range_kernel + bias_hist_kernel: the histogram of the finite w * bias[row] over EVERY row the call may
// return (all rows, or the rows its mask allows) - exact counts, kBiasBins bins between the smallest and the largest term.  Two
// passes over the bias array and the mask: n * 4 bytes each against n * d * 2 of the full pass.  The histogram of the threshold
// sample's rows would cost nothing, and is not enough: each sampled row then stands for pop / live corpus rows with exactly its
// term, and where a few rows of a heavy tail decide the top k (power-law citation counts) the threshold follows the two or
// three tail rows the sample happens to hold (measured, 256 queries on 1M x 768, k = 10: 32 queries under-filled and re-run
// with the sample's histogram; tests/test_bias_plan_cpu.py pins it on a CPU model).
//
// Per query, sample_select_biased_kernel: one workgroup turns that query's row of the dense sample score matrix
// (kernels_sample.h: RAW similarities, -inf = no such row / filtered out) into the pass threshold of the biased full pass
// (kernels_mfma_anyd.h, BIAS):
//   * a sample position is mapped to its corpus row as sample_scores_kernel maps it;
//   * mu / sigma of the live raw scores;
//   * the kk-th best WEIGHTED sample score (fmaf(w, bias[row], raw), the pass's own arithmetic) by lds_select_top: a lower
//     bound of the final kk-th best - the guaranteed threshold;
//   * the estimate of bias_plan.h (bias_solve_threshold: Gaussian similarities + the known additive term, bisected for the
//     target number of candidates; scale 1, the counts are the corpus's own), every thread taking two of the 1,024 bins;
//   * thr[q] = max(bound, estimate); count[q] = 0 (the shared list of the full pass starts empty).
// The estimate is not a bound: the final select re-runs a query exactly when fewer than min(k, rows) candidates came back.
#pragma once
#include "bias_plan.h"
#include "kernels_level.h"

namespace ts {

// out: kBiasBins counts, then ~ord_f32(smallest finite term) and ord_f32(largest) - both 0 (the memset) while no row has one
constexpr int kBiasHistWords = kBiasBins + 2;
struct BiasHistArgs {
    const float* bias;        // [n]
    float w;
    int64_t n;
    const u32* row_mask;      // optional: only rows whose bit is set count
    u32* out;                 // [kBiasHistWords], zeroed before bias_range_kernel
};

// the finite term of row r, or NaN where the row does not count (masked out, or its term is infinite / NaN)
__device__ __forceinline__ float bias_term_of(const BiasHistArgs& a, int64_t r) {
    if (a.row_mask && !((a.row_mask[r >> 5] >> (r & 31)) & 1u)) return NAN;
    const float term = a.w * a.bias[r];
    return fabsf(term) < INFINITY ? term : NAN;
}

__global__ void __launch_bounds__(256) bias_range_kernel(BiasHistArgs a) {
    u32 lo_inv = 0u, hi = 0u;         // ord_f32 of a finite float is never 0 or ~0
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += (int64_t)gridDim.x * blockDim.x) {
        const float term = bias_term_of(a, r);
        if (term == term) {
            const u32 o = ord_f32(term);
            lo_inv = max(lo_inv, ~o);
            hi = max(hi, o);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo_inv = max(lo_inv, (u32)__shfl_xor((int)lo_inv, off, 64));
        hi = max(hi, (u32)__shfl_xor((int)hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0 && hi) {
        atomicMax(&a.out[kBiasBins], lo_inv);
        atomicMax(&a.out[kBiasBins + 1], hi);
    }
}

__global__ void __launch_bounds__(256) bias_hist_kernel(BiasHistArgs a) {
    __shared__ u32 h[kBiasBins];
    if (a.out[kBiasBins + 1] == 0u) return;                   // no row with a finite term (uniform)
    const float lo = unord_f32(~a.out[kBiasBins]), hi = unord_f32(a.out[kBiasBins + 1]);
    const float width = hi > lo ? (hi - lo) / (float)kBiasBins : 0.0f;
    for (int i = threadIdx.x; i < kBiasBins; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += (int64_t)gridDim.x * blockDim.x) {
        const float term = bias_term_of(a, r);
        if (term == term) atomicAdd(&h[bias_bin(term, lo, width)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kBiasBins; i += blockDim.x)
        if (h[i]) atomicAdd(&a.out[i], h[i]);
}

struct BiasSelectArgs {
    const float* scores;      // [nq][row_stride] raw sample scores
    int row_stride;
    int64_t ntiles;           // sample tiles; position p = 32 * tile + row (positions >= 32 * ntiles hold -inf)
    int64_t tile_stride;      // sample tile j is global tile (j / run) * run * tile_stride + j % run
    int run;
    const float* bias;        // [n]
    float w;
    int kk;                   // threshold rank
    const u32* ghist;         // [kBiasHistWords] the call's histogram and range (bias_hist_kernel)
    double target;            // expected candidates per query the estimate aims at
    float* thr;               // [256]
    u32* count;               // [256]
};

constexpr int kBiasSelectLds = kLevelLds + kBiasBins * 4 + 2 * (kLevelThreads / 64) * 8 + (kLevelThreads / 64) * 4 * 8;
static_assert(kBiasSelectLds <= 160 * 1024, "the biased sample select must fit the CU's LDS");
static_assert(kLevelLds % 8 == 0, "the areas behind lds_select_top's are 8-byte aligned");

template <int KR>   // 1: kk <= 64, 4: kk <= 256 (as level_select_kernel)
__global__ void __launch_bounds__(kLevelThreads) sample_select_biased_kernel(BiasSelectArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NW = kLevelThreads / 64;
    const SelectLds lds = SelectLds::carve(smem, kLevelSortMax);   // keys: weighted sample scores keyed by position
    u32* bhist = (u32*)(smem + kLevelLds);                    // the call's histogram of w * bias, copied from a.ghist
    double* red = (double*)(bhist + kBiasBins);               // [2][NW] sums of the bisection
    double* stat = red + 2 * NW;                              // [NW][4]: sum, sum of squares, live rows, -
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int npos = (int)min(a.ntiles * (int64_t)kTileRows, (int64_t)kLevelSortMax);
    if (threadIdx.x == 0) {
        a.count[q] = 0;
        lds.ctr[kSelFill] = 0;                                // keys made
        lds.ctr[kSelShort] = 0;
    }
    for (int i = threadIdx.x; i < kLevelBins; i += blockDim.x) lds.hist[i] = 0;
    for (int i = threadIdx.x; i < kBiasBins; i += blockDim.x) bhist[i] = a.ghist[i];
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
        const bool live = raw == raw && raw > -INFINITY;      // a live position's row is a real, allowed row (< n)
        u64 key = 0ull;
        if (live) {
            const float ws = fmaf(a.w, a.bias[row_of(i)], raw);
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
    for (int w = 0; w < NW; ++w) {
        t1 += stat[4 * w];
        t2 += stat[4 * w + 1];
        live_rows += stat[4 * w + 2];
    }
    const double mu = live_rows > 0.0 ? t1 / live_rows : 0.0;
    const double sigma = live_rows > 0.0 ? sqrt(fmax(t2 / live_rows - mu * mu, 0.0)) : 0.0;
    // range of the call's histogram (no row with a finite term: hi < lo, and the solver has nothing to estimate from)
    const bool any_term = a.ghist[kBiasBins + 1] != 0u;
    const float lo = any_term ? unord_f32(~a.ghist[kBiasBins]) : INFINITY, hi = any_term ? unord_f32(a.ghist[kBiasBins + 1]) : -INFINITY;
    const float width = hi > lo ? (hi - lo) / (float)kBiasBins : 0.0f;
    const int cnt = (int)lds.ctr[kSelFill];

    // the guaranteed bound: the kk-th best weighted score of the sample
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
            for (int w = 0; w < NW; ++w) t += red[flip * NW + w];
            flip ^= 1;
            return t;
        };
        est = bias_solve_threshold(bhist, lo, width, hi, mu, sigma, 1.0, a.target, (int)threadIdx.x, (int)blockDim.x, total);
    }
    if (threadIdx.x == 0) a.thr[q] = fmaxf(bound, est);
}

}  // namespace ts
