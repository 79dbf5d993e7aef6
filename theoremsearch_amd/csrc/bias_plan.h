// The biased matrix search's host decisions (ts_search_biased_ex; search.hip, search_mfma.hip) and its threshold solver
// (kernels_sample_biased.h) as pure functions of plain values: which (storage type, width) the biased general-width pass
// serves, scan or matrix path, the batch from which AUTO prefers the matrix path, and the pass threshold of a query from the
// statistics of its threshold sample.  Nothing from HIP: the C ABI's codes (include/tsearch.h, plain C) and the standard
// library only, so tests/bias_plan_check.cpp runs all of it on the CPU under the host sanitizers.  The solver is also
// compiled for the device (TS_HD), where the threads of a workgroup share its sums.
#pragma once
#include <cmath>
#include <cstdint>

#include "anyd_plan.h"
#include "scan_plan.h"

#if defined(__HIPCC__)
#define TS_HD __host__ __device__
#else
#define TS_HD
#endif

namespace ts {

// ---------------------------------------------------------------------------------------------
// served widths, scan or matrix path
// ---------------------------------------------------------------------------------------------
// The biased pass is the general-width kernel (kernels_mfma_anyd.h) with the bias term in its epilogue: its row length is a
// run-time value, so it also runs the four widths the plain search gives to the hand-laid kernels (384 / 512 / 768 / 1024;
// a 4,096-byte row covers fp32 d = 1024).  A full pass only: the usual two-level search.
constexpr bool bias_served(int dtype, int d, bool two_level) {
    return (dtype == TS_BF16 || dtype == TS_F32) && two_level && d >= kAnydMinD && d % 64 == 0 &&
           anyd_row_bytes(dtype, d) <= kAnydMaxRowBytes;
}

// Largest batch AUTO still sends to the scan (AlgoInputs::scan_max_queries; scan_max_queries() drops it to 1 for k > 64,
// where the scan serves one query per pass - not timed for the biased search).  One pass of the kernel holds 256 queries
// whatever the batch, the scan pays a pass per four queries.  Measured on 1M rows, k = 10 (profiles/biased_timing.json,
// DESIGN.md section 3.4), scan against kernel in ms: bf16 at 5 queries - two scan passes - 0.75 against 0.63 (d = 768), 0.84
// against 0.72 (1024), 1.42 against 1.00 (1536): the limit is one scan pass.  fp32 runs the matrix pipe at 1/16 of the bf16
// rate: d = 768, 1.34 / 1.32 against 1.45 at 5 / 8 queries, 2.57 against 1.45 at 16 - two scan passes still win by 8-10 %, so
// fp32 batches of up to 8 stay on the scan (three scan passes are 1.5 x the two measured: above the kernel).
constexpr int kBiasScanMaxQueries = 4;
constexpr int kBiasScanMaxQueriesF32 = 8;
constexpr int bias_scan_max_queries(int dtype) { return dtype == TS_F32 ? kBiasScanMaxQueriesF32 : kBiasScanMaxQueries; }

// What ts_search_biased_ex runs.  `in`: the call as choose_algo() takes it (AlgoInputs::bias is not read here; mfma_ok is
// replaced by `served`); `served`: bias_served() for this index, rows unpadded, fp32 not switched off, at least one row.
// The mask rule is the filtered search's own (choose_algo with bias = false): a host mask that keeps at least a tenth of the
// rows, in front of a batch the matrix path takes.
inline AlgoInputs bias_algo_inputs(AlgoInputs in, bool served) {
    in.bias = false;
    in.mfma_ok = served;
    return in;
}
inline AlgoChoice choose_bias_algo(const AlgoInputs& call, bool served) {
    if (call.subset) return {0, "biased search on a subset index"};
    if (call.algo == TS_ALGO_SCAN) return {TS_ALGO_SCAN, nullptr};
    if (call.algo == TS_ALGO_MFMA && !served)
        return {0, "the biased matrix search needs a bf16 or fp32 index whose width is a multiple of 64 from 128 up to a 4,096-byte "
                   "row, under the default two-level search"};
    return choose_algo(bias_algo_inputs(call, served));
}

// ---------------------------------------------------------------------------------------------
// the pass threshold
// ---------------------------------------------------------------------------------------------
// A row's weighted score is similarity + w * bias[row].  The similarities of one query are close to Gaussian (normalised,
// high-dimensional rows: what the plain search's estimate assumes); the additive term is KNOWN, bounded, skewed and has a
// spike at 0 - a Gaussian fitted to the weighted scores overshoots the quantile and under-fills most queries (pinned in
// tests/test_bias_plan_cpu.py).  So the two terms are modelled apart: mu / sigma of the raw sample scores, and a histogram
// H of w * bias (kBiasBins bins of `width` from `lo`; a row counts at its bin's UPPER edge c_b, capped at `hi`, so the
// estimate errs towards more candidates).  Expected candidates of the full pass at threshold t:
//     E(t) = scale * sum_b H[b] * Q((t - c_b - mu) / sigma),    scale = rows the pass draws from / rows H counts,
// Q the standard normal tail.  The search takes H over every row the call may return (kernels_sample_biased.h: scale 1); a
// histogram of the threshold sample's rows alone (scale = rows / live sample rows) is too coarse for a heavy-tailed term.  E falls monotonically in t; bias_solve_threshold() bisects E(t) = target.
constexpr int kBiasBins = 1024;
constexpr int kBiasBisections = 26;      // the bracket is at most (hi - lo) + 18 sigma wide: 2^-26 of it is far below a score's ulp

TS_HD inline double normal_tail(double x) { return 0.5 * erfc(x * 0.70710678118654752440); }

// bin of a finite value v in [lo, hi] (width = (hi - lo) / kBiasBins; 0 when all values are equal: bin 0)
TS_HD inline int bias_bin(float v, float lo, float width) {
    if (!(width > 0.0f)) return 0;
    const float t = (v - lo) / width;
    return t >= (float)(kBiasBins - 1) ? kBiasBins - 1 : (t > 0.0f ? (int)t : 0);
}
TS_HD inline double bias_bin_edge(int b, float lo, float width, float hi) {
    const double c = (double)lo + (double)(b + 1) * (double)width;
    return c < (double)hi ? c : (double)hi;
}

// This caller's share of E(t) / scale: bins first, first + stride, ...
TS_HD inline double bias_expected_share(const uint32_t* hist, float lo, float width, float hi, double mu, double sigma, double t,
                                        int first, int stride) {
    double e = 0.0;
    for (int b = first; b < kBiasBins; b += stride)
        if (hist[b]) e += (double)hist[b] * normal_tail((t - bias_bin_edge(b, lo, width, hi) - mu) / sigma);
    return e;
}

// The t with E(t) = target, or -inf where there is nothing to estimate from (no live row with a finite term, sigma = 0) or
// where even the lowest threshold of the bracket admits fewer than target rows.  `total(x)`: the sum of x over the callers
// that share the bins (first / stride) - the identity for one caller (first = 0, stride = 1), a workgroup reduction on the
// device; every caller gets the same t.
template <class Total>
TS_HD inline float bias_solve_threshold(const uint32_t* hist, float lo, float width, float hi, double mu, double sigma, double scale,
                                        double target, int first, int stride, Total&& total) {
    if (!(sigma > 0.0) || !(scale > 0.0) || !(hi >= lo)) return -INFINITY;
    double a = mu + (double)lo - 9.0 * sigma, b = mu + (double)hi + 9.0 * sigma;      // E(a) ~ every row, E(b) ~ 0
    if (scale * total(bias_expected_share(hist, lo, width, hi, mu, sigma, a, first, stride)) < target) return -INFINITY;
    for (int it = 0; it < kBiasBisections; ++it) {
        const double mid = 0.5 * (a + b);
        const double e = scale * total(bias_expected_share(hist, lo, width, hi, mu, sigma, mid, first, stride));
        if (e >= target) a = mid;
        else b = mid;
    }
    return (float)a;                                                                  // E(a) >= target
}

}  // namespace ts
