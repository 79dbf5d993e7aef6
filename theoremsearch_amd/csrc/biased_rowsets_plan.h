// The host decisions of ts_search_biased_rowsets (search.hip, search_mfma.hip) and the weight mapping of its threshold
// estimate (kernels_biased_rowsets.h) as pure functions of plain values: the validation of its arguments, the classes
// (set, weight) of its queries, which of them ride the shared matrix pass and which go through one call of the existing
// biased search per class, the delegation, and the solver that reads ONE histogram of the raw bias per set through each
// query's own weight.  No handle, no HIP call: rowsets_plan.h and bias_plan.h and the standard library only, so
// tests/biased_rowsets_plan_check.cpp runs all of it on the CPU under the host sanitizers.  The solver is also compiled for
// the device (TS_HD), where the threads of a workgroup share its sums.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "bias_plan.h"
#include "rowsets_plan.h"

namespace ts {

// Classes from which AUTO prefers the shared pass to one call per class.  Measured on 1M x 768 bf16, 256 queries, k = 10, sets of
// density 0.5 (profiles/biased_rowsets_timing.json), pass against calls in ms: 1.38 against 1.76 at 2 classes
// (the per-class form's own spread: 0.06), 1.42 against 3.00 at 4, 1.83 against 67.6 at 256 - the pass wins from 2 on.
constexpr int kBiasedRowsetsMinClasses = 2;
// sets whose histograms one workgroup of bias_hist_sets_kernel keeps in its LDS (kBiasBins * 4 bytes each: 64 KB)
constexpr int kBiasedRowsetsHistGroup = 16;

// ---------------------------------------------------------------------------------------------
// arguments: NULL = valid, else the text of TS_ERR_INVALID (the sibling's rules first, in its order)
// ---------------------------------------------------------------------------------------------
inline const char* biased_rowsets_args_invalid(bool has_queries, bool has_scores, bool has_idx, bool has_sets, bool has_which, bool has_bias,
                                               const float* weights, int q_dtype, int nq, int k, int nsets, int algo) {
    if (const char* bad = rowsets_args_invalid(has_queries, has_scores, has_idx, has_sets, has_which, q_dtype, nq, k, nsets, algo)) return bad;
    if (!has_bias) return "bias is NULL";
    if (nq > 0 && !weights) return "weights is NULL";
    for (int q = 0; q < nq; ++q)
        if (!(std::fabs(weights[q]) < INFINITY)) return "a weight is not finite";
    return nullptr;
}

// ---------------------------------------------------------------------------------------------
// routing
// ---------------------------------------------------------------------------------------------
// Weights are classed by VALUE: -0.0f and 0.0f give every row the same key (fmaf(+-0, b, s) == s for a finite b, NaN for
// both otherwise), so they are one class.
inline bool biased_rowsets_same_class(int32_t set_a, float w_a, int32_t set_b, float w_b) { return set_a == set_b && w_a == w_b; }

enum BiasedRowsetsKind {
    kBiasedRowsetsUnsupported = 0,   // TS_ERR_UNSUPPORTED with BiasedRowsetsRoute::unsupported
    kBiasedRowsetsOneClass,          // one (set, weight): the call is ts_search_biased_rowset (set -1: ts_search_biased_ex)
    kBiasedRowsetsSplit              // the shared pass for `pass`, one call of the biased search per entry of `groups`
};

struct BiasedRowsetsGroup {
    int32_t set;                     // -1: every row
    float weight;
    bool empty;                      // the set allows nothing: padding, no launch
    std::vector<int32_t> queries;    // ascending
};

struct BiasedRowsetsRoute {
    int kind = kBiasedRowsetsUnsupported;
    const char* unsupported = nullptr;
    int32_t one_set = -1;
    float one_weight = 0.0f;
    int group_algo = TS_ALGO_AUTO;
    int sets_used = 0;                        // distinct entries of sets[] that which[] names
    int classes = 0;                          // distinct (set, weight) pairs of the call
    std::vector<int32_t> pass;                // queries of the shared pass, ascending; blocks of kRowsetsBlock
    std::vector<BiasedRowsetsGroup> groups;   // by first appearance of the class
    int pass_blocks() const { return ((int)pass.size() + kRowsetsBlock - 1) / kRowsetsBlock; }
    int scan_queries() const {
        int c = 0;
        for (const BiasedRowsetsGroup& g : groups) c += (int)g.queries.size();
        return c;
    }
    int scan_calls() const {
        int c = 0;
        for (const BiasedRowsetsGroup& g : groups) c += g.empty ? 0 : 1;
        return c;
    }
};

// class number of every query, by first appearance; returns the number of classes
inline int biased_rowsets_classes(const int32_t* which, const float* weights, int nq, std::vector<int32_t>* cls) {
    std::vector<int32_t> first;               // a query of each class
    cls->assign((size_t)nq, 0);
    for (int q = 0; q < nq; ++q) {
        size_t c = 0;
        while (c < first.size() && !biased_rowsets_same_class(which[first[c]], weights[first[c]], which[q], weights[q])) ++c;
        if (c == first.size()) first.push_back(q);
        (*cls)[(size_t)q] = (int32_t)c;
    }
    return (int)first.size();
}

// nq >= 1, arguments valid (above, and rowsets_sets_invalid); a subset index is refused by the caller before this.
inline BiasedRowsetsRoute biased_rowsets_route(const RowsetsIndex& ix, const RowsetsSet* sets, int nsets, const int32_t* which,
                                               const float* weights, int nq, int k, int algo) {
    BiasedRowsetsRoute r;
    std::vector<char> named((size_t)nsets + 1, 0);         // [0]: -1
    for (int q = 0; q < nq; ++q) named[(size_t)(which[q] + 1)] = 1;
    for (int s = 1; s <= nsets; ++s) r.sets_used += named[(size_t)s];
    std::vector<int32_t> cls;
    r.classes = biased_rowsets_classes(which, weights, nq, &cls);
    if (r.classes == 1) {
        r.kind = kBiasedRowsetsOneClass;
        r.one_set = which[0];
        r.one_weight = weights[0];
        return r;
    }
    // queries that may ride the pass, and the classes they span
    std::vector<char> rides((size_t)nq, 0);
    int eligible = 0;
    if (algo != TS_ALGO_SCAN && rowsets_pass_served(ix)) {
        std::vector<char> dense_class((size_t)r.classes, 0);
        for (int q = 0; q < nq; ++q)
            if (rowsets_dense(rowsets_pop(sets, which[q], ix.n), ix.n)) {
                rides[(size_t)q] = 1;
                ++eligible;
                dense_class[(size_t)cls[(size_t)q]] = 1;
            }
        int dense_classes = 0;
        for (char c : dense_class) dense_classes += c;
        const bool run = eligible > scan_max_queries(k, ix.scan_max_knob) && dense_classes >= kBiasedRowsetsMinClasses;
        if (!run) {
            std::fill(rides.begin(), rides.end(), 0);
            eligible = 0;
        }
    }
    if (algo == TS_ALGO_MFMA && eligible != nq) {
        r.unsupported = "TS_ALGO_MFMA: the shared biased pass needs a bf16 or fp32 index of at least TS_MFMA_MIN_ROWS rows whose width is a "
                        "multiple of 64 from 128 up to a 4,096-byte row, under the default two-level search, and every query behind "
                        "a set that allows at least a tenth of the rows, more queries than one scan pass serves";
        return r;
    }
    r.kind = kBiasedRowsetsSplit;
    r.group_algo = algo == TS_ALGO_SCAN ? TS_ALGO_SCAN : TS_ALGO_AUTO;
    for (int q = 0; q < nq; ++q)
        if (rides[(size_t)q]) r.pass.push_back(q);
    std::vector<int32_t> group_of((size_t)r.classes, -1);
    for (int q = 0; q < nq; ++q) {
        if (rides[(size_t)q]) continue;
        int32_t& g = group_of[(size_t)cls[(size_t)q]];
        if (g < 0) {
            g = (int32_t)r.groups.size();
            r.groups.push_back(BiasedRowsetsGroup{which[q], weights[q], which[q] >= 0 && sets[which[q]].allowed <= 0, {}});
        }
        r.groups[(size_t)g].queries.push_back(q);
    }
    return r;
}

// The histograms a pass needs: one per distinct set among its queries (-1: every row), numbered by first appearance.
// hist_of[j]: the histogram of pass query j; sets_out: the set of each histogram.
inline int biased_rowsets_hists(const int32_t* which_pass, int npass, std::vector<int32_t>* hist_of, std::vector<int32_t>* sets_out) {
    hist_of->assign((size_t)npass, 0);
    sets_out->clear();
    for (int j = 0; j < npass; ++j) {
        size_t h = 0;
        while (h < sets_out->size() && (*sets_out)[h] != which_pass[j]) ++h;
        if (h == sets_out->size()) sets_out->push_back(which_pass[j]);
        (*hist_of)[(size_t)j] = (int32_t)h;
    }
    return (int)sets_out->size();
}
// bytes the histogram stage reads per call: `bias` once for the range and once per group of kBiasedRowsetsHistGroup
// histograms, each set's mask once (n / 8 bytes)
inline int64_t biased_rowsets_hist_bytes(int64_t n, int nhists, int nmasks) {
    const int64_t groups = (nhists + kBiasedRowsetsHistGroup - 1) / kBiasedRowsetsHistGroup;
    return n * 4 * (1 + groups) + (n / 8) * (int64_t)nmasks;
}

// ---------------------------------------------------------------------------------------------
// the pass threshold under a weight per query
// ---------------------------------------------------------------------------------------------
// H counts the RAW bias of a set's rows (finite values only; kBiasBins bins of `width` from `lo`, the range of all rows).  A
// query with weight w reads it as the histogram of its own term w * bias: a row of bin b has a term of at most
//     w * (upper edge of b, capped at hi)   for w >= 0,
//     w * (lower edge of b)                 for w <  0   (the bins' order reverses: the lowest bias gives the highest term),
// so the estimate errs towards more candidates, as bias_plan.h's does.  w = 0: every term is 0, E(t) = rows * Q((t - mu) /
// sigma) - the plain search's Gaussian tail.
TS_HD inline double biased_rowsets_term_edge(int b, float lo, float width, float hi, float w) {
    if (w >= 0.0f) return (double)w * bias_bin_edge(b, lo, width, hi);
    return (double)w * ((double)lo + (double)b * (double)width);
}

// This caller's share of E(t): bins first, first + stride, ...
TS_HD inline double biased_rowsets_expected_share(const uint32_t* hist, float lo, float width, float hi, float w, double mu, double sigma,
                                                  double t, int first, int stride) {
    double e = 0.0;
    for (int b = first; b < kBiasBins; b += stride)
        if (hist[b]) e += (double)hist[b] * normal_tail((t - biased_rowsets_term_edge(b, lo, width, hi, w) - mu) / sigma);
    return e;
}

// bias_solve_threshold() for (raw histogram, w): the t with E(t) = target, or -inf where there is nothing to estimate from
// or even the lowest threshold of the bracket admits fewer than target rows.  `total`: as there.
template <class Total>
TS_HD inline float biased_rowsets_solve_threshold(const uint32_t* hist, float lo, float width, float hi, float w, double mu, double sigma,
                                                  double target, int first, int stride, Total&& total) {
    if (!(sigma > 0.0) || !(hi >= lo)) return -INFINITY;
    const double e0 = (double)w * (double)lo, e1 = (double)w * (double)hi;
    double a = mu + (e0 < e1 ? e0 : e1) - 9.0 * sigma, b = mu + (e0 < e1 ? e1 : e0) + 9.0 * sigma;      // E(a) ~ every row, E(b) ~ 0
    if (total(biased_rowsets_expected_share(hist, lo, width, hi, w, mu, sigma, a, first, stride)) < target) return -INFINITY;
    for (int it = 0; it < kBiasBisections; ++it) {
        const double mid = 0.5 * (a + b);
        const double e = total(biased_rowsets_expected_share(hist, lo, width, hi, w, mu, sigma, mid, first, stride));
        if (e >= target) a = mid;
        else b = mid;
    }
    return (float)a;                                                                                    // E(a) >= target
}

// One block's table on the device.  The row-set kernels the pass reuses (sample scores, final select) are handed its first
// member; the biased pass, its sample select and the unbias step read the rest.
struct BiasedRowsetsTable {
    RowsetsTable r;
    float weight[kRowsetsBlock];              // per query (entries past the block's queries: 0)
    int32_t hist[kRowsetsBlock];              // per query: which of the call's histograms is its set's
};

}  // namespace ts
