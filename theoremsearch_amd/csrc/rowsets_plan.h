// The host decisions of ts_search_rowsets (search.hip, search_mfma.hip) as pure functions of plain values: the validation of
// its arguments, which queries ride the shared matrix pass and which go through per-set calls of the existing search, the
// delegations, and the per-query numbers of the pass (threshold estimate, re-run limit).  No handle, no HIP call: the C ABI's
// codes (include/tsearch.h, plain C) and the standard library only, so tests/rowsets_plan_check.cpp runs all of it on the CPU
// under the host sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/tsearch.h"
#include "bias_plan.h"

namespace ts {

constexpr int kRowsetsBlock = 256;        // queries of one shared pass (kAnydQueries): a longer list goes in blocks
constexpr int kRowsetsMinSets = 2;        // distinct sets from which AUTO prefers the shared pass (provisional: DESIGN.md 3.3c)
static_assert(TS_MAX_ROWSETS == kRowsetsBlock, "a block's table holds one mask pointer per query at the most");
static_assert(kRowsetsBlock == kAnydQueries, "the shared pass is the general-width kernel's launch");

// Inverse of the standard normal CDF (Acklam's rational approximation, |error| < 1.2e-9): the z with P(X > z) = p.
inline double normal_tail_z(double p) {
    if (p <= 0.0) return 8.0;
    if (p >= 0.5) return 0.0;
    const double q = std::sqrt(-2.0 * std::log(p));
    static const double c[] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
                               -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
    static const double d[] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00};
    if (p < 0.02425)
        return -(((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) /
               ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0);
    // central region
    static const double a[] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
                               1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
    static const double b[] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
                               6.680131188771972e+01, -1.328068155288572e+01};
    const double x = (1.0 - p) - 0.5, r = x * x;
    return (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * x /
           (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0);
}

// ---------------------------------------------------------------------------------------------
// arguments: NULL = valid, else the text of TS_ERR_INVALID; the sizes are judged before the pointers
// ---------------------------------------------------------------------------------------------
inline const char* rowsets_args_invalid(bool has_queries, bool has_scores, bool has_idx, bool has_sets, bool has_which, int q_dtype, int nq,
                                        int k, int nsets, int algo) {
    if (q_dtype != TS_F32 && q_dtype != TS_BF16) return "q_dtype is neither TS_F32 nor TS_BF16";
    if (nq < 0) return "nq is negative";
    if (k < 1 || k > TS_MAX_K) return "k outside [1, TS_MAX_K]";
    if (nsets < 0 || nsets > TS_MAX_ROWSETS) return "nsets outside [0, TS_MAX_ROWSETS]";
    if (algo < TS_ALGO_AUTO || algo > TS_ALGO_MFMA) return "algo out of range";
    if (!has_queries || !has_scores || !has_idx) return "NULL argument";
    if (nsets > 0 && !has_sets) return "sets is NULL";
    if (nq > 0 && !has_which) return "which is NULL";
    return nullptr;
}

// What the routing needs to know of a row set; present = the entry of sets[] is not NULL.
struct RowsetsSet {
    bool present;
    int64_t n, allowed;
    int device;
};

// which[] against sets[] (judged without the index), then the index handle, then the named sets against the index (n rows on
// `device`): the rules of ts_search_rowset per set
inline const char* rowsets_sets_invalid(const RowsetsSet* sets, int nsets, const int32_t* which, int nq, bool has_index, int64_t n, int device) {
    for (int q = 0; q < nq; ++q) {
        const int32_t s = which[q];
        if (s < -1 || s >= nsets) return "an entry of which lies outside [-1, nsets)";
        if (s >= 0 && !sets[s].present) return "which names an entry of sets that is NULL";
    }
    if (!has_index) return "NULL argument";
    for (int q = 0; q < nq; ++q) {
        const int32_t s = which[q];
        if (s < 0) continue;
        if (sets[s].n != n) return "a named row set has another number of rows than the index";
        if (sets[s].device != device) return "a named row set lives on another device than the index";
    }
    return nullptr;
}

// ---------------------------------------------------------------------------------------------
// routing
// ---------------------------------------------------------------------------------------------
// The index and its options, as far as the routing reads them.
struct RowsetsIndex {
    int dtype, d;
    int64_t n;
    bool unpadded;            // ld == d
    bool two_level;           // the default two-level search (neither TS_MFMA_STAT=0 nor TS_MFMA_SAMPLE=0)
    bool f32_matrix;          // fp32 indexes: not switched off the matrix path (TS_MFMA_F32=0)
    int mfma_min_rows;        // TS_MFMA_MIN_ROWS
    int scan_max_knob;        // TS_SCAN_MAX_QUERIES, or the default of the general-width pass (bias_scan_max_queries)
};

// The shared pass is the general-width kernel at every width it can run (bias_served: the hand-laid widths included)
inline bool rowsets_pass_served(const RowsetsIndex& ix) {
    if (ix.dtype == TS_F32 && !ix.f32_matrix) return false;
    return ix.unpadded && ix.n >= 1 && ix.n >= ix.mfma_min_rows && bias_served(ix.dtype, ix.d, ix.two_level);
}

// rows query q may return: its set's count, n behind -1
inline int64_t rowsets_pop(const RowsetsSet* sets, int32_t which_q, int64_t n) { return which_q < 0 ? n : sets[which_q].allowed; }

// the tenth rule of the filtered matrix search (scan_plan.h: choose_algo)
inline bool rowsets_dense(int64_t allowed, int64_t n) { return allowed * 10 >= n; }

enum RowsetsKind {
    kRowsetsUnsupported = 0,  // TS_ERR_UNSUPPORTED with RowsetsRoute::unsupported
    kRowsetsSearchEx,         // every query names -1: the call is ts_search_ex
    kRowsetsSearchRowset,     // every query names sets[one_set]: the call is ts_search_rowset
    kRowsetsSplit             // the shared pass for `pass`, one call of the existing search per entry of `groups`
};

struct RowsetsGroup {
    int32_t set;                    // -1: every row
    bool empty;                     // the set allows nothing: padding, no launch
    std::vector<int32_t> queries;   // ascending
};

struct RowsetsRoute {
    int kind = kRowsetsUnsupported;
    const char* unsupported = nullptr;
    int32_t one_set = -1;
    int group_algo = TS_ALGO_AUTO;       // what the per-set calls are given
    int sets_used = 0;                   // distinct entries of sets[] that which[] names
    std::vector<int32_t> pass;           // queries of the shared pass, ascending; blocks of kRowsetsBlock
    std::vector<RowsetsGroup> groups;    // by set, -1 first
    int pass_blocks() const { return ((int)pass.size() + kRowsetsBlock - 1) / kRowsetsBlock; }
    int scan_queries() const {
        int c = 0;
        for (const RowsetsGroup& g : groups) c += (int)g.queries.size();
        return c;
    }
    int scan_calls() const {
        int c = 0;
        for (const RowsetsGroup& g : groups) c += g.empty ? 0 : 1;
        return c;
    }
};

// nq >= 1, arguments valid (above); a subset index is refused by the caller before this.
inline RowsetsRoute rowsets_route(const RowsetsIndex& ix, const RowsetsSet* sets, int nsets, const int32_t* which, int nq, int k, int algo) {
    RowsetsRoute r;
    std::vector<char> named((size_t)nsets + 1, 0);         // [0]: -1
    for (int q = 0; q < nq; ++q) named[(size_t)(which[q] + 1)] = 1;
    int distinct = 0;
    for (int s = 0; s <= nsets; ++s) distinct += named[(size_t)s];
    r.sets_used = distinct - named[0];
    if (distinct <= 1) {
        r.kind = named[0] ? kRowsetsSearchEx : kRowsetsSearchRowset;
        r.one_set = which[0];
        return r;
    }
    // queries that may ride the pass, and the distinct sets they name
    std::vector<char> rides((size_t)nq, 0);
    int eligible = 0;
    if (algo != TS_ALGO_SCAN && rowsets_pass_served(ix)) {
        std::vector<char> dense_named((size_t)nsets + 1, 0);
        for (int q = 0; q < nq; ++q)
            if (rowsets_dense(rowsets_pop(sets, which[q], ix.n), ix.n)) {
                rides[(size_t)q] = 1;
                ++eligible;
                dense_named[(size_t)(which[q] + 1)] = 1;
            }
        int dense_sets = 0;
        for (int s = 0; s <= nsets; ++s) dense_sets += dense_named[(size_t)s];
        const bool run = eligible > scan_max_queries(k, ix.scan_max_knob) && dense_sets >= kRowsetsMinSets;
        if (!run) {
            std::fill(rides.begin(), rides.end(), 0);
            eligible = 0;
        }
    }
    if (algo == TS_ALGO_MFMA && eligible != nq) {
        r.unsupported = "TS_ALGO_MFMA: the shared pass needs a bf16 or fp32 index of at least TS_MFMA_MIN_ROWS rows whose width is a "
                        "multiple of 64 from 128 up to a 4,096-byte row, under the default two-level search, and every query behind "
                        "a set that allows at least a tenth of the rows, more queries than one scan pass serves";
        return r;
    }
    r.kind = kRowsetsSplit;
    r.group_algo = algo == TS_ALGO_SCAN ? TS_ALGO_SCAN : TS_ALGO_AUTO;
    for (int q = 0; q < nq; ++q)
        if (rides[(size_t)q]) r.pass.push_back(q);
    for (int s = -1; s < nsets; ++s) {
        if (!named[(size_t)(s + 1)]) continue;
        RowsetsGroup g;
        g.set = s;
        g.empty = s >= 0 && sets[s].allowed <= 0;
        for (int q = 0; q < nq; ++q)
            if (which[q] == s && !rides[(size_t)q]) g.queries.push_back(q);
        if (!g.queries.empty()) r.groups.push_back(std::move(g));
    }
    return r;
}

// ---------------------------------------------------------------------------------------------
// the per-query numbers of the pass
// ---------------------------------------------------------------------------------------------
// What search_mfma.hip's plan computes once per call from the call's population, per query from its own: the Gaussian-tail
// quantile of the threshold estimate, the exceedance probability of the tail fit (0 = not armed) and the fewest candidates
// the final select accepts before it sends the query to the exact re-run.
struct RowsetsNumbers {
    float z_tail, tail_p;
    int32_t min_fill;
};
// kk: the threshold rank (>= k); stat_cands: expected candidates the estimate aims at; sample_rows: rows of the threshold
// sample; cand_cap: a query's candidate slots; estimate: the statistical two-level search; tail_fit: TS_MFMA_TAIL_FIT
inline RowsetsNumbers rowsets_numbers(int64_t pop, int64_t n, int k, int kk, int stat_cands, double sample_rows, int cand_cap, bool estimate,
                                      bool tail_fit) {
    RowsetsNumbers r;
    r.z_tail = estimate ? (float)normal_tail_z(std::min(0.25, (double)stat_cands / (double)std::max<int64_t>(pop, 1))) : 0.0f;
    const bool bound_swamps = (double)kk * (double)n / sample_rows > 0.5 * cand_cap;
    r.tail_p = (r.z_tail > 0.0f && bound_swamps && tail_fit)
                   ? (float)std::min(0.25, (double)std::max(2048, 8 * kk) / (double)std::max<int64_t>(pop, 1))
                   : 0.0f;
    r.min_fill = (int32_t)std::min<int64_t>(k, pop);
    return r;
}
// where the sample select cuts first: ~2 kl of the query's live sample rows above it on Gaussian-like scores
inline float rowsets_z_sel(int64_t pop, int64_t n, int kk, float tail_p, double sample_rows) {
    const int kl = tail_p > 0.0f ? std::max(kk, 32) : kk;
    const double live = sample_rows * (double)pop / (double)std::max<int64_t>(n, 1);
    return (float)normal_tail_z(std::min(0.25, 2.0 * kl / std::max(live, 1.0)));
}

// One block's table on the device: what the three kernels of the pass read per query.  Entries past the block's queries: set
// -1 (no mask), numbers of the whole corpus.
struct RowsetsTable {
    const uint32_t* mask[kRowsetsBlock];      // by set number: sets[s]'s device mask (entries nobody names: NULL)
    float z_tail[kRowsetsBlock], tail_p[kRowsetsBlock], z_sel[kRowsetsBlock];
    int32_t min_fill[kRowsetsBlock];
    int32_t set[kRowsetsBlock];               // per query: index into mask[], -1 = every row
};

}  // namespace ts
