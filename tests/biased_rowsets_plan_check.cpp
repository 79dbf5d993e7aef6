// Stand-alone check of theoremsearch_amd/csrc/biased_rowsets_plan.h, the host decisions of ts_search_biased_rowsets and the
// weight mapping of its threshold estimate (tests/test_biased_rowsets_plan_cpu.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it).  Exit 0 = every check held; otherwise each failed check is printed.
#include "biased_rowsets_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace ts;

static int g_failed = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++g_failed <= 40) {                        \
                printf("FAILED %s:%d: %s  [", __func__, __LINE__, #cond); \
                printf(__VA_ARGS__);                       \
                printf("]\n");                             \
            }                                              \
        }                                                  \
    } while (0)

static bool says(const char* text, const char* part) { return text && strstr(text, part); }

constexpr int64_t kN = 20000;

static RowsetsIndex index_of(int dtype = TS_BF16, int d = 768, int64_t n = kN) {
    RowsetsIndex ix;
    ix.dtype = dtype;
    ix.d = d;
    ix.n = n;
    ix.unpadded = true;
    ix.two_level = true;
    ix.f32_matrix = true;
    ix.mfma_min_rows = 16384;
    ix.scan_max_knob = bias_scan_max_queries(dtype);
    return ix;
}
static RowsetsSet set_of(int64_t allowed, int64_t n = kN, int device = 0) { return RowsetsSet{true, n, allowed, device}; }

// ---- every refusal --------------------------------------------------------------------------------------------------------
static void refusals() {
    const float w4[4] = {0.0f, 0.25f, -0.5f, 1.0f};
    auto args = [&](bool q, bool s, bool i, bool sets, bool which, bool bias, const float* w, int dt, int nq, int k, int nsets, int algo) {
        return biased_rowsets_args_invalid(q, s, i, sets, which, bias, w, dt, nq, k, nsets, algo);
    };
    CHECK(args(true, true, true, true, true, true, w4, TS_F32, 4, 10, 2, TS_ALGO_AUTO) == nullptr, "a valid call");
    CHECK(args(true, true, true, true, false, true, nullptr, TS_F32, 0, 10, 2, TS_ALGO_AUTO) == nullptr, "nq == 0 needs neither which nor weights");
    CHECK(says(args(true, true, true, true, true, false, w4, TS_F32, 4, 10, 2, 0), "bias is NULL"), "bias");
    CHECK(says(args(true, true, true, true, true, false, nullptr, TS_F32, 0, 10, 2, 0), "bias is NULL"), "bias, nq == 0");
    CHECK(says(args(true, true, true, true, true, true, nullptr, TS_F32, 4, 10, 2, 0), "weights is NULL"), "weights");
    for (float bad : {(float)NAN, (float)INFINITY, -(float)INFINITY})
        for (int at = 0; at < 4; ++at) {
            float w[4] = {0.0f, 0.25f, -0.5f, 1.0f};
            w[at] = bad;
            CHECK(says(args(true, true, true, true, true, true, w, TS_F32, 4, 10, 2, 0), "not finite"), "weight %g at %d", (double)bad, at);
        }
    // the sibling's rules come first, in its order: the sizes before the pointers, those before the bias and the weights
    CHECK(says(args(false, false, false, false, false, false, nullptr, TS_F32, 4, 0, 2, 0), "k outside"), "sizes first");
    CHECK(says(args(false, true, true, true, true, false, nullptr, TS_F32, 4, 10, 2, 0), "NULL argument"), "queries before bias");
    CHECK(says(args(true, true, true, true, false, false, nullptr, TS_F32, 4, 10, 2, 0), "which is NULL"), "which before bias");
    CHECK(says(args(true, true, true, true, true, true, w4, 7, 4, 10, 2, 0), "q_dtype"), "q_dtype");
    CHECK(says(args(true, true, true, true, true, true, w4, TS_F32, -1, 10, 2, 0), "nq is negative"), "nq");
    CHECK(says(args(true, true, true, true, true, true, w4, TS_F32, 4, TS_MAX_K + 1, 2, 0), "k outside"), "k");
    CHECK(says(args(true, true, true, true, true, true, w4, TS_F32, 4, 10, TS_MAX_ROWSETS + 1, 0), "nsets outside"), "nsets");
    CHECK(says(args(true, true, true, true, true, true, w4, TS_F32, 4, 10, 2, 3), "algo"), "algo");
}

// ---- classes and delegation ----------------------------------------------------------------------------------------------
static void classes_and_delegation() {
    {
        const int32_t which[6] = {0, 0, -1, 0, -1, 1};
        const float w[6] = {0.5f, 0.25f, 0.5f, 0.5f, 0.5f, 0.5f};
        std::vector<int32_t> cls;
        CHECK(biased_rowsets_classes(which, w, 6, &cls) == 4, "classes");
        CHECK(cls == (std::vector<int32_t>{0, 1, 2, 0, 2, 3}), "numbered by first appearance");
    }
    {   // by value: -0 and +0 are one class
        const int32_t which[2] = {0, 0};
        const float w[2] = {0.0f, -0.0f};
        std::vector<int32_t> cls;
        CHECK(biased_rowsets_classes(which, w, 2, &cls) == 1, "signed zeros");
    }
    std::vector<RowsetsSet> sets = {set_of(10000), set_of(5)};
    for (int algo : {TS_ALGO_AUTO, TS_ALGO_SCAN, TS_ALGO_MFMA}) {
        std::vector<int32_t> one(40, 1), all(40, -1);
        std::vector<float> w(40, 0.25f);
        BiasedRowsetsRoute r = biased_rowsets_route(index_of(), sets.data(), 2, one.data(), w.data(), 40, 10, algo);
        CHECK(r.kind == kBiasedRowsetsOneClass && r.one_set == 1 && r.one_weight == 0.25f && r.sets_used == 1 && r.classes == 1 && r.pass.empty() && r.groups.empty(),
              "one class, algo %d", algo);
        r = biased_rowsets_route(index_of(), sets.data(), 2, all.data(), w.data(), 40, 10, algo);
        CHECK(r.kind == kBiasedRowsetsOneClass && r.one_set == -1 && r.sets_used == 0, "all -1, algo %d", algo);
        // the same set under two weights is two classes: no delegation
        w[7] = 0.5f;
        std::vector<int32_t> dense(40, 0);
        r = biased_rowsets_route(index_of(), sets.data(), 2, dense.data(), w.data(), 40, 10, algo);
        CHECK(r.kind == kBiasedRowsetsSplit && r.classes == 2 && r.sets_used == 1, "two weights, algo %d: kind %d", algo, r.kind);
        if (algo == TS_ALGO_SCAN) CHECK(r.pass.empty() && r.groups.size() == 2 && r.group_algo == TS_ALGO_SCAN, "scan: one group per class");
        else CHECK(r.pass.size() == 40 && r.groups.empty(), "the pass takes all 40 (algo %d): %zu", algo, r.pass.size());
    }
}

// ---- the split -------------------------------------------------------------------------------------------------------------
static void split() {
    // sets: 0 dense, 1 sparse (5 %), 2 empty
    std::vector<RowsetsSet> sets = {set_of(10000), set_of(1000), set_of(0)};
    std::vector<int32_t> which;
    std::vector<float> w;
    for (int q = 0; q < 64; ++q) {
        const int m = q % 8;
        which.push_back(m < 3 ? -1 : m < 6 ? 0 : m == 6 ? 1 : 2);
        w.push_back(m == 4 ? 0.5f : 0.25f);
    }
    BiasedRowsetsRoute r = biased_rowsets_route(index_of(), sets.data(), 3, which.data(), w.data(), 64, 10, TS_ALGO_AUTO);
    CHECK(r.kind == kBiasedRowsetsSplit && r.classes == 5 && r.sets_used == 3, "kind %d classes %d sets %d", r.kind, r.classes, r.sets_used);
    CHECK(r.pass.size() == 48 && r.groups.size() == 2, "pass %zu groups %zu", r.pass.size(), r.groups.size());
    for (size_t j = 0; j < r.pass.size(); ++j) CHECK(which[(size_t)r.pass[j]] <= 0 && (j == 0 || r.pass[j] > r.pass[j - 1]), "pass query %d", r.pass[j]);
    CHECK(r.groups[0].set == 1 && !r.groups[0].empty && r.groups[0].queries.size() == 8 && r.groups[0].weight == 0.25f, "the sparse class");
    CHECK(r.groups[1].set == 2 && r.groups[1].empty && r.groups[1].queries.size() == 8, "the empty class");
    CHECK(r.scan_queries() == 16 && r.scan_calls() == 1 && r.group_algo == TS_ALGO_AUTO, "scan %d calls %d", r.scan_queries(), r.scan_calls());
    // the MFMA refusal: not every query rides
    r = biased_rowsets_route(index_of(), sets.data(), 3, which.data(), w.data(), 64, 10, TS_ALGO_MFMA);
    CHECK(r.kind == kBiasedRowsetsUnsupported && says(r.unsupported, "TS_ALGO_MFMA"), "MFMA with a sparse class");
    // scan: every class its own group, in order of first appearance
    r = biased_rowsets_route(index_of(), sets.data(), 3, which.data(), w.data(), 64, 10, TS_ALGO_SCAN);
    CHECK(r.kind == kBiasedRowsetsSplit && r.pass.empty() && r.groups.size() == 5 && r.scan_calls() == 4 && r.scan_queries() == 64, "scan: %zu groups", r.groups.size());
    CHECK(r.groups[0].set == -1 && r.groups[1].set == 0 && r.groups[1].weight == 0.25f && r.groups[2].set == 0 && r.groups[2].weight == 0.5f, "group order");

    // too few pass queries (4 is one scan pass of a bf16 index), an unserved width, a small index, k-chunked widths: per class
    std::vector<int32_t> few = {0, 0, -1, -1};
    std::vector<float> fw = {0.25f, 0.5f, 0.25f, 0.5f};
    r = biased_rowsets_route(index_of(), sets.data(), 3, few.data(), fw.data(), 4, 10, TS_ALGO_AUTO);
    CHECK(r.kind == kBiasedRowsetsSplit && r.pass.empty() && r.groups.size() == 4, "4 queries: %zu ride", r.pass.size());
    r = biased_rowsets_route(index_of(), sets.data(), 3, few.data(), fw.data(), 4, 10, TS_ALGO_MFMA);
    CHECK(r.kind == kBiasedRowsetsUnsupported, "MFMA with 4 queries");
    r = biased_rowsets_route(index_of(), sets.data(), 3, few.data(), fw.data(), 4, 100, TS_ALGO_AUTO);
    CHECK(r.pass.size() == 4, "k > 64: the scan serves one query per pass, 4 ride (%zu)", r.pass.size());
    std::vector<int32_t> many(16);
    std::vector<float> mw(16);
    for (int q = 0; q < 16; ++q) {
        many[(size_t)q] = (q & 1) ? 0 : -1;
        mw[(size_t)q] = 0.25f * (float)(q % 3);
    }
    for (const RowsetsIndex& ix : {index_of(TS_BF16, 4096), index_of(TS_BF16, 100), index_of(TS_BF16, 768, 10000), index_of(TS_F32, 2048)}) {
        std::vector<RowsetsSet> s2 = {set_of(ix.n / 2, ix.n)};
        r = biased_rowsets_route(ix, s2.data(), 1, many.data(), mw.data(), 16, 10, TS_ALGO_AUTO);
        CHECK(r.kind == kBiasedRowsetsSplit && r.pass.empty() && r.groups.size() == 6, "d %d n %lld: %zu ride", ix.d, (long long)ix.n, r.pass.size());
        r = biased_rowsets_route(ix, s2.data(), 1, many.data(), mw.data(), 16, 10, TS_ALGO_MFMA);
        CHECK(r.kind == kBiasedRowsetsUnsupported, "MFMA at d %d n %lld", ix.d, (long long)ix.n);
    }
    {   // fp32: two scan passes (8 queries) stay on the scan
        std::vector<RowsetsSet> s2 = {set_of(kN / 2)};
        r = biased_rowsets_route(index_of(TS_F32, 128), s2.data(), 1, many.data(), mw.data(), 8, 10, TS_ALGO_AUTO);
        CHECK(r.pass.empty(), "fp32, 8 queries");
        r = biased_rowsets_route(index_of(TS_F32, 128), s2.data(), 1, many.data(), mw.data(), 9, 10, TS_ALGO_AUTO);
        CHECK(r.pass.size() == 9, "fp32, 9 queries");
    }
    static_assert(kBiasedRowsetsMinClasses >= 2, "one class is delegated before the pass is considered");
}

// ---- blocks of 256, the histograms of a pass ----------------------------------------------------------------------------------
static void blocks_and_histograms() {
    std::vector<RowsetsSet> sets = {set_of(10000), set_of(4000)};
    for (int nq : {256, 257, 600}) {
        std::vector<int32_t> which((size_t)nq);
        std::vector<float> w((size_t)nq);
        for (int q = 0; q < nq; ++q) {
            which[(size_t)q] = q % 3 - 1;
            w[(size_t)q] = (float)(q % 5) * 0.25f;
        }
        const BiasedRowsetsRoute r = biased_rowsets_route(index_of(), sets.data(), 2, which.data(), w.data(), nq, 10, TS_ALGO_MFMA);
        CHECK(r.kind == kBiasedRowsetsSplit && (int)r.pass.size() == nq && r.pass_blocks() == (nq + 255) / 256 && r.classes == 15, "nq %d: blocks %d classes %d",
              nq, r.pass_blocks(), r.classes);
    }
    const int32_t wp[7] = {3, -1, 3, 0, -1, 7, 0};
    std::vector<int32_t> hist_of, hsets;
    CHECK(biased_rowsets_hists(wp, 7, &hist_of, &hsets) == 4, "histograms");
    CHECK(hsets == (std::vector<int32_t>{3, -1, 0, 7}) && hist_of == (std::vector<int32_t>{0, 1, 0, 2, 1, 3, 2}), "numbered by first appearance");
    // the cost formula: bias once for the range, once per group of 16 histograms; each mask once
    CHECK(biased_rowsets_hist_bytes(1000000, 1, 0) == 8000000, "one histogram, no mask");
    CHECK(biased_rowsets_hist_bytes(1000000, 16, 16) == 8000000 + 16 * 125000, "16 sets");
    CHECK(biased_rowsets_hist_bytes(1000000, 17, 16) == 12000000 + 16 * 125000, "17 histograms: two groups");
    CHECK(biased_rowsets_hist_bytes(1000000, 257, 256) == 4000000LL * 18 + 256 * 125000LL, "257 histograms");
    static_assert(kBiasedRowsetsHistGroup * kBiasBins * 4 == 64 * 1024, "a group's histograms take 64 KB of LDS");
    static_assert(sizeof(BiasedRowsetsTable) == sizeof(RowsetsTable) + 8 * kRowsetsBlock, "the table adds a weight and a histogram number per query");
}

// ---- the weight mapping and the solver ----------------------------------------------------------------------------------------
static double identity(double x) { return x; }

// E(t) of the model, summed directly
static double expected(const std::vector<uint32_t>& h, float lo, float width, float hi, float w, double mu, double sigma, double t) {
    return biased_rowsets_expected_share(h.data(), lo, width, hi, w, mu, sigma, t, 0, 1);
}

static void weight_mapping() {
    const float lo = 0.0f, hi = 8.0f, width = (hi - lo) / (float)kBiasBins;
    // the term's upper edge
    CHECK(biased_rowsets_term_edge(0, lo, width, hi, 1.0f) == (double)width, "w = 1: the bin's upper edge");
    CHECK(biased_rowsets_term_edge(kBiasBins - 1, lo, width, hi, 0.5f) == 4.0, "w = 0.5, the last bin: capped at hi");
    CHECK(biased_rowsets_term_edge(5, lo, width, hi, 0.0f) == 0.0, "w = 0");
    CHECK(biased_rowsets_term_edge(0, lo, width, hi, -0.5f) == 0.0, "w < 0: w * the bin's LOWER edge");
    CHECK(biased_rowsets_term_edge(kBiasBins - 1, lo, width, hi, -0.5f) == -0.5 * (8.0 - (double)width), "w < 0, the last bin");
    for (int b = 1; b < kBiasBins; ++b) {
        CHECK(biased_rowsets_term_edge(b, lo, width, hi, 0.25f) >= biased_rowsets_term_edge(b - 1, lo, width, hi, 0.25f), "w > 0 ascends at %d", b);
        CHECK(biased_rowsets_term_edge(b, lo, width, hi, -0.5f) < biased_rowsets_term_edge(b - 1, lo, width, hi, -0.5f), "w < 0 reverses the bins at %d", b);
    }
    // every value of a bin has a term at or below the bin's edge, for either sign
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> u(lo, hi);
    for (int i = 0; i < 20000; ++i) {
        const float v = i == 0 ? lo : i == 1 ? hi : u(rng);
        const int b = bias_bin(v, lo, width);
        for (float w : {0.0f, 0.25f, 1.0f, -0.5f})
            CHECK((double)w * (double)v <= biased_rowsets_term_edge(b, lo, width, hi, w) + 1e-9, "v %g w %g bin %d", (double)v, (double)w, b);
    }

    // a known histogram: a spike at 0, an exponential body, a dozen rows at the top
    std::vector<float> bias;
    std::exponential_distribution<float> ex(1.0f);
    for (int i = 0; i < 200000; ++i) bias.push_back(i % 10 == 0 ? 0.0f : std::min(ex(rng), 7.5f));
    for (int i = 0; i < 12; ++i) bias.push_back(8.0f);
    std::vector<uint32_t> raw((size_t)kBiasBins, 0);
    for (float v : bias) ++raw[(size_t)bias_bin(v, lo, width)];
    const double mu = 0.01, sigma = 0.04, target = 64.0;
    for (float w : {0.0f, 0.25f, 1.0f, -0.5f}) {
        const float t = biased_rowsets_solve_threshold(raw.data(), lo, width, hi, w, mu, sigma, target, 0, 1, identity);
        CHECK(std::isfinite(t), "w %g: solved", (double)w);
        // E(t) = target within the bisection's resolution: the bracket, ((hi - lo) |w| + 18 sigma), halved kBiasBisections times
        // (and the float rounding of t), on either side of the root
        const double res = ((double)(hi - lo) * std::fabs((double)w) + 18.0 * sigma) / (double)(1 << kBiasBisections) + std::fabs((double)t) * 1.2e-7;
        CHECK(expected(raw, lo, width, hi, w, mu, sigma, (double)t - res) >= target, "w %g: E(t - res) = %g", (double)w, expected(raw, lo, width, hi, w, mu, sigma, (double)t - res));
        CHECK(expected(raw, lo, width, hi, w, mu, sigma, (double)t + res) <= target, "w %g: E(t + res) = %g", (double)w, expected(raw, lo, width, hi, w, mu, sigma, (double)t + res));
        // against bias_solve_threshold on the histogram of w * bias built directly (its own range): equal up to one bin width
        // of the raw histogram times |w| (plus the direct histogram's own bin, |w| (hi - lo) / kBiasBins - the same size)
        if (w != 0.0f) {
            const float tlo = std::min(w * lo, w * hi), thi = std::max(w * lo, w * hi), twidth = (thi - tlo) / (float)kBiasBins;
            std::vector<uint32_t> direct((size_t)kBiasBins, 0);
            for (float v : bias) ++direct[(size_t)bias_bin(w * v, tlo, twidth)];
            const float td = bias_solve_threshold(direct.data(), tlo, twidth, thi, mu, sigma, 1.0, target, 0, 1, identity);
            CHECK(std::fabs((double)t - (double)td) <= (double)width * std::fabs((double)w) + 1e-6, "w %g: %g against %g directly", (double)w, (double)t, (double)td);
        } else {
            // w = 0: the plain Gaussian quantile of the rows the histogram counts
            const double z = normal_tail_z(target / (double)bias.size());
            CHECK(std::fabs((double)t - (mu + z * sigma)) <= 1e-6, "w = 0: %g against the quantile %g", (double)t, mu + z * sigma);
        }
    }
    // nothing to estimate from
    std::vector<uint32_t> none((size_t)kBiasBins, 0);
    CHECK(biased_rowsets_solve_threshold(none.data(), lo, width, hi, 0.25f, mu, sigma, target, 0, 1, identity) == -INFINITY, "an empty histogram");
    CHECK(biased_rowsets_solve_threshold(raw.data(), lo, width, hi, 0.25f, mu, 0.0, target, 0, 1, identity) == -INFINITY, "sigma = 0");
    CHECK(biased_rowsets_solve_threshold(raw.data(), INFINITY, 0.0f, -INFINITY, 0.25f, mu, sigma, target, 0, 1, identity) == -INFINITY, "no finite bias");
    // the bins shared between callers sum to the whole
    double parts = 0.0;
    for (int first = 0; first < 256; ++first) parts += biased_rowsets_expected_share(raw.data(), lo, width, hi, -0.5f, mu, sigma, 0.05, first, 256);
    CHECK(std::fabs(parts - expected(raw, lo, width, hi, -0.5f, mu, sigma, 0.05)) <= 1e-6 * parts, "256 callers");
}

int main() {
    refusals();
    classes_and_delegation();
    split();
    blocks_and_histograms();
    weight_mapping();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
