// Stand-alone check of theoremsearch_amd/csrc/bias_plan.h, the biased matrix search's host decisions and threshold solver
// (tests/test_bias_plan_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it).
//   bias_plan_check          walks the served / refused table and the AUTO rule; exit 0 = every check held
//   bias_plan_check solve    reads problems from stdin, one per line -
//                                lo hi mu sigma scale target nbins_set  then nbins_set pairs  bin count
//                            - and prints bias_solve_threshold()'s answer for each (%.9g; "-inf" for none)
#include "bias_plan.h"

#include <cstdio>
#include <cstring>
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

static void served_set() {
    for (int dtype : {TS_F32, TS_BF16}) {
        const int elem = dtype == TS_BF16 ? 2 : 4;
        int widest = 0, count = 0;
        for (int d = 1; d <= 4096; ++d) {
            const bool want = d % 64 == 0 && d >= 128 && d * elem <= 4096;
            CHECK(bias_served(dtype, d, true) == want, "dtype %d d %d", dtype, d);
            CHECK(!bias_served(dtype, d, false), "dtype %d d %d without the two-level search", dtype, d);
            // everything the plain general-width pass serves, and the four hand-laid widths on top
            if (anyd_served(dtype, d, true)) CHECK(bias_served(dtype, d, true), "dtype %d d %d", dtype, d);
            if (bias_served(dtype, d, true)) { widest = d; ++count; }
        }
        CHECK(widest == (dtype == TS_BF16 ? 2048 : 1024), "dtype %d widest %d", dtype, widest);
        CHECK(count == (dtype == TS_BF16 ? 31 : 15), "dtype %d count %d", dtype, count);
        for (int d : {384, 512, 768, 1024}) CHECK(bias_served(dtype, d, true) && !anyd_served(dtype, d, true), "dtype %d d %d", dtype, d);
        for (int d : {64, 0, -64, 200, 100, 1000}) CHECK(!bias_served(dtype, d, true), "dtype %d d %d", dtype, d);
        // the staging tile of every served width fits the launch the general-width kernel is given
        for (int d = 128; d <= 2048; d += 64)
            if (bias_served(dtype, d, true)) CHECK(anyd_lds_bytes(anyd_row_bytes(dtype, d)) <= kAnydLdsMax, "dtype %d d %d", dtype, d);
    }
    CHECK(!bias_served(TS_BF16, 2112, true) && !bias_served(TS_F32, 1088, true), "row limit");
    CHECK(!bias_served(7, 192, true) && !bias_served(-1, 192, true), "unknown storage types");
}

static AlgoInputs call(int algo, int64_t n, int nq, int k) {
    AlgoInputs in;
    memset(&in, 0, sizeof(in));
    in.algo = algo;
    in.mfma_ok = false;          // not read: `served` replaces it
    in.n = n;
    in.nq = nq;
    in.k = k;
    in.mfma_min_rows = 16384;
    in.scan_max_queries = kBiasScanMaxQueries;
    in.bias = true;
    return in;
}

static void algo_rule() {
    // SCAN is always the scan; a subset index is refused whatever the hint
    for (int algo : {TS_ALGO_AUTO, TS_ALGO_SCAN, TS_ALGO_MFMA})
        for (bool served : {false, true}) {
            AlgoInputs in = call(algo, 100000, 40, 10);
            in.subset = true;
            CHECK(choose_bias_algo(in, served).unsupported != nullptr, "algo %d served %d", algo, (int)served);
            in.subset = false;
            if (algo == TS_ALGO_SCAN) {
                const AlgoChoice c = choose_bias_algo(in, served);
                CHECK(!c.unsupported && c.algo == TS_ALGO_SCAN, "served %d", (int)served);
            }
        }
    // MFMA: served or refused; any batch size and any corpus size
    for (int nq : {1, 4, 5, 256, 1000})
        for (int64_t n : {(int64_t)1, (int64_t)16383, (int64_t)10000000}) {
            const AlgoChoice c = choose_bias_algo(call(TS_ALGO_MFMA, n, nq, 10), true);
            CHECK(!c.unsupported && c.algo == TS_ALGO_MFMA, "nq %d n %lld", nq, (long long)n);
            CHECK(choose_bias_algo(call(TS_ALGO_MFMA, n, nq, 10), false).unsupported != nullptr, "nq %d n %lld", nq, (long long)n);
        }
    // AUTO: above the scan limit (4; 1 for k > 64), over at least mfma_min_rows rows, where served
    CHECK(bias_scan_max_queries(TS_BF16) == 4 && bias_scan_max_queries(TS_F32) == 8, "the AUTO limits");
    for (int dtype : {TS_BF16, TS_F32})
        for (int k : {1, 10, 64, 65, 256})
            for (int nq = 1; nq <= 300; ++nq)
                for (int64_t n : {(int64_t)16383, (int64_t)16384, (int64_t)1000000}) {
                    const int limit = k > 64 ? 1 : (dtype == TS_F32 ? 8 : 4);
                    const int want = (nq > limit && n >= 16384) ? TS_ALGO_MFMA : TS_ALGO_SCAN;
                    AlgoInputs in = call(TS_ALGO_AUTO, n, nq, k);
                    in.scan_max_queries = bias_scan_max_queries(dtype);
                    const AlgoChoice c = choose_bias_algo(in, true);
                    CHECK(!c.unsupported && c.algo == want, "dtype %d k %d nq %d n %lld -> %d", dtype, k, nq, (long long)n, c.algo);
                    const AlgoChoice u = choose_bias_algo(in, false);
                    CHECK(!u.unsupported && u.algo == TS_ALGO_SCAN, "dtype %d k %d nq %d n %lld", dtype, k, nq, (long long)n);
                }
    // masks: the filtered search's rule - a host mask that keeps at least a tenth of the rows, in front of a matrix batch
    for (int algo : {TS_ALGO_AUTO, TS_ALGO_MFMA}) {
        AlgoInputs in = call(algo, 100000, 40, 10);
        in.mask = true;
        CHECK(mask_wants_count(bias_algo_inputs(in, true)) && !mask_wants_count(bias_algo_inputs(in, false)), "algo %d", algo);
        CHECK(!mask_wants_count(in), "choose_algo's own rule never counts for a biased call");
        in.allowed = 10000;
        AlgoChoice c = choose_bias_algo(in, true);
        CHECK(!c.unsupported && c.algo == TS_ALGO_MFMA, "algo %d: a tenth of the rows", algo);
        in.allowed = 9999;
        c = choose_bias_algo(in, true);
        if (algo == TS_ALGO_MFMA) CHECK(c.unsupported != nullptr, "too sparse a mask under MFMA");
        else CHECK(!c.unsupported && c.algo == TS_ALGO_SCAN, "too sparse a mask under AUTO");
        in.allowed = 50000;
        in.mask_on_device = true;
        CHECK(!mask_wants_count(bias_algo_inputs(in, true)), "a device mask is not counted");
        c = choose_bias_algo(in, true);
        if (algo == TS_ALGO_MFMA) CHECK(c.unsupported != nullptr, "a device mask under MFMA");
        else CHECK(!c.unsupported && c.algo == TS_ALGO_SCAN, "a device mask under AUTO");
        // a masked batch the matrix path does not take (4 queries): MFMA refused, AUTO scans
        AlgoInputs few = call(algo, 100000, 4, 10);
        few.mask = true;
        few.allowed = 90000;
        c = choose_bias_algo(few, true);
        if (algo == TS_ALGO_MFMA) CHECK(c.unsupported != nullptr, "a masked batch of 4 under MFMA");
        else CHECK(!c.unsupported && c.algo == TS_ALGO_SCAN, "a masked batch of 4 under AUTO");
    }
}

static double identity(double x) { return x; }

static void solver_edges() {
    std::vector<uint32_t> h(kBiasBins, 0);
    // nothing to estimate from
    CHECK(bias_solve_threshold(h.data(), 0.f, 0.f, 0.f, 0.0, 0.0, 8.0, 64.0, 0, 1, identity) == -INFINITY, "sigma 0");
    CHECK(bias_solve_threshold(h.data(), 0.f, 0.f, 0.f, 0.0, 1.0, 8.0, 64.0, 0, 1, identity) == -INFINITY, "empty histogram");
    CHECK(bias_solve_threshold(h.data(), INFINITY, 0.f, -INFINITY, 0.0, 1.0, 8.0, 64.0, 0, 1, identity) == -INFINITY, "no finite term");
    // all terms equal (width 0): a plain Gaussian shifted by the term - 1,000 sample rows standing for 1e6, 100 wanted:
    // Q(z) = 1e-4 at z = 3.719
    h[0] = 1000;
    const float t = bias_solve_threshold(h.data(), 0.25f, 0.f, 0.25f, 1.0, 2.0, 1000.0, 100.0, 0, 1, identity);
    CHECK(std::fabs((double)t - (1.0 + 0.25 + 2.0 * 3.71902)) < 1e-3, "t = %.6f", (double)t);
    // fewer rows than the target: no threshold
    CHECK(bias_solve_threshold(h.data(), 0.25f, 0.f, 0.25f, 1.0, 2.0, 0.05, 100.0, 0, 1, identity) == -INFINITY, "target above the population");
    // shared bins: two callers' shares add up to the one caller's sum
    for (int b = 0; b < kBiasBins; ++b) h[b] = (uint32_t)(b % 7);
    const double whole = bias_expected_share(h.data(), 0.f, 0.001f, 1.024f, 0.0, 0.05, 0.9, 0, 1);
    const double halves = bias_expected_share(h.data(), 0.f, 0.001f, 1.024f, 0.0, 0.05, 0.9, 0, 2) +
                          bias_expected_share(h.data(), 0.f, 0.001f, 1.024f, 0.0, 0.05, 0.9, 1, 2);
    CHECK(std::fabs(whole - halves) <= 1e-12 * whole && whole > 0.0, "%.17g against %.17g", whole, halves);
    // bins: every value of [lo, hi] lands in [0, kBiasBins), its bin's upper edge is at or above it
    const float lo = -0.3f, hi = 0.7f, width = (hi - lo) / (float)kBiasBins;
    for (int i = 0; i <= 5000; ++i) {
        const float v = lo + (hi - lo) * (float)i / 5000.f;
        const int b = bias_bin(v, lo, width);
        CHECK(b >= 0 && b < kBiasBins, "v %.6f bin %d", (double)v, b);
        CHECK(bias_bin_edge(b, lo, width, hi) >= (double)v - 1e-6, "v %.6f bin %d edge %.6f", (double)v, b, bias_bin_edge(b, lo, width, hi));
    }
    CHECK(bias_bin(5.f, 5.f, 0.f) == 0 && bias_bin_edge(0, 5.f, 0.f, 5.f) == 5.0, "width 0");
}

static int solve_stdin() {
    std::vector<uint32_t> h(kBiasBins);
    for (;;) {
        double lo, hi, mu, sigma, scale, target;
        int nset;
        if (scanf("%lf %lf %lf %lf %lf %lf %d", &lo, &hi, &mu, &sigma, &scale, &target, &nset) != 7) break;
        std::fill(h.begin(), h.end(), 0u);
        for (int i = 0; i < nset; ++i) {
            int b;
            unsigned c;
            if (scanf("%d %u", &b, &c) != 2 || b < 0 || b >= kBiasBins) return 2;
            h[(size_t)b] = c;
        }
        const float flo = (float)lo, fhi = (float)hi;
        const float width = fhi > flo ? (fhi - flo) / (float)kBiasBins : 0.0f;
        const float t = bias_solve_threshold(h.data(), flo, width, fhi, mu, sigma, scale, target, 0, 1, identity);
        if (std::isinf(t)) printf("-inf\n");
        else printf("%.9g\n", (double)t);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "solve") == 0) return solve_stdin();
    served_set();
    algo_rule();
    solver_edges();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
