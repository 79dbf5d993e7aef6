// Stand-alone check of theoremsearch_amd/csrc/rowsets_plan.h, the host decisions of ts_search_rowsets (tests/test_rowsets_plan_cpu.py
// builds it with the host compiler under -fsanitize=address,undefined and runs it).  Exit 0 = every check held; otherwise each
// failed check is printed.
#include "rowsets_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
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
    auto args = [](bool q, bool s, bool i, bool sets, bool which, int dt, int nq, int k, int nsets, int algo) {
        return rowsets_args_invalid(q, s, i, sets, which, dt, nq, k, nsets, algo);
    };
    CHECK(args(true, true, true, true, true, TS_F32, 4, 10, 2, TS_ALGO_AUTO) == nullptr, "a valid call");
    CHECK(args(true, true, true, false, true, TS_F32, 4, 10, 0, TS_ALGO_AUTO) == nullptr, "nsets == 0 needs no sets");
    CHECK(args(true, true, true, true, false, TS_F32, 0, 10, 2, TS_ALGO_AUTO) == nullptr, "nq == 0 needs no which");
    CHECK(says(args(true, true, true, true, true, 7, 4, 10, 2, 0), "q_dtype"), "q_dtype");
    CHECK(says(args(true, true, true, true, true, TS_F32, -1, 10, 2, 0), "nq is negative"), "nq");
    for (int k : {0, -3, TS_MAX_K + 1}) CHECK(says(args(true, true, true, true, true, TS_F32, 4, k, 2, 0), "k outside"), "k %d", k);
    CHECK(args(true, true, true, true, true, TS_F32, 4, TS_MAX_K, 2, 0) == nullptr, "k = TS_MAX_K");
    for (int ns : {-1, TS_MAX_ROWSETS + 1}) CHECK(says(args(true, true, true, true, true, TS_F32, 4, 10, ns, 0), "nsets outside"), "nsets %d", ns);
    CHECK(args(true, true, true, true, true, TS_F32, 4, 10, TS_MAX_ROWSETS, 0) == nullptr, "nsets = 256");
    for (int algo : {-1, 3}) CHECK(says(args(true, true, true, true, true, TS_F32, 4, 10, 2, algo), "algo"), "algo %d", algo);
    CHECK(says(args(false, true, true, true, true, TS_F32, 4, 10, 2, 0), "NULL argument"), "queries");
    CHECK(says(args(true, false, true, true, true, TS_F32, 4, 10, 2, 0), "NULL argument"), "scores");
    CHECK(says(args(true, true, false, true, true, TS_F32, 4, 10, 2, 0), "NULL argument"), "idx");
    CHECK(says(args(true, true, true, false, true, TS_F32, 4, 10, 2, 0), "sets is NULL"), "sets");
    CHECK(says(args(true, true, true, true, false, TS_F32, 4, 10, 2, 0), "which is NULL"), "which");
    // the sizes are judged before the pointers
    CHECK(says(args(false, false, false, false, false, TS_F32, 4, 0, 2, 0), "k outside"), "sizes first");

    std::vector<RowsetsSet> sets = {set_of(100), RowsetsSet{false, 0, 0, 0}, set_of(100, kN + 1), set_of(100, kN, 1)};
    auto named = [&](std::vector<int32_t> which, bool has_index = true) {
        return rowsets_sets_invalid(sets.data(), (int)sets.size(), which.data(), (int)which.size(), has_index, kN, 0);
    };
    CHECK(named({0, -1, 0}) == nullptr, "valid");
    CHECK(named({}) == nullptr, "no queries");
    CHECK(says(named({0, 4}), "outside [-1, nsets)"), "which = nsets");
    CHECK(says(named({-2}), "outside [-1, nsets)"), "which = -2");
    CHECK(says(named({0, 1}), "NULL"), "a NULL set that is named");
    CHECK(says(named({2}), "number of rows"), "another n");
    CHECK(says(named({3}), "another device"), "another device");
    CHECK(says(named({0}, false), "NULL argument"), "no index");
    CHECK(says(named({9}, false), "outside [-1, nsets)"), "which is judged before the index");
    // a set nobody names may be anything
    CHECK(named({0, 0, -1}) == nullptr, "unnamed sets are not judged");
}

// ---- the tenth rule --------------------------------------------------------------------------------------------------------
static void tenth_rule() {
    CHECK(rowsets_dense(2000, 20000), "allowed * 10 == n");
    CHECK(!rowsets_dense(1999, 20000), "one row fewer");
    CHECK(rowsets_dense(2001, 20001) && !rowsets_dense(2000, 20001), "n not a multiple of 10");
    CHECK(rowsets_dense(0, 0) && !rowsets_dense(0, 1), "empty");
    // through the routing: a batch of dense queries on two sets, one of them exactly at / just below the rule
    for (int64_t allowed : {2000, 1999}) {
        std::vector<RowsetsSet> sets = {set_of(10000), set_of(allowed)};
        std::vector<int32_t> which(16);
        for (int q = 0; q < 16; ++q) which[q] = q & 1;
        const RowsetsRoute r = rowsets_route(index_of(), sets.data(), 2, which.data(), 16, 10, TS_ALGO_AUTO);
        CHECK(r.kind == kRowsetsSplit, "kind %d", r.kind);
        if (allowed == 2000) CHECK(r.pass.size() == 16 && r.groups.empty(), "pass %zu groups %zu", r.pass.size(), r.groups.size());
        // below the rule only ONE dense set is left: no shared pass at all
        else CHECK(r.pass.empty() && r.groups.size() == 2, "pass %zu groups %zu", r.pass.size(), r.groups.size());
    }
}

// ---- delegation -----------------------------------------------------------------------------------------------------------
static void delegation() {
    std::vector<RowsetsSet> sets = {set_of(10000), set_of(5)};
    for (int algo : {TS_ALGO_AUTO, TS_ALGO_SCAN, TS_ALGO_MFMA}) {
        std::vector<int32_t> one(40, 1), all(40, -1);
        RowsetsRoute r = rowsets_route(index_of(), sets.data(), 2, one.data(), 40, 10, algo);
        CHECK(r.kind == kRowsetsSearchRowset && r.one_set == 1 && r.sets_used == 1 && r.pass.empty() && r.groups.empty(), "one set, algo %d", algo);
        r = rowsets_route(index_of(), sets.data(), 2, all.data(), 40, 10, algo);
        CHECK(r.kind == kRowsetsSearchEx && r.one_set == -1 && r.sets_used == 0 && r.pass.empty() && r.groups.empty(), "all -1, algo %d", algo);
        r = rowsets_route(index_of(), nullptr, 0, all.data(), 40, 10, algo);
        CHECK(r.kind == kRowsetsSearchEx && r.sets_used == 0, "nsets == 0, algo %d", algo);
        r = rowsets_route(index_of(), sets.data(), 2, one.data(), 1, 10, algo);
        CHECK(r.kind == kRowsetsSearchRowset && r.one_set == 1, "one query, algo %d", algo);
    }
}

// the partition a route describes, against the rules restated here
static void check_partition(const RowsetsRoute& r, const std::vector<RowsetsSet>& sets, const std::vector<int32_t>& which, bool pass_expected,
                            const char* what) {
    const int nq = (int)which.size();
    std::vector<int> seen((size_t)nq, 0);
    int prev = -1;
    for (int32_t q : r.pass) {
        CHECK(q > prev && q < nq, "%s: pass order", what);
        prev = q;
        ++seen[(size_t)q];
        const int64_t pop = which[(size_t)q] < 0 ? kN : sets[(size_t)which[(size_t)q]].allowed;
        CHECK(pop * 10 >= kN, "%s: query %d of the pass is sparse", what, q);
    }
    int prev_set = -2, calls = 0, scanq = 0;
    for (const RowsetsGroup& g : r.groups) {
        CHECK(g.set > prev_set, "%s: groups by set", what);
        prev_set = g.set;
        CHECK(!g.queries.empty(), "%s: an empty group", what);
        CHECK(g.empty == (g.set >= 0 && sets[(size_t)g.set].allowed == 0), "%s: empty flag of set %d", what, g.set);
        calls += g.empty ? 0 : 1;
        int pq = -1;
        for (int32_t q : g.queries) {
            CHECK(q > pq && q < nq && which[(size_t)q] == g.set, "%s: group of set %d holds query %d", what, g.set, q);
            pq = q;
            ++seen[(size_t)q];
            ++scanq;
        }
    }
    for (int q = 0; q < nq; ++q) CHECK(seen[(size_t)q] == 1, "%s: query %d answered %d times", what, q, seen[(size_t)q]);
    CHECK(r.scan_queries() == scanq && r.scan_calls() == calls, "%s: counters", what);
    CHECK(r.pass.empty() == !pass_expected, "%s: pass of %zu queries", what, r.pass.size());
    if (pass_expected)
        for (int q = 0; q < nq; ++q) {
            const int64_t pop = which[(size_t)q] < 0 ? kN : sets[(size_t)which[(size_t)q]].allowed;
            CHECK((pop * 10 >= kN) == (std::find(r.pass.begin(), r.pass.end(), q) != r.pass.end()), "%s: query %d", what, q);
        }
    std::set<int32_t> named;
    for (int32_t s : which)
        if (s >= 0) named.insert(s);
    CHECK(r.sets_used == (int)named.size(), "%s: sets_used %d", what, r.sets_used);
}

// ---- mixed batches ---------------------------------------------------------------------------------------------------------
static void mixed() {
    // dense 0.5, sparse 0.05, empty, and -1 as a set of its own
    const std::vector<RowsetsSet> sets = {set_of(10000), set_of(1000), set_of(0), set_of(18000), RowsetsSet{false, 0, 0, 0}};
    std::mt19937 rng(7);
    for (int trial = 0; trial < 50; ++trial) {
        const int nq = 2 + (int)(rng() % 600);
        std::vector<int32_t> which((size_t)nq);
        for (auto& w : which) w = (int32_t)(rng() % 5) - 1;            // -1 .. 3
        if (std::set<int32_t>(which.begin(), which.end()).size() < 2) continue;
        int eligible = 0;
        std::set<int32_t> dense_sets;
        for (int32_t w : which)
            if (w == -1 || w == 0 || w == 3) { ++eligible; dense_sets.insert(w); }
        for (int k : {10, 64, 65, 200}) {
            const int limit = k > 64 ? 1 : 4;
            const bool pass = eligible > limit && dense_sets.size() >= 2;
            const RowsetsRoute r = rowsets_route(index_of(), sets.data(), 5, which.data(), nq, k, TS_ALGO_AUTO);
            CHECK(r.kind == kRowsetsSplit && r.group_algo == TS_ALGO_AUTO, "kind %d", r.kind);
            check_partition(r, sets, which, pass, "auto");
            CHECK(r.pass_blocks() == ((int)r.pass.size() + 255) / 256, "blocks");
            // the scan hint: no pass, every group on the scan
            const RowsetsRoute s = rowsets_route(index_of(), sets.data(), 5, which.data(), nq, k, TS_ALGO_SCAN);
            CHECK(s.kind == kRowsetsSplit && s.group_algo == TS_ALGO_SCAN, "scan kind %d", s.kind);
            check_partition(s, sets, which, false, "scan");
        }
    }
    // -1 counts as a set: 8 queries on one dense set and 8 unfiltered ride together
    {
        std::vector<int32_t> which(16, 0);
        for (int q = 8; q < 16; ++q) which[(size_t)q] = -1;
        const RowsetsRoute r = rowsets_route(index_of(), sets.data(), 5, which.data(), 16, 10, TS_ALGO_AUTO);
        CHECK(r.pass.size() == 16 && r.groups.empty() && r.sets_used == 1, "pass %zu", r.pass.size());
    }
    // a small remainder: 4 dense queries (bf16: the scan's limit) on two sets stay off the pass, 5 ride
    for (int dense : {4, 5}) {
        std::vector<int32_t> which;
        for (int q = 0; q < dense; ++q) which.push_back(q & 1 ? 0 : 3);
        for (int q = 0; q < 7; ++q) which.push_back(1);
        const RowsetsRoute r = rowsets_route(index_of(), sets.data(), 5, which.data(), (int)which.size(), 10, TS_ALGO_AUTO);
        CHECK((int)r.pass.size() == (dense == 5 ? 5 : 0), "dense %d: pass %zu", dense, r.pass.size());
        CHECK((int)r.groups.size() == (dense == 5 ? 1 : 3), "dense %d: groups %zu", dense, r.groups.size());
    }
    // fp32: the limit is 8
    {
        std::vector<int32_t> which;
        for (int q = 0; q < 8; ++q) which.push_back(q & 1 ? 0 : 3);
        RowsetsRoute r = rowsets_route(index_of(TS_F32, 128), sets.data(), 5, which.data(), 8, 10, TS_ALGO_AUTO);
        CHECK(r.pass.empty(), "fp32, 8 queries");
        which.push_back(0);
        r = rowsets_route(index_of(TS_F32, 128), sets.data(), 5, which.data(), 9, 10, TS_ALGO_AUTO);
        CHECK(r.pass.size() == 9, "fp32, 9 queries");
        r = rowsets_route(index_of(TS_F32, 128), sets.data(), 5, which.data(), 2, 200, TS_ALGO_AUTO);
        CHECK(r.pass.size() == 2, "fp32, k = 200: more than one query");
    }
    // what the pass does not serve: every query to its set's group
    std::vector<int32_t> which(64);
    for (int q = 0; q < 64; ++q) which[(size_t)q] = q % 3 == 0 ? -1 : (q % 3 == 1 ? 0 : 3);
    auto groups_only = [&](RowsetsIndex ix, const char* what) {
        const RowsetsRoute r = rowsets_route(ix, sets.data(), 5, which.data(), 64, 10, TS_ALGO_AUTO);
        CHECK(r.kind == kRowsetsSplit && r.pass.empty() && r.groups.size() == 3 && r.scan_queries() == 64 && r.scan_calls() == 3, "%s", what);
        const RowsetsRoute m = rowsets_route(ix, sets.data(), 5, which.data(), 64, 10, TS_ALGO_MFMA);
        CHECK(m.kind == kRowsetsUnsupported && says(m.unsupported, "TS_ALGO_MFMA"), "%s under mfma", what);
    };
    CHECK(rowsets_route(index_of(), sets.data(), 5, which.data(), 64, 10, TS_ALGO_AUTO).pass.size() == 64, "served");
    for (int d : {128, 192, 384, 512, 768, 1024, 2048}) CHECK(rowsets_pass_served(index_of(TS_BF16, d)), "bf16 d = %d", d);
    for (int d : {128, 768, 1024}) CHECK(rowsets_pass_served(index_of(TS_F32, d)), "fp32 d = %d", d);
    groups_only(index_of(TS_BF16, 2304), "a k-chunked width");
    groups_only(index_of(TS_BF16, 96), "a width that is no multiple of 64");
    groups_only(index_of(TS_BF16, 64), "below 128");
    groups_only(index_of(TS_F32, 1088), "an fp32 row above 4,096 bytes");
    groups_only(index_of(2, 768), "another storage type");
    { RowsetsIndex ix = index_of(); ix.n = 16383; groups_only(ix, "below TS_MFMA_MIN_ROWS"); }
    { RowsetsIndex ix = index_of(); ix.two_level = false; groups_only(ix, "not the two-level search"); }
    { RowsetsIndex ix = index_of(); ix.unpadded = false; groups_only(ix, "padded rows"); }
    { RowsetsIndex ix = index_of(TS_F32, 768); ix.f32_matrix = false; groups_only(ix, "TS_MFMA_F32=0"); }
    { RowsetsIndex ix = index_of(); ix.scan_max_knob = 64; groups_only(ix, "TS_SCAN_MAX_QUERIES at the batch"); }
}

// ---- TS_ALGO_MFMA ----------------------------------------------------------------------------------------------------------
static void mfma_hint() {
    const std::vector<RowsetsSet> sets = {set_of(10000), set_of(1000), set_of(0), set_of(18000)};
    std::vector<int32_t> which(32);
    for (int q = 0; q < 32; ++q) which[(size_t)q] = q & 1 ? 0 : 3;
    RowsetsRoute r = rowsets_route(index_of(), sets.data(), 4, which.data(), 32, 10, TS_ALGO_MFMA);
    CHECK(r.kind == kRowsetsSplit && r.pass.size() == 32 && r.groups.empty(), "every query rides");
    which[5] = 1;       // one sparse query
    r = rowsets_route(index_of(), sets.data(), 4, which.data(), 32, 10, TS_ALGO_MFMA);
    CHECK(r.kind == kRowsetsUnsupported && says(r.unsupported, "TS_ALGO_MFMA"), "a sparse query");
    which[5] = 2;       // an empty set
    r = rowsets_route(index_of(), sets.data(), 4, which.data(), 32, 10, TS_ALGO_MFMA);
    CHECK(r.kind == kRowsetsUnsupported, "an empty set");
    // too few queries for the pass
    std::vector<int32_t> few = {0, 3, 0, 3};
    r = rowsets_route(index_of(), sets.data(), 4, few.data(), 4, 10, TS_ALGO_MFMA);
    CHECK(r.kind == kRowsetsUnsupported, "four queries");
    CHECK(rowsets_route(index_of(), sets.data(), 4, few.data(), 4, 10, TS_ALGO_AUTO).pass.empty(), "four queries under auto");
}

// ---- blocks of 256 ---------------------------------------------------------------------------------------------------------
static void blocks() {
    const std::vector<RowsetsSet> sets = {set_of(10000), set_of(18000), set_of(3000)};
    for (int nq : {2, 255, 256, 257, 300, 512, 513, 1000}) {
        std::vector<int32_t> which((size_t)nq);
        for (int q = 0; q < nq; ++q) which[(size_t)q] = q % 3;
        const RowsetsRoute r = rowsets_route(index_of(), sets.data(), 3, which.data(), nq, 10, TS_ALGO_AUTO);
        const bool pass = nq > 4;
        CHECK((int)r.pass.size() == (pass ? nq : 0), "nq %d: pass %zu", nq, r.pass.size());
        CHECK(r.pass_blocks() == (pass ? (nq + 255) / 256 : 0), "nq %d: blocks %d", nq, r.pass_blocks());
    }
    CHECK(kRowsetsBlock == 256 && TS_MAX_ROWSETS == 256, "the block");
    CHECK(sizeof(RowsetsTable) == 256 * (sizeof(void*) + 5 * 4), "the table: %zu bytes", sizeof(RowsetsTable));
}

// ---- the per-query numbers -------------------------------------------------------------------------------------------------
// the quantile by bisection on erfc, independent of the rational approximation
static double tail_z_bisect(double p) {
    if (p >= 0.5) return 0.0;
    double lo = 0.0, hi = 40.0;
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (0.5 * std::erfc(mid / std::sqrt(2.0)) > p) lo = mid;
        else hi = mid;
    }
    return 0.5 * (lo + hi);
}

static void numbers() {
    for (double p : {0.25, 0.1, 0.02425, 0.0242, 1e-3, 3.2e-6, 1e-9})
        CHECK(std::fabs(normal_tail_z(p) - tail_z_bisect(p)) < 1e-7, "p %g: %.12g against %.12g", p, normal_tail_z(p), tail_z_bisect(p));
    CHECK(normal_tail_z(0.0) == 8.0 && normal_tail_z(0.5) == 0.0 && normal_tail_z(0.7) == 0.0, "the ends");
    constexpr int kCap = 8192;
    for (int64_t n : {20000ll, 1000000ll, 10000000ll, 50000000ll})
        for (int k : {1, 10, 64, 200}) {
            const int kk = k;
            const int stat_cands = std::min(2048, std::max(2 * kk, std::max(64, 6 * kk)));
            // the sample as the plan makes it: the smallest power-of-two tile stride that leaves at most first_rows rows
            const int64_t first_rows = n < 4000000 ? 4096 : 8192, T = (n + 31) / 32;
            int64_t stride = 2;
            while (((T + stride - 1) / stride) * 32 > first_rows) stride *= 2;
            const double sample_rows = (double)(((T + stride - 1) / stride) * 32);
            for (int64_t pop : {n, n / 2, n / 10, (int64_t)5, (int64_t)1}) {
                const RowsetsNumbers r = rowsets_numbers(pop, n, k, kk, stat_cands, sample_rows, kCap, true, true);
                // independently: the quantile by bisection, the rule restated
                const double pz = std::min(0.25, (double)stat_cands / (double)pop);
                CHECK(std::fabs((double)r.z_tail - tail_z_bisect(pz)) < 1e-6, "n %lld k %d pop %lld: z_tail %.9g against %.9g", (long long)n, k,
                      (long long)pop, (double)r.z_tail, tail_z_bisect(pz));
                const bool swamps = (double)kk * (double)n / sample_rows > 4096.0;
                const float tail_p = (pz < 0.5 && r.z_tail > 0.0f && swamps) ? (float)std::min(0.25, (double)std::max(2048, 8 * kk) / (double)pop) : 0.0f;
                CHECK(r.tail_p == tail_p, "n %lld k %d pop %lld: tail_p %g against %g", (long long)n, k, (long long)pop, (double)r.tail_p, (double)tail_p);
                CHECK(r.min_fill == (int32_t)std::min<int64_t>(k, pop), "n %lld k %d pop %lld: min_fill %d", (long long)n, k, (long long)pop, r.min_fill);
                CHECK(rowsets_numbers(pop, n, k, kk, stat_cands, sample_rows, kCap, true, false).tail_p == 0.0f, "TS_MFMA_TAIL_FIT=0");
                const RowsetsNumbers off = rowsets_numbers(pop, n, k, kk, stat_cands, sample_rows, kCap, false, true);
                CHECK(off.z_tail == 0.0f && off.tail_p == 0.0f && off.min_fill == r.min_fill, "no estimate");
                // a sparser set: a higher exceedance probability, a lower quantile, never a larger min_fill
                const RowsetsNumbers whole = rowsets_numbers(n, n, k, kk, stat_cands, sample_rows, kCap, true, true);
                CHECK(r.z_tail <= whole.z_tail && r.min_fill <= whole.min_fill, "monotone in pop");
                const float z_sel = rowsets_z_sel(pop, n, kk, r.tail_p, sample_rows);
                const int kl = r.tail_p > 0.0f ? std::max(kk, 32) : kk;
                const double live = std::max(sample_rows * (double)pop / (double)n, 1.0);
                CHECK(std::fabs((double)z_sel - tail_z_bisect(std::min(0.25, 2.0 * kl / live))) < 1e-6, "z_sel");
            }
            // pop = n: exactly the scalar formulas of the search behind one mask (search_mfma.hip: mfma_plan / mfma_sample)
            const RowsetsNumbers r = rowsets_numbers(n, n, k, kk, stat_cands, sample_rows, kCap, true, true);
            const float z_tail = (float)normal_tail_z(std::min(0.25, (double)stat_cands / (double)std::max<int64_t>(n, 1)));
            const bool bound_swamps = (double)kk * (double)n / sample_rows > 0.5 * kCap;
            const float tail_p = (z_tail > 0.0f && bound_swamps) ? (float)std::min(0.25, (double)std::max(2048, 8 * kk) / (double)std::max<int64_t>(n, 1)) : 0.0f;
            CHECK(memcmp(&r.z_tail, &z_tail, 4) == 0 && memcmp(&r.tail_p, &tail_p, 4) == 0 && r.min_fill == (int)std::min<int64_t>(k, n),
                  "n %lld k %d: the scalar formulas", (long long)n, k);
            const int kl = tail_p > 0.0f ? std::max(kk, 32) : kk;
            const float z_sel = (float)normal_tail_z(std::min(0.25, 2.0 * kl / std::max(sample_rows * (double)n / (double)std::max<int64_t>(n, 1), 1.0)));
            const float got = rowsets_z_sel(n, n, kk, tail_p, sample_rows);
            CHECK(memcmp(&got, &z_sel, 4) == 0, "n %lld k %d: z_sel", (long long)n, k);
        }
    // an empty set never reaches the pass, but its numbers are defined
    const RowsetsNumbers e = rowsets_numbers(0, 20000, 10, 10, 64, 4096.0, kCap, true, true);
    CHECK(e.min_fill == 0 && e.z_tail == (float)normal_tail_z(0.25), "pop = 0");
}

int main() {
    refusals();
    tenth_rule();
    delegation();
    mixed();
    mfma_hint();
    blocks();
    numbers();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("rowsets_plan.h: all checks passed\n");
    return 0;
}
