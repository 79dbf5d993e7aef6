// Stand-alone check of theoremsearch_amd/csrc/scan_plan.h, the scan path's host decisions (tests/test_scan_plan_cpu.py builds
// it with the host compiler under -fsanitize=address,undefined and runs it).  Exit 0 = every check held; otherwise each
// failed check is printed.  Expected values are literals here: what search.hip launched before the decisions moved.
#include "scan_plan.h"

#include <cmath>
#include <cstdio>
#include <limits>
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

static void width_table() {
    const ScanWidth want[8] = {{TS_F32, 768, 3, 64},  {TS_F32, 1024, 4, 64}, {TS_BF16, 768, 3, 32}, {TS_BF16, 1024, 2, 64},
                               {TS_F32, 384, 3, 32},  {TS_BF16, 384, 3, 16}, {TS_F32, 512, 2, 64},  {TS_BF16, 512, 2, 32}};
    CHECK(kScanWidths == 8, "%d", kScanWidths);
    for (const ScanWidth& w : want) {
        const int i = scan_width(w.dtype, w.ld);
        CHECK(i >= 0 && i < kScanWidths, "dtype %d ld %d", w.dtype, w.ld);
        if (i < 0) continue;
        CHECK(kScanWidth[i].ch == w.ch && kScanWidth[i].g == w.g, "dtype %d ld %d: CH %d G %d", w.dtype, w.ld, kScanWidth[i].ch, kScanWidth[i].g);
        CHECK(kScanWidth[i].ch * kScanWidth[i].g * 16 == w.ld * (w.dtype == TS_BF16 ? 2 : 4), "dtype %d ld %d", w.dtype, w.ld);
    }
    for (int dtype : {TS_F32, TS_BF16})
        for (int64_t ld : {64, 128, 256 /* d = 200 padded */, 2048, 8256})
            CHECK(scan_width(dtype, ld) == -1, "dtype %d ld %lld", dtype, (long long)ld);
    // the generic form: four queries per pass only while ld <= 8192 and (k <= 64 or EMIT)
    for (int64_t ld : {64, 256, 8192, 8256, 16384})
        for (int k : {1, 64, 65, 256})
            for (bool emit : {false, true}) {
                const int want4 = (ld <= 8192 && (k <= 64 || emit)) ? 4 : 1;
                CHECK(scan_generic_qb(4, ld, scan_kr(k), emit) == want4, "ld %lld k %d emit %d", (long long)ld, k, emit);
                CHECK(scan_generic_qb(1, ld, scan_kr(k), emit) == 1, "ld %lld k %d emit %d", (long long)ld, k, emit);
            }
    CHECK(scan_generic_lds(200, 1) == 8192 + 800 && scan_generic_lds(200, 4) == 8192 + 3200, "%d", scan_generic_lds(200, 4));
    CHECK(rank_generic_lds(200) == 800, "%d", rank_generic_lds(200));
}

static void pass_shape() {
    auto is = [](ScanPass p, int grid, int kr, int qb) { return p.grid == grid && p.kr == kr && p.qb == qb; };
    CHECK(is(scan_pass(256, 1000000, TS_F32, 768, 1, 10, false), 1024, 1, 1), "single query");
    CHECK(is(scan_pass(256, 1000000, TS_F32, 768, 2, 64, false), 1024, 1, 4), "two queries");
    CHECK(is(scan_pass(256, 1000000, TS_F32, 768, 4, 65, false), 1024, 4, 4), "k = 65");
    // wide_k_one_wave: bf16 at 768 / 384 and k > 64 takes one query per pass
    CHECK(is(scan_pass(256, 1000000, TS_BF16, 768, 8, 200, false), 1024, 4, 1), "bf16 768 k 200");
    CHECK(is(scan_pass(256, 1000000, TS_BF16, 384, 8, 65, false), 1024, 4, 1), "bf16 384 k 65");
    CHECK(is(scan_pass(256, 1000000, TS_BF16, 768, 8, 64, false), 1024, 1, 4), "bf16 768 k 64");
    CHECK(is(scan_pass(256, 1000000, TS_BF16, 1024, 8, 200, false), 1024, 4, 4), "bf16 1024 k 200");
    CHECK(is(scan_pass(256, 1000000, TS_F32, 384, 8, 200, false), 1024, 4, 4), "f32 384 k 200");
    // the small-corpus clamp: k > 64 and n <= 16384
    CHECK(is(scan_pass(256, 5000, TS_F32, 768, 1, 200, false), 61, 4, 1), "n 5000 k 200");
    CHECK(is(scan_pass(256, 16384, TS_F32, 768, 1, 256, false), 48, 4, 1), "n 16384 k 256");
    CHECK(is(scan_pass(256, 16385, TS_F32, 768, 1, 256, false), 1024, 4, 1), "n 16385 k 256");
    CHECK(is(scan_pass(256, 5000, TS_F32, 768, 1, 64, false), 1024, 1, 1), "n 5000 k 64");
    CHECK(is(scan_pass(1, 5000, TS_F32, 768, 1, 256, false), 4, 4, 1), "1 CU");
    CHECK(scan_grid(8, 5000, 65) == 32 && scan_grid(256, 5000, 65) == 189, "%d", scan_grid(256, 5000, 65));
    // the matrix path's re-run: one workgroup per CU, four queries per pass even for one slot
    CHECK(is(scan_pass(256, 1000000, TS_F32, 768, 1, 10, true), 256, 1, 4), "re-run");
    CHECK(is(scan_pass(256, 5000, TS_F32, 768, 1, 200, true), 61, 4, 4), "re-run, small corpus");
    CHECK(is(scan_pass(256, 1000000, TS_BF16, 768, 1, 200, true), 256, 4, 1), "re-run, bf16 768 k 200");
}

static const int kCUs[] = {8, 16, 32, 64, 80, 96, 104, 120, 128, 256, 304};

static void select_plans_and_scratch() {
    int most_rounds = 0;
    for (int cu : kCUs)
        for (int k = 1; k <= 256; ++k) {
            const ScanScratch have = scan_scratch(cu, k);
            const int full = cu * 4;
            const size_t todays_partial2 = (size_t)32 * full * k + 4096;
            if (cu >= 128) CHECK(have.partial2 <= todays_partial2, "cu %d k %d: %zu keys", cu, k, have.partial2);
            CHECK(have.partial2 >= todays_partial2 && have.partial == (size_t)256 * full * k, "cu %d k %d", cu, k);
            for (int grid : {full, scan_grid(cu, 16384, k)}) {
                const SelectPlan p = select_plan(grid * k, k);
                CHECK(p.nrounds >= 0 && p.nrounds <= kSelectMaxRounds, "cu %d k %d grid %d: %d rounds", cu, k, grid, p.nrounds);
                if (p.nrounds < 0) continue;
                most_rounds = std::max(most_rounds, p.nrounds);
                CHECK((size_t)256 * grid * k <= have.partial, "cu %d k %d grid %d: the scan's lists", cu, k, grid);
                int m = grid * k;
                for (int r = 0; r < p.nrounds; ++r) {
                    const SelectRound& rd = p.round[r];
                    CHECK(rd.seg == 1024 || rd.seg == 4096, "cu %d k %d round %d: seg %d", cu, k, r, rd.seg);
                    // the segments cover the previous output, and no more than it
                    CHECK((int64_t)rd.nseg * rd.seg >= m && (int64_t)(rd.nseg - 1) * rd.seg < m, "cu %d k %d round %d: %d x %d over %d", cu, k, r, rd.nseg, rd.seg, m);
                    CHECK(rd.out == rd.nseg * k && rd.out < m, "cu %d k %d round %d: out %d of %d", cu, k, r, rd.out, m);
                    const size_t room = (r & 1) ? have.partial : have.partial2;
                    CHECK((size_t)256 * rd.out <= room, "cu %d k %d grid %d round %d: %zu keys into %zu", cu, k, grid, r, (size_t)256 * rd.out, room);
                    m = rd.out;
                }
                CHECK(p.final_m == m, "cu %d k %d: final reads %d of %d", cu, k, p.final_m, m);
                if (p.final_form == kSelectHist) {
                    CHECK(m > 1024 && m <= 12288, "cu %d k %d: histogram over %d", cu, k, m);
                    CHECK(p.hist_kr == (k <= 64 ? 1 : 4), "cu %d k %d: KR %d", cu, k, p.hist_kr);
                } else if (p.final_form == kSelectSort1024) {
                    CHECK(m <= 1024, "cu %d k %d: <1024> over %d", cu, k, m);
                } else {
                    CHECK(p.final_form == kSelectSort4096 && m <= 4096 && k > 64, "cu %d k %d: <4096> over %d", cu, k, m);
                }
            }
        }
    CHECK(most_rounds == 2, "%d", most_rounds);
    // the formula `partial2` was sized by before (an eighth of `partial` + 4,096 keys) does not hold 64 CUs at k = 256
    const SelectPlan p = select_plan(64 * 4 * 256, 256);
    CHECK(p.nrounds >= 1 && (size_t)256 * p.round[0].out == 4194304, "%d", p.round[0].out);
    CHECK((size_t)32 * (64 * 4) * 256 + 4096 == 2101248 && (size_t)256 * p.round[0].out > (size_t)32 * (64 * 4) * 256 + 4096, "today's formula");
    CHECK(scan_scratch(64, 256).partial2 == 4194304, "%zu", scan_scratch(64, 256).partial2);
    const SelectPlan p32 = select_plan(32 * 4 * 129, 129);
    CHECK(p32.nrounds >= 1 && (size_t)256 * p32.round[0].out == 561408 && (size_t)32 * (32 * 4) * 129 + 4096 == 532480, "32 CUs, k = 129");
    CHECK(select_plan(1 << 30, 257).nrounds == -1, "k past TS_MAX_K has no plan");
}

static void pinned_plans() {      // 256 CUs, the full grid of 1,024 workgroups
    SelectPlan p = select_plan(1024 * 10, 10);
    CHECK(p.nrounds == 0 && p.final_form == kSelectHist && p.hist_kr == 1 && p.final_m == 10240, "k = 10");
    p = select_plan(1024 * 13, 13);
    CHECK(p.nrounds == 1 && p.round[0].seg == 1024 && p.round[0].nseg == 13 && p.round[0].out == 169 && p.final_form == kSelectSort1024 &&
              p.final_m == 169, "k = 13");
    p = select_plan(1024 * 64, 64);
    CHECK(p.nrounds == 1 && p.round[0].seg == 1024 && p.round[0].nseg == 64 && p.round[0].out == 4096 && p.final_form == kSelectHist &&
              p.hist_kr == 1 && p.final_m == 4096, "k = 64");
    p = select_plan(1024 * 200, 200);
    CHECK(p.nrounds == 1 && p.round[0].seg == 4096 && p.round[0].nseg == 50 && p.round[0].out == 10000 && p.final_form == kSelectHist &&
              p.hist_kr == 4 && p.final_m == 10000, "k = 200");
    p = select_plan(1216 * 256, 256);       // 304 CUs: two rounds
    CHECK(p.nrounds == 2 && p.round[0].seg == 4096 && p.round[0].nseg == 76 && p.round[0].out == 19456 && p.round[1].seg == 1024 &&
              p.round[1].nseg == 19 && p.round[1].out == 4864 && p.final_form == kSelectHist && p.hist_kr == 4, "304 CUs, k = 256");
    p = select_plan(8 * 256, 256);          // the clamp's floor of 8 workgroups
    CHECK(p.nrounds == 0 && p.final_form == kSelectHist && p.hist_kr == 4, "8 x 256");
    p = select_plan(4 * 100, 100);
    CHECK(p.nrounds == 0 && p.final_form == kSelectSort1024, "4 x 100");
}

static void allowed_rows() {
    std::mt19937 rng(20261018);
    for (int64_t n : {1, 31, 32, 33, 64, 1000}) {
        const size_t words = (size_t)((n + 31) / 32);
        for (int kind = 0; kind < 4; ++kind) {      // ones below n, zero, random (bits past n too), ones in every bit
            std::vector<uint32_t> mask(words, 0u);  // exactly the words the function may read
            for (size_t w = 0; w < words; ++w) mask[w] = kind == 1 ? 0u : kind == 2 ? (uint32_t)rng() : 0xFFFFFFFFu;
            if (kind == 0 && n % 32) mask[words - 1] = (1u << (n % 32)) - 1u;
            int64_t want = 0;
            for (int64_t r = 0; r < n; ++r) want += (mask[(size_t)(r / 32)] >> (r % 32)) & 1u;
            CHECK(count_allowed_rows(mask.data(), n) == want, "n %lld kind %d: %lld, want %lld", (long long)n, kind,
                  (long long)count_allowed_rows(mask.data(), n), (long long)want);
            if (kind == 0 || kind == 3) CHECK(want == n, "n %lld kind %d", (long long)n, kind);
        }
    }
}

static AlgoInputs inputs(int algo, int nq, int k) {     // a 1M-row index the matrix path serves, no bias, no mask
    AlgoInputs in;
    memset(&in, 0, sizeof(in));
    in.algo = algo;
    in.mfma_ok = true;
    in.n = 1000000;
    in.nq = nq;
    in.k = k;
    in.mfma_min_rows = 16384;
    in.scan_max_queries = 4;
    return in;
}

static void algo_choice() {
    auto gives = [](const AlgoInputs& in, int algo) { const AlgoChoice c = choose_algo(in); return !c.unsupported && c.algo == algo; };
    auto refuses = [](const AlgoInputs& in, const char* text) { const AlgoChoice c = choose_algo(in); return c.unsupported && !strcmp(c.unsupported, text); };
    const char* kSubset = "biased search on a subset index";
    const char* kBiasMfma = "the biased search runs on the scan kernel";
    const char* kMask = "the MFMA path serves host masks that keep at least a tenth of the rows, for more than 4 queries";
    // auto: the batch size, the corpus size, the index
    CHECK(gives(inputs(TS_ALGO_AUTO, 4, 10), TS_ALGO_SCAN) && gives(inputs(TS_ALGO_AUTO, 5, 10), TS_ALGO_MFMA), "nq 4 | 5");
    CHECK(gives(inputs(TS_ALGO_AUTO, 1, 65), TS_ALGO_SCAN) && gives(inputs(TS_ALGO_AUTO, 2, 65), TS_ALGO_MFMA), "k > 64: the limit is 1");
    CHECK(gives(inputs(TS_ALGO_AUTO, 2, 64), TS_ALGO_SCAN), "k = 64: the limit is 4");
    CHECK(scan_max_queries(64, 4) == 4 && scan_max_queries(65, 4) == 1 && scan_max_queries(10, 8) == 8 && scan_max_queries(200, 8) == 1, "scan_max_queries");
    AlgoInputs in = inputs(TS_ALGO_AUTO, 256, 10);
    in.n = 16383;
    CHECK(gives(in, TS_ALGO_SCAN), "below TS_MFMA_MIN_ROWS");
    in.n = 16384;
    CHECK(gives(in, TS_ALGO_MFMA), "at TS_MFMA_MIN_ROWS");
    in.mfma_ok = false;
    CHECK(gives(in, TS_ALGO_SCAN), "no matrix kernel for the index");
    in = inputs(TS_ALGO_AUTO, 8, 10);
    in.scan_max_queries = 8;
    CHECK(gives(in, TS_ALGO_SCAN), "TS_SCAN_MAX_QUERIES = 8");
    // the requested algorithm is honoured
    CHECK(gives(inputs(TS_ALGO_SCAN, 256, 10), TS_ALGO_SCAN) && gives(inputs(TS_ALGO_MFMA, 1, 10), TS_ALGO_MFMA), "as requested");
    // bias: the scan, whatever the batch; refused with algo = mfma and on a subset index (the subset first)
    in = inputs(TS_ALGO_AUTO, 256, 10);
    in.bias = true;
    CHECK(gives(in, TS_ALGO_SCAN), "bias forces the scan");
    in.algo = TS_ALGO_MFMA;
    CHECK(refuses(in, kBiasMfma), "bias with algo = mfma");
    in.subset = true;
    CHECK(refuses(in, kSubset), "bias on a subset index, algo = mfma");
    in.algo = TS_ALGO_AUTO;
    CHECK(refuses(in, kSubset), "bias on a subset index");
    in = inputs(TS_ALGO_AUTO, 256, 10);
    in.bias = in.mask = true;
    in.allowed = in.n;
    CHECK(!mask_wants_count(in) && gives(in, TS_ALGO_SCAN), "bias behind a dense mask: the scan, no count");
    // masks
    in = inputs(TS_ALGO_AUTO, 5, 10);
    in.mask = true;
    in.allowed = 100000;
    CHECK(mask_wants_count(in) && gives(in, TS_ALGO_MFMA), "a host mask that keeps a tenth, 5 queries");
    in.allowed = 99999;
    CHECK(gives(in, TS_ALGO_SCAN), "a sparse host mask");
    in.algo = TS_ALGO_MFMA;
    CHECK(refuses(in, kMask), "algo = mfma with a sparse mask");
    in.allowed = 100000;
    CHECK(gives(in, TS_ALGO_MFMA), "algo = mfma with a dense mask");
    in.algo = TS_ALGO_SCAN;
    CHECK(!mask_wants_count(in) && gives(in, TS_ALGO_SCAN), "algo = scan with a dense mask");
    in.algo = TS_ALGO_AUTO;
    in.nq = 4;
    CHECK(!mask_wants_count(in) && gives(in, TS_ALGO_SCAN), "a dense mask, 4 queries");
    in.algo = TS_ALGO_MFMA;
    CHECK(refuses(in, kMask), "algo = mfma with a mask, 4 queries");
    in = inputs(TS_ALGO_AUTO, 256, 10);
    in.mask = in.mask_on_device = true;
    in.allowed = in.n;
    CHECK(!mask_wants_count(in) && gives(in, TS_ALGO_SCAN), "a device mask");
    in.algo = TS_ALGO_MFMA;
    CHECK(refuses(in, kMask), "algo = mfma with a device mask");
    in = inputs(TS_ALGO_AUTO, 256, 10);
    in.mask = true;
    in.allowed = in.n = 16383;
    CHECK(!mask_wants_count(in) && gives(in, TS_ALGO_SCAN), "a dense mask below TS_MFMA_MIN_ROWS");
    in.n = in.allowed = 1000000;
    in.mfma_ok = false;
    CHECK(!mask_wants_count(in) && gives(in, TS_ALGO_SCAN), "a dense mask, no matrix kernel");
    in = inputs(TS_ALGO_AUTO, 2, 200);
    in.mask = true;
    in.allowed = in.n;
    CHECK(mask_wants_count(in) && gives(in, TS_ALGO_MFMA), "a dense mask, 2 queries at k = 200");
}

static void host_keys() {
    const float inf = std::numeric_limits<float>::infinity(), den = std::numeric_limits<float>::denorm_min();
    const float rising[] = {-inf, -3.0e38f, -2.0f, -1.0f, -1e-30f, -2 * den, -den, 0.0f, den, 2 * den, 1e-30f, 0.5f, 1.0f, 2.0f, 3.0e38f, inf};
    const int cnt = (int)(sizeof(rising) / sizeof(rising[0]));
    for (int i = 0; i + 1 < cnt; ++i) {
        CHECK(host_ord_f32(rising[i]) < host_ord_f32(rising[i + 1]), "%g against %g", rising[i], rising[i + 1]);
        CHECK(count_above_key(rising[i], 5, 10) < count_above_key(rising[i + 1], 7, 10), "%g against %g", rising[i], rising[i + 1]);
    }
    CHECK(host_ord_f32(-0.0f) == host_ord_f32(0.0f) && host_ord_f32(0.0f) == 0x80000000u, "%08x %08x", host_ord_f32(-0.0f), host_ord_f32(0.0f));
    CHECK(count_above_key(-0.0f, 3, 10) == count_above_key(0.0f, 3, 10), "-0 and +0");
    const uint64_t hi = (uint64_t)host_ord_f32(1.5f) << 32;
    CHECK(count_above_key(1.5f, -1, 10) == (hi | 0xFFFFFFFFull), "a row before the shard loses every tie");
    CHECK(count_above_key(1.5f, -5000000000ll, 10) == (hi | 0xFFFFFFFFull), "far before the shard");
    CHECK(count_above_key(1.5f, 0, 10) == (hi | 0xFFFFFFFFull) && count_above_key(1.5f, 9, 10) == (hi | (0xFFFFFFFFull - 9)), "inside the shard");
    CHECK(count_above_key(1.5f, 10, 10) == hi && count_above_key(1.5f, 5000000000ll, 10) == hi, "behind the shard wins every tie");
    CHECK(count_above_key(1.5f, 3, 10) > count_above_key(1.5f, 4, 10), "the smaller row ranks first");
    CHECK(count_above_key(std::nanf(""), 3, 10) == ~0ull && count_above_key(-std::nanf(""), -1, 10) == ~0ull, "NaN: all ones");
}

int main() {
    width_table();
    pass_shape();
    select_plans_and_scratch();
    pinned_plans();
    allowed_rows();
    algo_choice();
    host_keys();
    if (g_failed) printf("scan_plan_check: %d checks FAILED\n", g_failed);
    else printf("scan_plan_check: all checks passed\n");
    return g_failed ? 1 : 0;
}
