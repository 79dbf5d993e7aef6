// Stand-alone check of theoremsearch_amd/csrc/anyd_plan.h, the general-width matrix kernel's host decisions
// (tests/test_anywidth_plan_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it).
// Exit 0 = every check held; otherwise each failed check is printed.
#include "anyd_plan.h"
#include "scan_plan.h"

#include <cstdio>

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

// the threshold sample's launch (kernels_sample.h, search_mfma.hip: 32 rows per workgroup, 16 bytes of padding a row)
static int sample_lds_bytes(int rows, int row_bytes) { return rows * (row_bytes + 16); }
constexpr int kSampleLdsMax = 144 * 1024;

static void served_set() {
    for (int dtype : {TS_F32, TS_BF16}) {
        const int elem = dtype == TS_BF16 ? 2 : 4;
        int widest = 0, count = 0;
        for (int d = 1; d <= 4096; ++d) {
            const bool want = d % 64 == 0 && d >= 128 && d != 384 && d != 512 && d != 768 && d != 1024 && d * elem <= 4096;
            CHECK(anyd_served(dtype, d, true) == want, "dtype %d d %d", dtype, d);
            CHECK(!anyd_served(dtype, d, false), "dtype %d d %d without the two-level search", dtype, d);
            if (anyd_served(dtype, d, true)) { widest = d; ++count; }
        }
        // bf16: 128 .. 2048 in steps of 64 = 31 widths less the four; fp32: 128 .. 1024 = 15 less the four
        CHECK(widest == (dtype == TS_BF16 ? 2048 : 960), "dtype %d widest %d", dtype, widest);
        CHECK(count == (dtype == TS_BF16 ? 27 : 11), "dtype %d count %d", dtype, count);
        for (int d : {384, 512, 768, 1024, 64, 0, -64, 200, 100, 1000}) CHECK(!anyd_served(dtype, d, true), "dtype %d d %d", dtype, d);
    }
    CHECK(anyd_served(TS_BF16, 2048, true) && !anyd_served(TS_BF16, 2112, true), "bf16 row limit");
    CHECK(anyd_row_bytes(TS_F32, 1024) == 4096 && !anyd_served(TS_F32, 1024, true) && !anyd_served(TS_F32, 1088, true), "fp32 row limit");
    CHECK(!anyd_served(7, 192, true) && !anyd_served(-1, 192, true), "unknown storage types");
}

static void tiles_and_lds() {
    for (int dtype : {TS_F32, TS_BF16})
        for (int d = 64; d <= 4096; d += 64) {
            if (!anyd_served(dtype, d, true)) continue;
            const int rb = anyd_row_bytes(dtype, d);
            CHECK(rb == d * (dtype == TS_BF16 ? 2 : 4) && rb % 128 == 0, "dtype %d d %d", dtype, d);
            const int rows = anyd_tile_rows(rb);
            CHECK(rows == (rb <= 2048 ? 64 : 32) && rows == 16 * anyd_row_blocks(rb), "dtype %d d %d: %d rows", dtype, d, rows);
            const int lds = anyd_lds_bytes(rb);
            CHECK(lds == rows * (rb + 16), "dtype %d d %d: %d", dtype, d, lds);
            CHECK(lds <= 163840 && lds <= kAnydLdsMax, "dtype %d d %d: %d bytes of LDS", dtype, d, lds);
            CHECK(sample_lds_bytes(32, rb) <= kSampleLdsMax, "dtype %d d %d: the sample's %d bytes", dtype, d, sample_lds_bytes(32, rb));
            // whole staging tiles inside an allocation padded to 256 rows, and a whole number of 32-row search tiles each
            CHECK(256 % rows == 0 && rows % 32 == 0, "dtype %d d %d", dtype, d);
        }
    CHECK(anyd_lds_bytes(4096) == 131584 && anyd_lds_bytes(2048) == 132096 && kAnydLdsMax == 132096, "%d %d", anyd_lds_bytes(4096), anyd_lds_bytes(2048));
    CHECK(anyd_lds_bytes(384) == 64 * 400 && anyd_lds_bytes(2560) == 32 * 2576, "%d %d", anyd_lds_bytes(384), anyd_lds_bytes(2560));
    CHECK(kAnydQueries == 256, "%d", kAnydQueries);
}

// AUTO takes the kernel above the limit, the scan at or below it; k > 64 drops the limit to 1
static void auto_limit() {
    for (int dtype : {TS_F32, TS_BF16}) {
        const int limit = anyd_scan_max_queries(dtype);
        CHECK(limit == 4, "dtype %d: %d", dtype, limit);
        for (int k : {1, 10, 64}) CHECK(anyd_scan_limit(dtype, k) == 4, "dtype %d k %d", dtype, k);
        for (int k : {65, 100, 256}) CHECK(anyd_scan_limit(dtype, k) == (dtype == TS_F32 ? 2 : 1), "dtype %d k %d", dtype, k);
        AlgoInputs in;
        memset(&in, 0, sizeof(in));
        in.algo = TS_ALGO_AUTO;
        in.mfma_ok = true;
        in.n = 1000000;
        in.mfma_min_rows = 16384;
        in.scan_max_queries = limit;
        for (int nq : {1, 4, 5, 16, 17, 64, 256, 1000}) {
            in.nq = nq;
            in.k = 10;
            CHECK(choose_algo(in).algo == (nq > limit ? TS_ALGO_MFMA : TS_ALGO_SCAN), "dtype %d nq %d", dtype, nq);
            in.k = 64;
            CHECK(choose_algo(in).algo == (nq > limit ? TS_ALGO_MFMA : TS_ALGO_SCAN), "dtype %d nq %d k 64", dtype, nq);
            in.k = 65;
            CHECK(choose_algo(in).algo == (nq > 1 ? TS_ALGO_MFMA : TS_ALGO_SCAN), "dtype %d nq %d k 65", dtype, nq);
        }
        in.nq = 256;
        in.k = 10;
        in.n = 16383;
        CHECK(choose_algo(in).algo == TS_ALGO_SCAN, "below TS_MFMA_MIN_ROWS");
        in.n = 16384;
        CHECK(choose_algo(in).algo == TS_ALGO_MFMA, "at TS_MFMA_MIN_ROWS");
        in.mfma_ok = false;
        CHECK(choose_algo(in).algo == TS_ALGO_SCAN, "an index the matrix path does not serve");
        in.mfma_ok = true;
        in.algo = TS_ALGO_SCAN;
        CHECK(choose_algo(in).algo == TS_ALGO_SCAN, "algo = scan");
        in.algo = TS_ALGO_MFMA;
        in.nq = 1;
        in.n = 1;
        CHECK(choose_algo(in).algo == TS_ALGO_MFMA && !choose_algo(in).unsupported, "algo = mfma");
    }
}

int main() {
    served_set();
    tiles_and_lds();
    auto_limit();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
