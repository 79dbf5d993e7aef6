// Stand-alone check of theoremsearch_amd/csrc/wide_plan.h, the k-chunked matrix kernel's host decisions
// (tests/test_wide_plan_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it).
// Exit 0 = every check held; otherwise each failed check is printed.
#include "wide_plan.h"
#include "scan_plan.h"

#include <cstdio>
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

constexpr int kMaxD = 16640;
static bool hand_laid(int d) { return d == 384 || d == 512 || d == 768 || d == 1024; }

static void served_set() {
    for (int dtype : {TS_F32, TS_BF16}) {
        const int elem = dtype == TS_BF16 ? 2 : 4;
        int first = 0, widest = 0, count = 0;
        for (int d = 1; d <= kMaxD; ++d) {
            const bool want = d % 256 == 0 && d * elem > 4096 && d * elem <= 16384;
            CHECK(wide_served(dtype, d, true) == want, "dtype %d d %d", dtype, d);
            CHECK(!wide_served(dtype, d, false), "dtype %d d %d without the two-level search", dtype, d);
            CHECK(!(wide_served(dtype, d, true) && (anyd_served(dtype, d, true) || hand_laid(d))), "dtype %d d %d: served twice", dtype, d);
            if (wide_served(dtype, d, true)) {
                if (!first) first = d;
                widest = d;
                ++count;
            }
        }
        CHECK(first == (dtype == TS_BF16 ? 2304 : 1280), "dtype %d first %d", dtype, first);
        CHECK(widest == (dtype == TS_BF16 ? 8192 : 4096), "dtype %d widest %d", dtype, widest);
        CHECK(count == (dtype == TS_BF16 ? 24 : 12), "dtype %d count %d", dtype, count);
        for (int d : {0, -256, -2560, 256, 768, 1024}) CHECK(!wide_served(dtype, d, true), "dtype %d d %d", dtype, d);
        CHECK(!wide_served(dtype, 4096 / elem, true), "dtype %d: a 4,096-byte row is the general-width kernel's", dtype);
    }
    for (int d : {2112, 1088, 2176, 8448}) CHECK(!wide_served(TS_BF16, d, true), "bf16 d %d", d);
    for (int d : {1088, 1344, 4352}) CHECK(!wide_served(TS_F32, d, true), "fp32 d %d", d);
    CHECK(wide_served(TS_BF16, 2304, true) && wide_served(TS_BF16, 8192, true) && wide_served(TS_F32, 1280, true) && wide_served(TS_F32, 4096, true), "the ends");
    CHECK(!wide_served(7, 2560, true) && !wide_served(-1, 2560, true) && !wide_served(TS_BF16 + TS_F32 + 5, 1536, true), "unknown storage types");
    // the narrower rule is what it was
    CHECK(kAnydMaxRowBytes == 4096 && anyd_served(TS_BF16, 2048, true) && !anyd_served(TS_BF16, 2304, true) && !anyd_served(TS_F32, 1280, true), "anyd_plan.h");
}

// walk the chunks of every served row: they tile it, each a whole number of four-k-step groups, each ONE DMA wave instruction
// (64 lanes x 16 bytes = 1,024 contiguous LDS bytes at most) that stays inside its LDS row
static void chunks_and_lds() {
    CHECK(kWideChunkBytes == 1024 && kWideGroupBytes == 256 && kWidePitch == 1040 && kWideBuffers == 2, "%d %d %d %d", kWideChunkBytes, kWideGroupBytes, kWidePitch, kWideBuffers);
    for (int dtype : {TS_F32, TS_BF16})
        for (int d = 1; d <= kMaxD; ++d) {
            if (!wide_served(dtype, d, true)) continue;
            const int rb = anyd_row_bytes(dtype, d);
            CHECK(rb == d * (dtype == TS_BF16 ? 2 : 4) && rb % 512 == 0, "dtype %d d %d", dtype, d);
            std::vector<unsigned char> seen((size_t)rb, 0);
            const int nc = wide_chunks(rb);
            CHECK(nc >= 5 && nc <= 16, "dtype %d d %d: %d chunks", dtype, d, nc);
            for (int c = 0; c < nc; ++c) {
                const int cb = wide_chunk_bytes(rb, c);
                CHECK(cb > 0 && cb % kWideGroupBytes == 0 && cb <= kWideChunkBytes, "dtype %d d %d chunk %d: %d bytes", dtype, d, c, cb);
                CHECK(c + 1 == nc || cb == kWideChunkBytes, "dtype %d d %d chunk %d: only the last chunk is short", dtype, d, c);
                // the lanes of the chunk's DMA instruction: lane l moves row bytes [1,024 c + 16 l, + 16) to LDS row bytes [16 l, + 16)
                for (int lane = 0; lane < 64; ++lane) {
                    if (lane * 16 >= cb) continue;
                    CHECK(lane * 16 + 16 <= kWidePitch - kWideRowPad, "dtype %d d %d chunk %d lane %d leaves the LDS row", dtype, d, c, lane);
                    for (int b = 0; b < 16; ++b) {
                        const int at = c * kWideChunkBytes + lane * 16 + b;
                        CHECK(at < rb, "dtype %d d %d chunk %d lane %d reads past the row", dtype, d, c, lane);
                        if (at < rb) ++seen[(size_t)at];
                    }
                }
            }
            int wrong = 0;
            for (int at = 0; at < rb; ++at) wrong += seen[(size_t)at] != 1;
            CHECK(wrong == 0, "dtype %d d %d: %d bytes not moved exactly once", dtype, d, wrong);
            if (dtype == TS_F32) CHECK(wide_chunk_bytes(rb, nc - 1) == kWideChunkBytes, "fp32 d %d: no ragged chunk", d);
        }
    CHECK(wide_chunks(4608) == 5 && wide_chunk_bytes(4608, 4) == 512 && wide_chunks(5120) == 5 && wide_chunk_bytes(5120, 4) == 1024 && wide_chunks(16384) == 16, "examples");
    // the launches
    CHECK(kWideBuffers * kWideTileRows * kWidePitch <= wide_lds_bytes() && wide_lds_bytes() <= kAnydLdsLimit && wide_lds_bytes() == 133120, "%d", wide_lds_bytes());
    CHECK(kWideBuffers * kWideSampleRows * kWidePitch <= wide_sample_lds_bytes() && wide_sample_lds_bytes() <= kWideSampleLdsLimit, "%d", wide_sample_lds_bytes());
    CHECK(2 * wide_sample_lds_bytes() <= kAnydLdsLimit && kWideSampleLdsLimit == 144 * 1024, "two sample workgroups a CU");
    CHECK(256 % kWideTileRows == 0 && kWideTileRows % 32 == 0 && kWideSampleRows == 32, "%d", kWideTileRows);
    CHECK(kWideQueries == 256, "%d", kWideQueries);
}

// AUTO takes the kernel above the limit, the scan at or below it; k > 64 drops choose_algo's limit to 1 and search_choose
// keeps AUTO on the scan up to wide_scan_limit
static void auto_limit() {
    for (int dtype : {TS_F32, TS_BF16}) {
        const int limit = wide_scan_max_queries(dtype);
        CHECK(limit == (dtype == TS_F32 ? 8 : 4), "dtype %d: %d", dtype, limit);
        for (int k : {1, 10, 64}) CHECK(wide_scan_limit(dtype, k) == limit, "dtype %d k %d", dtype, k);
        for (int k : {65, 100, 256}) CHECK(wide_scan_limit(dtype, k) == (dtype == TS_F32 ? 2 : 1), "dtype %d k %d", dtype, k);
        AlgoInputs in;
        memset(&in, 0, sizeof(in));
        in.algo = TS_ALGO_AUTO;
        in.n = 1000000;
        in.mfma_min_rows = 16384;
        in.scan_max_queries = limit;
        for (int nq : {1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 256, 1000})
            for (int k : {10, 64, 65, 100}) {
                in.nq = nq;
                in.k = k;
                in.mfma_ok = !(nq <= wide_scan_limit(dtype, k));          // search_choose: not offered to AUTO at or below the limit
                CHECK(choose_algo(in).algo == (nq > wide_scan_limit(dtype, k) ? TS_ALGO_MFMA : TS_ALGO_SCAN), "dtype %d nq %d k %d", dtype, nq, k);
                in.mfma_ok = true;                                         // ... and choose_algo's own limit is never above it
                if (nq <= scan_max_queries(k, limit)) CHECK(nq <= wide_scan_limit(dtype, k), "dtype %d nq %d k %d", dtype, nq, k);
            }
        in.mfma_ok = true;
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
    chunks_and_lds();
    auto_limit();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
