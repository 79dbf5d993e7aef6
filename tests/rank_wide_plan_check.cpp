// Stand-alone check of theoremsearch_amd/csrc/rank_wide_plan.h, the many-targets rank pass's host decisions at the k-chunked row
// widths (tests/test_rank_wide_plan_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it).
// Exit 0 = every check held; otherwise each failed check is printed.
#include "rank_wide_plan.h"

#include <cstdio>
#include <initializer_list>

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
        int narrowest = 0, widest = 0, count = 0;
        for (int d = -256; d <= 9000; ++d) {
            // the k-chunked search's full pass, width for width ...
            CHECK(rank_wide_served(dtype, d) == wide_served(dtype, d, true), "dtype %d d %d", dtype, d);
            // ... which is: a multiple of 256, a row above 4,096 and of at most 16,384 bytes
            const bool want = d > 0 && d % 256 == 0 && d * elem > 4096 && d * elem <= 16384;
            CHECK(rank_wide_served(dtype, d) == want, "dtype %d d %d", dtype, d);
            // never together with the whole-row pass
            CHECK(!(rank_wide_served(dtype, d) && rank_many_served(dtype, d)), "dtype %d d %d: served twice", dtype, d);
            if (rank_wide_served(dtype, d)) {
                if (!count) narrowest = d;
                widest = d;
                ++count;
            }
        }
        CHECK(count == (dtype == TS_BF16 ? 24 : 12), "dtype %d count %d", dtype, count);
        CHECK(narrowest == (dtype == TS_BF16 ? 2304 : 1280) && widest == (dtype == TS_BF16 ? 8192 : 4096), "dtype %d: %d .. %d", dtype, narrowest, widest);
    }
    for (int d : {2112, 2368, 2048, 8448}) CHECK(!rank_wide_served(TS_BF16, d), "bf16 d %d", d);
    for (int d : {1088, 1024, 4352}) CHECK(!rank_wide_served(TS_F32, d), "fp32 d %d", d);
    for (int d : {2304, 2560, 4096, 8192}) CHECK(rank_wide_served(TS_BF16, d), "bf16 d %d", d);
    for (int d : {1280, 1536, 4096}) CHECK(rank_wide_served(TS_F32, d), "fp32 d %d", d);
    CHECK(!rank_wide_served(7, 2560) && !rank_wide_served(-1, 2560), "unknown storage types");
    // the whole-row pass keeps its limit: the two rules meet at a 4,096-byte row and share no width
    CHECK(kRankMaxRowBytes == 4096 && rank_many_served(TS_BF16, 2048) && !rank_many_served(TS_BF16, 2304), "bf16 at the seam");
    CHECK(rank_many_served(TS_F32, 1024) && !rank_many_served(TS_F32, 1280), "fp32 at the seam");
}

static void tile_and_lds() {
    CHECK(rank_wide_tile_rows() == 64 && rank_wide_tile_rows() == kWideTileRows, "%d", rank_wide_tile_rows());
    CHECK(256 % rank_wide_tile_rows() == 0, "whole tiles inside an allocation padded to 256 rows");
    CHECK(rank_wide_lds_bytes() == 133120 && rank_wide_lds_bytes() == wide_lds_bytes(), "%d", rank_wide_lds_bytes());
    CHECK(rank_wide_lds_bytes() == kWideBuffers * kWideTileRows * kWidePitch && kWideBuffers == 2 && kWidePitch == 1040 && kWideChunkBytes == 1024,
          "%d buffers, pitch %d, chunk %d", kWideBuffers, kWidePitch, kWideChunkBytes);
    CHECK(rank_wide_lds_bytes() <= 160 * 1024 && rank_wide_lds_bytes() <= kRankLdsLimit, "%d bytes of LDS", rank_wide_lds_bytes());
    CHECK(kRankQueries == kWideQueries && kRankT == 16, "%d %d %d", kRankQueries, kWideQueries, kRankT);
    for (int dtype : {TS_F32, TS_BF16})
        for (int d = 256; d <= 8192; d += 256) {
            if (!rank_wide_served(dtype, d)) continue;
            const int row = rank_row_bytes(dtype, d);
            const int nc = wide_chunks(row);
            CHECK(nc >= 5 && nc <= 16, "dtype %d d %d: %d chunks", dtype, d, nc);
            int sum = 0;
            for (int c = 0; c < nc; ++c) {
                const int cb = wide_chunk_bytes(row, c);
                // whole groups of four k-steps; only the last chunk of a bf16 row with d % 512 == 256 is short
                CHECK(cb % 256 == 0 && (cb == 1024 || (cb == 512 && c == nc - 1 && dtype == TS_BF16 && d % 512 == 256)), "dtype %d d %d chunk %d: %d", dtype, d, c, cb);
                sum += cb;
            }
            CHECK(sum == row, "dtype %d d %d: chunks cover %d of %d bytes", dtype, d, sum, row);
        }
    // odd chunk counts: the buffer turn carries across tiles
    CHECK(wide_chunks(rank_row_bytes(TS_BF16, 2304)) == 5 && wide_chunks(rank_row_bytes(TS_BF16, 2560)) == 5 && wide_chunks(rank_row_bytes(TS_F32, 1280)) == 5,
          "%d %d %d", wide_chunks(4608), wide_chunks(5120), wide_chunks(5120));
    CHECK(wide_chunks(rank_row_bytes(TS_BF16, 4096)) % 2 == 0 && wide_chunks(rank_row_bytes(TS_F32, 1536)) % 2 == 0, "even ones");
    CHECK(wide_chunk_bytes(4608, 4) == 512 && wide_chunk_bytes(5120, 4) == 1024, "the ragged last chunk of bf16 2,304");
}

int main() {
    served_set();
    tile_and_lds();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
