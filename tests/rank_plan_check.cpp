// Stand-alone check of theoremsearch_amd/csrc/rank_plan.h, the many-targets rank pass's host decisions
// (tests/test_rank_plan_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it).
// Exit 0 = every check held; otherwise each failed check is printed.
#include "rank_plan.h"

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
        int widest = 0, count = 0;
        for (int d = -128; d <= 4608; ++d) {
            const bool want = d >= 128 && d % 64 == 0 && d * elem <= 4096;
            CHECK(rank_many_served(dtype, d) == want, "dtype %d d %d", dtype, d);
            if (rank_many_served(dtype, d)) { widest = d; ++count; }
        }
        // every multiple of 64 from 128 to the limit: bf16 128 .. 2048 = 31 widths, fp32 128 .. 1024 = 15
        CHECK(widest == (dtype == TS_BF16 ? 2048 : 1024), "dtype %d widest %d", dtype, widest);
        CHECK(count == (dtype == TS_BF16 ? 31 : 15), "dtype %d count %d", dtype, count);
        for (int d = 128; d * elem <= 4096; d += 64) CHECK(rank_many_served(dtype, d), "dtype %d d %d", dtype, d);
        for (int d : {384, 512, 768, 1024}) CHECK(rank_many_served(dtype, d), "dtype %d d %d: served before", dtype, d);
        for (int d : {64, 100, 200, 0, -64, 1000}) CHECK(!rank_many_served(dtype, d), "dtype %d d %d", dtype, d);
    }
    CHECK(rank_many_served(TS_BF16, 2048) && !rank_many_served(TS_BF16, 2112), "bf16 row limit");
    CHECK(rank_many_served(TS_F32, 1024) && !rank_many_served(TS_F32, 1088), "fp32 row limit");
    CHECK(!rank_many_served(7, 192) && !rank_many_served(-1, 192), "unknown storage types");
}

static void tiles_and_lds() {
    for (int dtype : {TS_F32, TS_BF16})
        for (int d = 64; d <= 4096; d += 64) {
            if (!rank_many_served(dtype, d)) continue;
            const int row = rank_row_bytes(dtype, d);
            CHECK(row == d * (dtype == TS_BF16 ? 2 : 4) && row % 128 == 0 && row <= kRankMaxRowBytes, "dtype %d d %d", dtype, d);
            const int rb = rank_rb(row);
            CHECK(rb == (row <= 2048 ? 4 : 2) && rank_tile_rows(row) == 16 * rb, "dtype %d d %d: RB %d", dtype, d, rb);
            const int lds = rank_lds_bytes(rb, row);
            CHECK(lds == 16 * rb * (row + 16), "dtype %d d %d: %d", dtype, d, lds);
            CHECK(lds <= 160 * 1024 && lds <= kRankLdsLimit && lds <= rank_lds_max(rb), "dtype %d d %d: %d bytes of LDS", dtype, d, lds);
            // whole tiles inside an allocation padded to 256 rows
            CHECK(256 % rank_tile_rows(row) == 0, "dtype %d d %d", dtype, d);
            // k-steps of 64 bytes a row quarter: fp32 needs no tail group, bf16 has one of two steps where d % 128 == 64
            const int steps = rank_steps(dtype, d);
            CHECK(steps * 64 == row && steps % 2 == 0, "dtype %d d %d: %d steps", dtype, d, steps);
            CHECK(rank_tail(dtype, d) == (dtype == TS_BF16 && d % 128 == 64) && rank_tail(dtype, d) == (steps % 4 == 2), "dtype %d d %d: %d steps", dtype, d, steps);
        }
    // at the tile change: a 2,048-byte row keeps 64 rows, the next served row (2,176 bytes) and the widest take 32
    CHECK(rank_rb(2048) == 4 && rank_lds_bytes(4, 2048) == 132096, "%d %d", rank_rb(2048), rank_lds_bytes(4, 2048));
    CHECK(rank_rb(2049) == 2 && rank_rb(2176) == 2 && rank_lds_bytes(2, 2176) == 32 * 2192, "%d %d", rank_rb(2176), rank_lds_bytes(2, 2176));
    CHECK(rank_rb(4096) == 2 && rank_lds_bytes(2, 4096) == 131584, "%d %d", rank_rb(4096), rank_lds_bytes(2, 4096));
    CHECK(rank_lds_max(4) == 132096 && rank_lds_max(2) == 131584, "%d %d", rank_lds_max(4), rank_lds_max(2));
    // the four widths served before this header existed keep their tile and their LDS bytes
    struct Old { int dtype, d, rb, lds; };
    const Old old[] = {{TS_BF16, 384, 4, 64 * 784},  {TS_BF16, 512, 4, 64 * 1040}, {TS_BF16, 768, 4, 64 * 1552}, {TS_BF16, 1024, 4, 64 * 2064},
                       {TS_F32, 384, 4, 64 * 1552},  {TS_F32, 512, 4, 64 * 2064},  {TS_F32, 768, 2, 32 * 3088},  {TS_F32, 1024, 2, 32 * 4112}};
    for (const Old& o : old) {
        const int row = rank_row_bytes(o.dtype, o.d);
        CHECK(rank_rb(row) == o.rb && rank_lds_bytes(rank_rb(row), row) == o.lds, "dtype %d d %d: RB %d, %d bytes", o.dtype, o.d, rank_rb(row),
              rank_lds_bytes(rank_rb(row), row));
        CHECK(!rank_tail(o.dtype, o.d), "dtype %d d %d: the kernel form without the tail group, as before", o.dtype, o.d);
    }
    CHECK(kRankT == 16 && kRankQueries == 256 && kRankRowPad == 16, "%d %d %d", kRankT, kRankQueries, kRankRowPad);
}

int main() {
    served_set();
    tiles_and_lds();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
