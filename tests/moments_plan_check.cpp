// Stand-alone check of theoremsearch_amd/csrc/moments_plan.h, the corpus-moments pass's host decisions and LDS image
// (tests/test_moments_plan_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it).
// Exit 0 = every check held; otherwise each failed check is printed.
#include "moments_plan.h"

#include <cstdio>
#include <cstring>
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

constexpr int64_t kL = kMomFlushRows;
static const int64_t kNs[] = {1, 31, 32, 33, 255, 257, kL - 1, kL, kL + 1, 10000000};
static const int kCUs[] = {1, 8, 256};

static void served_set() {
    for (int dtype : {TS_F32, TS_BF16}) {
        int count = 0;
        for (int d = -64; d <= 4096; ++d) {
            const bool want = d >= 128 && d <= 1024 && d % 64 == 0;
            CHECK(mom_served(dtype, d) == want, "dtype %d d %d", dtype, d);
            count += mom_served(dtype, d);
        }
        CHECK(count == 15, "dtype %d: %d widths", dtype, count);
    }
    for (int d : {384, 512, 768, 1024}) CHECK(mom_served(TS_BF16, d) && mom_served(TS_F32, d), "d %d", d);
    CHECK(!mom_served(7, 768) && !mom_served(-1, 768), "unknown storage types");
    CHECK(!mom_served(TS_BF16, 64) && !mom_served(TS_BF16, 1088) && !mom_served(TS_F32, 2048), "the refused widths of the issue");
}

static void pairs_cover_the_upper_triangle() {
    for (int d = kMomMinD; d <= kMomMaxD; d += 64) {
        const int P = mom_panels(d);
        int cols = 0;
        for (int p = 0; p < P; ++p) {
            const int w = mom_panel_cols(d, p);
            CHECK(w == 128 || (w == 64 && p == P - 1), "d %d panel %d width %d", d, p, w);
            cols += w;
        }
        CHECK(cols == d, "d %d: panels hold %d columns", d, cols);
        std::vector<int> seen((size_t)P * P, 0);
        for (int idx = 0; idx < mom_pairs(d); ++idx) {
            int pi = -1, pj = -1;
            mom_pair(P, idx, &pi, &pj);
            CHECK(0 <= pi && pi <= pj && pj < P, "d %d pair %d = (%d, %d)", d, idx, pi, pj);
            if (0 <= pi && pi <= pj && pj < P) ++seen[(size_t)pi * P + pj];
        }
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < P; ++j) CHECK(seen[(size_t)i * P + j] == (i <= j ? 1 : 0), "d %d pair (%d, %d) seen %d times", d, i, j, seen[(size_t)i * P + j]);
    }
    CHECK(mom_pairs(128) == 1 && mom_pairs(192) == 3 && mom_pairs(1024) == 36, "pair counts");
}

static void ranges_lds_and_partials() {
    for (int dtype : {TS_F32, TS_BF16})
        for (int d = kMomMinD; d <= kMomMaxD; d += 64)
            for (int64_t n : kNs)
                for (int cus : kCUs)
                    for (int pass = 0; pass < 3; ++pass) {      // the pair pass, the indicator pass with 1 and with 256 groups
                        const int ngroups = pass == 2 ? kMomMaxGroups : 1;
                        const int units = pass == 0 ? mom_pairs(d) : mom_panels(d) * mom_group_chunks(ngroups);
                        const int64_t unit_bytes = pass == 0 ? mom_pair_tile_bytes() : mom_group_tile_bytes();
                        const int R = mom_ranges(n, cus, units, unit_bytes);
                        CHECK(R >= 1 && R <= kMomMaxRanges && R <= mom_tiles(n), "d %d n %lld cus %d: %d ranges", d, (long long)n, cus, R);
                        CHECK((int64_t)units * R <= (int64_t)kMomBlocksPerCU * cus || R == 1, "d %d n %lld cus %d: %d x %d workgroups are more than one round", d,
                              (long long)n, cus, units, R);
                        CHECK(mom_partial_bytes(R, units, unit_bytes) <= kMomPartialCap, "d %d n %lld cus %d: %lld partial bytes", d, (long long)n, cus,
                              (long long)mom_partial_bytes(R, units, unit_bytes));
                        // the ranges tile [0, ceil32(n)) exactly once, each starts on a tile, none is empty
                        const int64_t end = (n + 31) / 32 * 32;
                        int64_t at = 0;
                        for (int i = 0; i < R; ++i) {
                            int64_t r0 = -1, r1 = -1;
                            mom_range_rows(n, R, i, &r0, &r1);
                            CHECK(r0 == at && r1 > r0 && r0 % kMomTileRows == 0, "d %d n %lld cus %d range %d/%d = [%lld, %lld) after %lld", d, (long long)n, cus,
                                  i, R, (long long)r0, (long long)r1, (long long)at);
                            at = r1;
                        }
                        CHECK(at == end, "d %d n %lld cus %d: ranges end at %lld, not %lld", d, (long long)n, cus, (long long)at, (long long)end);
                        const MomGrid g = mom_grid(units, R);
                        CHECK(g.x == units && g.y == R && g.y <= 65535, "grid %d x %d", g.x, g.y);
                        CHECK(mom_lds_bytes(dtype, pass == 0) <= kMomLdsLimit, "dtype %d: %d LDS bytes", dtype, mom_lds_bytes(dtype, pass == 0));
                    }
    CHECK(mom_ranges(0, 256, 36, mom_pair_tile_bytes()) == 0, "no rows, no ranges");
    CHECK(mom_lds_bytes(TS_BF16, true) == 32768 && mom_lds_bytes(TS_F32, true) == 65536 && mom_lds_bytes(TS_BF16, false) == 16384, "LDS bytes");
    // a 1024-wide index on the whole device: the partials stay far below the cap
    CHECK(mom_partial_bytes(mom_ranges(10000000, 256, 36, mom_pair_tile_bytes()), 36, mom_pair_tile_bytes()) <= (int64_t)128 << 20, "1024-wide partials");
}

// The image, replayed: stage a tile the way the DMA lanes do, then read every fragment the way the lanes do and compare with
// the matrix; count the banks a half wave touches.
static void lds_image() {
    for (int f32 = 0; f32 < 2; ++f32) {
        const int elem = f32 ? 4 : 2, subs = 2 * mom_panel_subs(f32 ? TS_F32 : TS_BF16), sub_cols = kMomSubBytes / elem;
        const int bytes = mom_lds_bytes(f32 ? TS_F32 : TS_BF16, true);
        CHECK(bytes == subs * kMomTileRows * kMomSubBytes, "image bytes");
        // value of (sub, row, column of the sub-image): unique 16-bit id; the image holds it per element
        std::vector<int> img((size_t)bytes / elem, -1);
        std::vector<int> written((size_t)bytes / 16, 0);
        for (int sub = 0; sub < subs; ++sub)
            for (int r8 = 0; r8 < kMomTileRows; r8 += 8)
                for (int lane = 0; lane < 64; ++lane) {
                    const int row = r8 + (lane >> 3), ch = mom_stage_chunk(f32, lane, r8);
                    CHECK(ch >= 0 && ch < 8, "chunk %d", ch);
                    const int dst = (sub * kMomTileRows + r8) * kMomSubBytes + 16 * lane;      // where the DMA puts the lane's 16 bytes
                    CHECK(dst == mom_lds_off(f32, sub, row, ch), "sub %d row %d lane %d: slot %d, image says %d", sub, row, lane, dst, mom_lds_off(f32, sub, row, ch));
                    ++written[(size_t)dst / 16];
                    for (int e = 0; e < 16 / elem; ++e) img[(size_t)dst / elem + e] = (sub * kMomTileRows + row) * sub_cols + ch * (16 / elem) + e;
                }
        for (size_t i = 0; i < written.size(); ++i) CHECK(written[i] == 1, "slot %zu written %d times", i, written[i]);

        const int blocks = 2 * kMomPanel / 16;       // 16-column blocks of the two panels
        for (int cb = 0; cb < blocks; ++cb) {
            const int sub_base = cb < blocks / 2 ? 0 : subs / 2, cbp = cb % (blocks / 2);
            if (f32) {
                for (int s = 0; s < kMomTileRows / 4; ++s) {
                    std::set<int> banks[2];
                    for (int lane = 0; lane < 64; ++lane) {
                        const int off = mom_frag_off(true, lane, sub_base, cbp) + s * mom_step_bytes(true);
                        CHECK(off >= 0 && off + 4 <= bytes && off % 4 == 0, "offset %d", off);
                        const int row = 4 * s + (lane >> 4), col = 16 * cbp + (lane & 15);
                        const int want = ((sub_base + col / sub_cols) * kMomTileRows + row) * sub_cols + col % sub_cols;
                        CHECK(img[(size_t)off / 4] == want, "fp32 block %d step %d lane %d reads %d, wants %d", cb, s, lane, img[(size_t)off / 4], want);
                        banks[lane >> 5].insert((off / 4) % 32);
                    }
                    CHECK(banks[0].size() == 32 && banks[1].size() == 32, "fp32 block %d step %d: %zu / %zu banks", cb, s, banks[0].size(), banks[1].size());
                }
            } else {
                for (int ks = 0; ks < 2; ++ks)
                    for (int h = 0; h < 2; ++h) {
                        // the transposed read: per group of 16 lanes, lane 4 q + p names row q, columns 4 p .. 4 p + 3 of a 4 x 16
                        // block; lane i receives column i of the four rows, row q in element q
                        std::set<int> banks[2];
                        int addr[64];
                        for (int lane = 0; lane < 64; ++lane) {
                            addr[lane] = mom_frag_off(false, lane, sub_base, cbp) + ks * mom_step_bytes(false) + h * kMomTrSecond;
                            CHECK(addr[lane] >= 0 && addr[lane] + 8 <= bytes && addr[lane] % 8 == 0, "address %d of lane %d", addr[lane], lane);
                            banks[lane >> 5].insert((addr[lane] / 4) % 64);
                            banks[lane >> 5].insert((addr[lane] / 4 + 1) % 64);
                        }
                        CHECK(banks[0].size() == 64 && banks[1].size() == 64, "bf16 block %d step %d.%d: %zu / %zu banks", cb, ks, h, banks[0].size(), banks[1].size());
                        for (int lane = 0; lane < 64; ++lane) {
                            const int g = lane >> 4, i = lane & 15;
                            for (int q = 0; q < 4; ++q) {
                                const int src = addr[16 * g + 4 * q + i / 4] + 2 * (i % 4);      // row q, column i of the block
                                const int row = 32 * ks + mom_frag_row(lane, 4 * h + q), col = 16 * cbp + i;
                                const int want = ((sub_base + col / sub_cols) * kMomTileRows + row) * sub_cols + col % sub_cols;
                                CHECK(img[(size_t)src / 2] == want, "bf16 block %d step %d.%d lane %d element %d reads %d, wants %d", cb, ks, h, lane, q,
                                      img[(size_t)src / 2], want);
                            }
                        }
                    }
                // every row of a k-step is held by exactly one (lane group, element)
                int held[32];
                memset(held, 0, sizeof(held));
                for (int g = 0; g < 4; ++g)
                    for (int e = 0; e < 8; ++e) ++held[mom_frag_row(16 * g, e)];
                for (int r = 0; r < 32; ++r) CHECK(held[r] == 1, "row %d of a step held %d times", r, held[r]);
            }
        }
    }
}

int main() {
    served_set();
    pairs_cover_the_upper_triangle();
    ranges_lds_and_partials();
    lds_image();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
