// Stand-alone check of the sliding-window attention's walked ranges in theoremsearch_amd/csrc/encoder_plan.h (attn_window_range: the
// chunks a workgroup of 64 queries walks, the key tiles a wave multiplies); tests/test_attn_window_plan_cpu.py builds it with the host
// compiler under -fsanitize=address,undefined and runs it.  Exit 0 = every check held; otherwise each failed check is printed.
// Expected values come from brute force: the smallest and largest key any query of the block (of the wave's tile) may read under
// |q - k| < W and k <= q if causal.  Every S in 1 .. 700, W in kWindows, causal and not, chunks of 32 / 64 / 128 keys.  The lines
// "hash <C> <causal> <W> <value>" fold every (c_first, nchunk, kt_first, kt_end) of a (C, causal, W) in the order S, block, wave;
// the Python side computes the same from its own restatement of the formulas.
#include "encoder_plan.h"

#include <climits>
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

static const int kWindows[] = {1, 2, 16, 17, 31, 32, 33, 64, 65, 128, 129, 257, 700, 701};
static const int kChunks[] = {32, 64, 128};
static const int kMaxSeq = 700;

static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

static void ranges() {
    for (int C : kChunks)
        for (int causal = 0; causal < 2; ++causal)
            for (int W : kWindows) {
                unsigned long long h = 0;
                for (int S = 1; S <= kMaxSeq; ++S) {
                    const int T = (S + 15) / 16, QB = (T + 3) / 4, NCH = (S + C - 1) / C, CT = C / 16;
                    for (int qblk = 0; qblk < QB; ++qblk) {
                        // the block's keys by brute force
                        int kmin = INT_MAX, kmax = -1;
                        for (int q = 64 * qblk; q <= imin(64 * qblk + 63, S - 1); ++q) {
                            kmin = imin(kmin, imax(0, q - (W - 1)));
                            kmax = imax(kmax, imin(S - 1, causal ? q : q + (W - 1)));
                        }
                        for (int wave = 0; wave < 4; ++wave) {
                            const AttnWindowRange r = attn_window_range(S, W, causal != 0, C, qblk, wave);
                            for (int v : {r.c_first, r.nchunk, r.kt_first, r.kt_end}) h = h * 1000003ull + (unsigned long long)v;
                            CHECK(r.nchunk >= 1, "C %d causal %d W %d S %d qblk %d: nchunk %d", C, causal, W, S, qblk, r.nchunk);
                            CHECK(r.c_first >= 0 && r.c_first + r.nchunk <= NCH, "C %d causal %d W %d S %d qblk %d: chunks %d + %d of %d", C, causal,
                                  W, S, qblk, r.c_first, r.nchunk, NCH);
                            CHECK(r.c_first == kmin / C && r.c_first + r.nchunk - 1 == kmax / C, "C %d causal %d W %d S %d qblk %d: chunks %d + %d, keys %d .. %d",
                                  C, causal, W, S, qblk, r.c_first, r.nchunk, kmin, kmax);
                            const int qi = 4 * qblk + wave;
                            if (qi >= T) {
                                CHECK(r.kt_first == 0 && r.kt_end == 0, "a wave past the sequence walks no tile: %d %d", r.kt_first, r.kt_end);
                                continue;
                            }
                            int tmin = INT_MAX, tmax = -1;
                            for (int q = 16 * qi; q <= imin(16 * qi + 15, S - 1); ++q) {
                                tmin = imin(tmin, imax(0, q - (W - 1)));
                                tmax = imax(tmax, imin(S - 1, causal ? q : q + (W - 1)));
                            }
                            // no allowed key outside the wave's tiles (and no tile without one at either end)
                            CHECK(r.kt_first == tmin / 16 && r.kt_end == tmax / 16 + 1, "C %d causal %d W %d S %d qi %d: tiles %d .. %d, keys %d .. %d", C,
                                  causal, W, S, qi, r.kt_first, r.kt_end, tmin, tmax);
                            // ... and every walked tile lies in a walked chunk
                            CHECK(r.kt_first / CT >= r.c_first && (r.kt_end - 1) / CT < r.c_first + r.nchunk, "C %d causal %d W %d S %d qi %d: tiles outside the chunks",
                                  C, causal, W, S, qi);
                            // a window that reaches the sequence's length: the unwindowed kernels' ranges
                            if (W >= S) {
                                const int kt_blk = causal ? imin(4 * qblk + 4, T) : T;
                                CHECK(r.c_first == 0 && r.nchunk == (kt_blk + CT - 1) / CT && r.kt_first == 0 && r.kt_end == (causal ? qi + 1 : T),
                                      "C %d causal %d W %d S %d qi %d: not the unwindowed walk", C, causal, W, S, qi);
                            }
                        }
                    }
                }
                printf("hash %d %d %d %llu\n", C, causal, W, h);
            }
}

// the largest window and sequence: no overflow (the sanitizer aborts on one), the unwindowed ranges
static void extremes() {
    for (int causal = 0; causal < 2; ++causal) {
        const AttnWindowRange r = attn_window_range(32768, INT_MAX, causal != 0, 32, 511, 3);
        CHECK(r.c_first == 0 && r.nchunk == 1024 && r.kt_first == 0 && r.kt_end == 2048, "%d %d %d %d", r.c_first, r.nchunk, r.kt_first, r.kt_end);
        const AttnWindowRange w = attn_window_range(32768, 257, causal != 0, 32, 511, 3);
        CHECK(w.c_first == (32704 - 256) / 32 && w.c_first + w.nchunk == 1024 && w.kt_first == (32752 - 256) / 16 && w.kt_end == 2048, "%d %d %d %d",
              w.c_first, w.nchunk, w.kt_first, w.kt_end);
    }
}

int main() {
    ranges();
    extremes();
    if (g_failed) {
        printf("%d checks FAILED\n", g_failed);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
