// Stand-alone check of theoremsearch_amd/csrc/encoder_plan.h, the encoder ops' host decisions (tests/test_encoder_plan_cpu.py
// builds it with the host compiler under -fsanitize=address,undefined and runs it).  Exit 0 = every check held; otherwise each
// failed check is printed.  Expected values are literals here: what encoder_ops.hip launched before the decisions moved.
#include "encoder_plan.h"

#include <climits>
#include <cstdio>
#include <random>

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

constexpr int kCuLds = 160 * 1024;

static void norm_family() {
    struct Case { int dtype, d, ln; };      // ln 0 = refused
    const Case cases[] = {{TS_F32, 4, 1},  {TS_F32, 256, 1},  {TS_F32, 260, 2},  {TS_F32, 512, 2},   {TS_F32, 516, 4},   {TS_F32, 1024, 4},  {TS_F32, 1028, 0},
                          {TS_BF16, 8, 1}, {TS_BF16, 512, 1}, {TS_BF16, 520, 2}, {TS_BF16, 1024, 2}, {TS_BF16, 1032, 4}, {TS_BF16, 2048, 4}, {TS_BF16, 2056, 0},
                          // the widths of the three encoders: BERT-base, Qwen3-0.6B, embeddinggemma
                          {TS_F32, 768, 4}, {TS_BF16, 768, 2}, {TS_F32, 1024, 4}, {TS_BF16, 1024, 2},
                          // not a multiple of the vector, below one vector
                          {TS_F32, 6, 0}, {TS_F32, 0, 0}, {TS_F32, -4, 0}, {TS_BF16, 4, 0}, {TS_BF16, 12, 0}};
    for (const Case& c : cases) {
        const NormPlan p = norm_plan(c.dtype, 5, c.d);
        CHECK(p.ok == (c.ln != 0), "dtype %d d %d", c.dtype, c.d);
        CHECK(p.vec == (c.dtype == TS_BF16 ? 8 : 4) && p.max_d == (c.dtype == TS_BF16 ? 2048 : 1024), "dtype %d: vec %d max %d", c.dtype, p.vec, p.max_d);
        if (p.ok) CHECK(p.ln == c.ln && p.grid == 2, "dtype %d d %d: ln %d grid %u", c.dtype, c.d, p.ln, p.grid);
    }
    const int64_t rows[] = {0, 1, 4, 5, 8192, 8193};
    const unsigned grids[] = {0, 1, 1, 2, 2048, 2049};
    for (int i = 0; i < 6; ++i) CHECK(norm_plan(TS_F32, rows[i], 768).grid == grids[i], "rows %lld", (long long)rows[i]);
    CHECK(!norm_plan(TS_F32, -1, 768).ok && norm_plan(TS_F32, 0, 768).ok, "rows < 0 is refused, rows == 0 is not");
}

static void pooling() {
    CHECK(pool_vec_form(TS_F32, 768, 32, true) && pool_vec_form(TS_BF16, 768, 32, true), "the encoders' widths");
    CHECK(pool_vec_form(TS_F32, 1024, 1024, true) && pool_vec_form(TS_BF16, 2048, 1, true), "256 vectors, 1024 tokens");
    CHECK(!pool_vec_form(TS_F32, 1028, 32, true) && !pool_vec_form(TS_BF16, 2056, 32, true), "257 vectors");
    CHECK(!pool_vec_form(TS_F32, 770, 32, true) && !pool_vec_form(TS_BF16, 772, 32, true), "not whole vectors");
    CHECK(!pool_vec_form(TS_F32, 768, 1025, true) && !pool_vec_form(TS_F32, 768, 32, false), "too long; unaligned");
    CHECK(kPoolVecSeq == 1024, "%d", kPoolVecSeq);
}

static void attention_short_and_gqa() {
    struct Case { int seq, tiles; bool rows; };   // tiles 0 = refused
    const Case cases[] = {{1, 1, false}, {16, 1, false}, {17, 2, false}, {64, 4, false}, {65, 5, true}, {128, 8, true}, {129, 0, false}};
    // what the kernels' LDS formulas give, per T: attention_rows_kernel (per wave, T = 5 .. 8), attention_gqa_kernel (per wave,
    // T = 1 .. 4), attention_gqa_rows_kernel (per workgroup, T = 5 .. 8 by R = 1, 2, 4), attention_short_kernel (static, per wave)
    const int rows_wave[9] = {0, 0, 0, 0, 0, 13312, 13312, 17408, 17408};
    const int gqa_wave[5] = {0, 11520, 12800, 25344, 27648};
    const int gqa_rows[9][3] = {{}, {}, {}, {}, {}, {30976, 35328, 44032}, {30976, 35328, 44032}, {39168, 43520, 52224}, {39168, 43520, 52224}};
    const int short_wave[5] = {0, 7424, 9728, 16128, 18432};
    for (int t = 1; t <= 4; ++t) CHECK(attn_wave_lds(t) == short_wave[t] && attn_gqa_wave_lds(t) == gqa_wave[t], "T %d", t);
    for (int t = 5; t <= 8; ++t) {
        CHECK(attn_rows_wave_lds(t) == rows_wave[t], "T %d: %d", t, attn_rows_wave_lds(t));
        for (int ri = 0; ri < 3; ++ri) CHECK(attn_gqa_rows_lds(t, 1 << ri) == gqa_rows[t][ri], "T %d R %d: %d", t, 1 << ri, attn_gqa_rows_lds(t, 1 << ri));
    }
    for (const Case& c : cases) {
        const AttnPlan s = attn_short_plan(256, c.seq, 12, 64);
        const AttnPlan g = attn_gqa_plan(256, c.seq, 16, 8, 128);
        CHECK(s.ok == (c.tiles != 0) && g.ok == (c.tiles != 0), "seq %d", c.seq);
        if (!s.ok || !g.ok) continue;
        CHECK(s.tiles == c.tiles && s.rows == c.rows && s.grid == 768 && s.block == 256, "short seq %d: T %d rows %d grid %u", c.seq, s.tiles, s.rows, s.grid);
        CHECK(s.lds == (c.rows ? 4 * rows_wave[c.tiles] : 0) && s.lds <= kCuLds, "short seq %d: lds %d", c.seq, s.lds);
        CHECK(g.tiles == c.tiles && g.rows == c.rows, "gqa seq %d: T %d rows %d", c.seq, g.tiles, g.rows);
        if (!c.rows) CHECK(g.grid == 1024 && g.block == 256 && g.lds == 4 * gqa_wave[c.tiles] && g.lds <= kCuLds, "gqa seq %d: grid %u lds %d", c.seq, g.grid, g.lds);
        else CHECK(g.r == 2 && g.grid == 2048 && g.block == 128 && g.lds == gqa_rows[c.tiles][1] && g.lds <= kCuLds, "gqa seq %d: R %d grid %u lds %d", c.seq, g.r, g.grid, g.lds);
    }
    CHECK(attn_short_plan(3, 20, 5, 64).grid == 4 && attn_gqa_plan(3, 20, 5, 5, 128).grid == 4, "ceil(15 / 4)");
    // the wrong head size is refused at any length
    for (int hd : {32, 128, 256}) CHECK(!attn_short_plan(2, 16, 4, hd).ok, "short head %d", hd);
    for (int hd : {32, 64, 256}) CHECK(!attn_gqa_plan(2, 16, 4, 2, hd).ok, "gqa head %d", hd);
    // R of the rows form: the largest of 4, 2, 1 that divides the query heads of a key / value head
    const int per_kv[] = {1, 2, 3, 4, 6, 8}, want_r[] = {1, 2, 1, 4, 2, 4};
    for (int i = 0; i < 6; ++i) {
        const AttnPlan g = attn_gqa_plan(2, 100, 2 * per_kv[i], 2, 128);
        CHECK(g.ok && g.rows && g.tiles == 7 && g.r == want_r[i], "per_kv %d: R %d", per_kv[i], g.r);
        CHECK(g.block == 64u * want_r[i] && g.grid == 4u * (per_kv[i] / want_r[i]), "per_kv %d: grid %u block %u", per_kv[i], g.grid, g.block);
        CHECK(g.lds == gqa_rows[7][want_r[i] == 4 ? 2 : want_r[i] - 1], "per_kv %d: lds %d", per_kv[i], g.lds);
        CHECK(attn_gqa_plan(2, 64, 2 * per_kv[i], 2, 128).r == 0, "up to 64 tokens there is no R");
    }
}

static void attention_float() {
    struct Case { int hd, max_seq, lds; };
    const Case cases[] = {{64, 512, 132096}, {128, 256, 133120}, {256, 128, 135168}};
    for (const Case& c : cases) {
        const AttnPlan p = attn_float_plan(3, c.max_seq, 5, c.hd);
        CHECK(p.ok && p.tiles == c.max_seq / 16 && p.grid == 15 && p.block == 256 && p.lds == c.lds, "head %d: T %d grid %u block %u lds %d", c.hd, p.tiles, p.grid, p.block, p.lds);
        CHECK(attn_f32_lds_limit(c.hd) == c.lds && c.lds <= kCuLds && attn_f32_max_seq(c.hd) == c.max_seq, "head %d: limit %d", c.hd, attn_f32_lds_limit(c.hd));
        CHECK(!attn_float_plan(3, c.max_seq + 1, 5, c.hd).ok, "head %d, one token past", c.hd);
        const int seqs[] = {1, 16, 17, 32, 33, 48, 49, 64, 65}, tiles[] = {1, 1, 2, 2, 3, 3, 4, 4, 5};
        for (int i = 0; i < 9; ++i) {
            const AttnPlan q = attn_float_plan(1, seqs[i], 1, c.hd);
            CHECK(q.ok && q.tiles == tiles[i] && q.block == 64u * (tiles[i] < 4 ? tiles[i] : 4) && q.grid == 1, "head %d seq %d: T %d block %u", c.hd, seqs[i], q.tiles, q.block);
            CHECK(q.lds == c.hd * (16 * tiles[i] + 4) * 4 && q.lds <= attn_f32_lds_limit(c.hd), "head %d seq %d: lds %d", c.hd, seqs[i], q.lds);
        }
    }
    for (int hd : {0, 32, 96, 512}) CHECK(!attn_float_plan(1, 16, 1, hd).ok, "head %d", hd);
}

static void grids() {
    // *_qk_norm_rope: 32 tokens of 4 + 2 heads = 192 (token, head) items
    CHECK(qk_norm_rope_grid(TS_F32, 32, 4, 2, 128) == 24 && qk_norm_rope_grid(TS_BF16, 32, 4, 2, 128) == 12, "head 128");
    CHECK(qk_norm_rope_grid(TS_F32, 32, 4, 2, 256) == 48 && qk_norm_rope_grid(TS_BF16, 32, 4, 2, 256) == 24, "head 256");
    CHECK(qk_norm_rope_grid(TS_BF16, 1, 1, 1, 128) == 1 && qk_norm_rope_grid(TS_F32, 1, 2, 1, 256) == 1, "a single item");
    CHECK(qk_norm_rope_grid(TS_BF16, 32768, 16, 8, 128) == 49152, "256 x 128 tokens of Qwen3");
    // the elementwise launches: 256 items per workgroup, at most 16384 workgroups (the kernels stride)
    const int64_t totals[] = {1, 256, 257, (int64_t)16384 * 256, (int64_t)16384 * 256 + 1, (int64_t)1 << 40};
    const unsigned want[] = {1, 1, 2, 16384, 16384, 16384};
    for (int i = 0; i < 6; ++i) CHECK(elementwise_grid(totals[i]) == want[i], "total %lld: %u", (long long)totals[i], elementwise_grid(totals[i]));
}

// a few thousand random shapes, good and bad: the invariants every accepted one keeps
static void sweep() {
    std::mt19937 rng(20240607);
    auto pick = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    int accepted = 0;
    for (int i = 0; i < 4000; ++i) {
        const int dtype = pick(0, 1), vec = dtype == TS_BF16 ? 8 : 4;
        const int d = pick(0, 9) == 0 ? pick(-16, 2200) : vec * pick(-1, 280);
        const int64_t rows = pick(0, 19) == 0 ? -pick(1, 5) : (pick(0, 3) == 0 ? (int64_t)pick(0, INT_MAX) * 8 : pick(0, 70000));
        const NormPlan p = norm_plan(dtype, rows, d);
        CHECK(p.ok == (rows >= 0 && d >= vec && d % vec == 0 && d <= 256 * vec), "dtype %d rows %lld d %d", dtype, (long long)rows, d);
        if (p.ok) {
            ++accepted;
            CHECK(p.ln == 1 || p.ln == 2 || p.ln == 4, "ln %d", p.ln);
            CHECK(p.ln * 64 * p.vec >= d && (p.ln == 1 || p.ln / 2 * 64 * p.vec < d), "dtype %d d %d: ln %d is not the smallest that covers the row", dtype, d, p.ln);
            CHECK((int64_t)p.grid * 4 >= rows && ((int64_t)p.grid - 1) * 4 < rows && (rows == 0 || p.grid >= 1), "rows %lld: grid %u", (long long)rows, p.grid);
        }
        const int hds[] = {32, 64, 128, 256, 512};
        const int hd = hds[pick(0, 4)], batch = pick(1, 4096), kv = pick(1, 8), per_kv = pick(1, 8), hq = kv * per_kv;
        const int seq = pick(0, 9) == 0 ? pick(600, INT_MAX) : pick(1, 600);
        const AttnPlan plans[3] = {attn_short_plan(batch, seq, hq, hd), attn_gqa_plan(batch, seq, hq, kv, hd), attn_float_plan(batch, seq, hq, hd)};
        const bool want_ok[3] = {hd == 64 && seq <= 128, hd == 128 && seq <= 128, (hd == 64 && seq <= 512) || (hd == 128 && seq <= 256) || (hd == 256 && seq <= 128)};
        for (int k = 0; k < 3; ++k) {
            const AttnPlan& a = plans[k];
            CHECK(a.ok == want_ok[k], "plan %d: head %d seq %d", k, hd, seq);
            if (!a.ok) continue;
            ++accepted;
            CHECK(a.lds >= 0 && a.lds <= kCuLds && a.grid >= 1 && a.block >= 64 && a.block <= 256 && a.block % 64 == 0, "plan %d: head %d seq %d: lds %d grid %u block %u", k, hd, seq, a.lds, a.grid, a.block);
            CHECK(16 * a.tiles >= seq && 16 * (a.tiles - 1) < seq && a.tiles >= 1 && a.tiles <= (k == 2 ? 32 : 8), "plan %d: seq %d T %d", k, seq, a.tiles);
            if (k < 2) CHECK(a.rows == (seq > 64), "plan %d seq %d", k, seq);
            // every (sequence, query head) has a wave: four to a workgroup, r to one of the gqa rows form, a workgroup each (float)
            const int64_t waves = (int64_t)a.grid * (k == 2 ? 1 : (k == 1 && a.rows) ? a.r : 4);
            CHECK(waves >= (int64_t)batch * hq && waves < (int64_t)batch * hq + 4, "plan %d: batch %d heads %d: grid %u", k, batch, hq, a.grid);
            if (k == 1 && a.rows) CHECK((a.r == 1 || a.r == 2 || a.r == 4) && per_kv % a.r == 0 && (a.r == 4 || per_kv % (2 * a.r) != 0) && a.block == 64u * a.r, "per_kv %d: R %d", per_kv, a.r);
            if (k == 2) CHECK(a.lds <= attn_f32_lds_limit(hd), "head %d seq %d: lds %d over the limit %d", hd, seq, a.lds, attn_f32_lds_limit(hd));
        }
        const int64_t total = (int64_t)pick(1, INT_MAX) * pick(1, 64);
        const unsigned g = elementwise_grid(total);
        CHECK(g >= 1 && g <= 16384 && (g == 16384 || ((int64_t)g * 256 >= total && ((int64_t)g - 1) * 256 < total)), "total %lld: %u", (long long)total, g);
        const int qhd = pick(0, 1) ? 256 : 128;
        const int64_t tokens = pick(1, 100000);
        const int64_t per_wg = 4 * (64 / (qhd / vec));
        const unsigned qg = qk_norm_rope_grid(dtype, tokens, hq, kv, qhd);
        CHECK(qg >= 1 && (int64_t)qg * per_wg >= tokens * (hq + kv) && ((int64_t)qg - 1) * per_wg < tokens * (hq + kv), "tokens %lld heads %d + %d head %d: %u", (long long)tokens, hq, kv, qhd, qg);
    }
    CHECK(accepted > 2000, "the sweep accepted only %d shapes", accepted);
}

int main() {
    norm_family();
    pooling();
    attention_short_and_gqa();
    attention_float();
    grids();
    sweep();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
