// Stand-alone check of ts_attention_tiled's host decisions in theoremsearch_amd/csrc/encoder_plan.h (kAttnTiledMaxSeq,
// kAttnTiledQueries, attn_tiled_chunk, attn_tiled_lds, attn_tiled_plan); tests/test_attn_tiled_plan_cpu.py builds it with the host
// compiler under -fsanitize=address,undefined and runs it.  Exit 0 = every check held; otherwise each failed check is printed.
// Expected values are literals.  The lines "chunk <head> <keys>" and "max_seq <tokens>" are what the Python side holds
// fused_forward._TILED_CHUNK / _TILED_MAX_SEQ against.
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

static void shapes() {
    struct Head { int hd, chunk, lds; };
    const Head heads[] = {{64, 128, 67584}, {128, 64, 69632}, {256, 32, 73728}};      // lds = 2 buffers x hd x (chunk + 4) floats
    CHECK(kAttnTiledMaxSeq == 32768 && kAttnTiledQueries == 64, "%d %d", kAttnTiledMaxSeq, kAttnTiledQueries);
    for (const Head& h : heads) {
        CHECK(attn_tiled_chunk(h.hd) == h.chunk && h.chunk % 16 == 0, "head %d: chunk %d", h.hd, attn_tiled_chunk(h.hd));
        CHECK(attn_tiled_lds(h.hd) == h.lds && h.lds <= 80 * 1024, "head %d: lds %d", h.hd, attn_tiled_lds(h.hd));
        // a chunk is staged in whole rounds of the workgroup's 256 threads, 16 bytes a thread
        CHECK(h.chunk * (h.hd / 4) % 256 == 0, "head %d", h.hd);
        struct Case { int seq, tiles, qblocks; };
        const Case cases[] = {{1, 1, 1}, {16, 1, 1}, {17, 2, 1}, {63, 4, 1}, {64, 4, 1}, {65, 5, 2},
                              {h.chunk - 1, (h.chunk + 14) / 16, (h.chunk + 62) / 64}, {h.chunk + 1, h.chunk / 16 + 1, h.chunk / 64 + 1},
                              {32768, 2048, 512}};
        for (const Case& c : cases) {
            const AttnTiledPlan p = attn_tiled_plan(3, c.seq, 5, h.hd);
            CHECK(p.ok && p.tiles == c.tiles && p.qblocks == c.qblocks, "head %d seq %d: ok %d T %d blocks %d", h.hd, c.seq, p.ok, p.tiles, p.qblocks);
            CHECK(p.grid == 15u * (unsigned)c.qblocks && p.block == 256 && p.lds == h.lds, "head %d seq %d: grid %u block %u lds %d", h.hd, c.seq, p.grid, p.block, p.lds);
        }
        // one token past the limit, and far past it
        CHECK(!attn_tiled_plan(3, 32769, 5, h.hd).ok && !attn_tiled_plan(1, INT_MAX, 1, h.hd).ok, "head %d past the limit", h.hd);
        // the grid must fit 31 bits: 2^22 x 512 blocks = 2^31 is refused, one (sequence, head) less is served
        CHECK(!attn_tiled_plan(1 << 20, 32768, 4, h.hd).ok, "head %d: 2^31 blocks", h.hd);
        const AttnTiledPlan big = attn_tiled_plan((1 << 22) - 1, 32768, 1, h.hd);
        CHECK(big.ok && big.grid == 2147483136u, "head %d: %u", h.hd, big.grid);
        const AttnTiledPlan edge = attn_tiled_plan(INT_MAX, 64, 1, h.hd);
        CHECK(edge.ok && edge.grid == 2147483647u && !attn_tiled_plan(INT_MAX, 65, 1, h.hd).ok, "head %d: 2^31 - 1 blocks", h.hd);
        CHECK(attn_tiled_plan(0, 100, 4, h.hd).ok && attn_tiled_plan(0, 100, 4, h.hd).grid == 0, "head %d: an empty batch", h.hd);
    }
    for (int hd : {0, 32, 96, 512}) {
        CHECK(!attn_tiled_plan(1, 16, 1, hd).ok && !attn_tiled_plan(1, 1000, 1, hd).ok, "head %d", hd);
        CHECK(attn_tiled_chunk(hd) == 0, "head %d", hd);
    }
    // where ts_attention_float serves a shape, so does ts_attention_tiled
    for (const Head& h : heads)
        for (int seq = 1; seq <= attn_f32_max_seq(h.hd); ++seq) CHECK(attn_tiled_plan(3, seq, 5, h.hd).ok, "head %d seq %d", h.hd, seq);
}

int main() {
    shapes();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    for (int hd : {64, 128, 256}) printf("chunk %d %d\n", hd, attn_tiled_chunk(hd));
    printf("max_seq %d\n", kAttnTiledMaxSeq);
    printf("all checks passed\n");
    return 0;
}
