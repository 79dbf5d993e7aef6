// Stand-alone check of ts_attention_flash's host decisions in theoremsearch_amd/csrc/encoder_plan.h (kAttnBf16TiledMaxSeq,
// kAttnBf16TiledQueries, attn_bf16_tiled_chunk, attn_bf16_tiled_lds, attn_bf16_tiled_plan); tests/test_attn_bf16_plan_cpu.py builds it
// with the host compiler under -fsanitize=address,undefined and runs it.  Exit 0 = every check held; otherwise each failed check
// is printed.  Expected values are literals or formulas re-stated here.  The lines "chunk <head> <keys>" and "max_seq <tokens>" are
// what the Python side holds fused_forward._BF16_TILED_CHUNK / _BF16_TILED_MAX_SEQ against.
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

struct Head { int hd, chunk, lds; };
// lds = 2 buffers x chunk keys x (K row of hd + 8 elements + V row of hd + 16 elements) x 2 bytes
static const Head kHeads[] = {{64, 128, 77824}, {128, 64, 71680}, {256, 32, 68608}};

static void shapes() {
    CHECK(kAttnBf16TiledMaxSeq == 32768 && kAttnBf16TiledQueries == 64, "%d %d", kAttnBf16TiledMaxSeq, kAttnBf16TiledQueries);
    for (const Head& h : kHeads) {
        CHECK(attn_bf16_tiled_chunk(h.hd) == h.chunk && h.chunk % 32 == 0, "head %d: chunk %d", h.hd, attn_bf16_tiled_chunk(h.hd));
        CHECK(h.chunk * h.hd * 2 == 16 * 1024, "head %d: 16 KiB of K and of V per buffer", h.hd);
        CHECK(attn_bf16_tiled_lds(h.hd) == h.lds && h.lds == 2 * h.chunk * ((h.hd + 8) + (h.hd + 16)) * 2, "head %d: lds %d", h.hd, attn_bf16_tiled_lds(h.hd));
        CHECK(2 * h.lds <= 160 * 1024 && h.lds <= 80 * 1024, "head %d: two workgroups per CU", h.hd);
        // rows of 16-byte pieces, 8-byte aligned transposed reads; the four waves' output tiles fit the buffers
        CHECK((attn_bf16_tiled_k_pitch(h.hd) * 2) % 16 == 0 && (attn_bf16_tiled_v_pitch(h.hd) * 2) % 16 == 0, "head %d: pitches", h.hd);
        CHECK(4 * 16 * (h.hd + 8) * 2 <= h.lds, "head %d: output tiles", h.hd);
        // a chunk is staged in whole rounds of the workgroup's 256 threads, 16 bytes a thread and matrix
        CHECK(h.chunk * (h.hd / 8) % 256 == 0, "head %d", h.hd);
        struct Case { int seq, tiles, qblocks; };
        const Case cases[] = {{1, 1, 1}, {16, 1, 1}, {17, 2, 1}, {63, 4, 1}, {64, 4, 1}, {65, 5, 2},
                              {h.chunk - 1, (h.chunk + 14) / 16, (h.chunk + 62) / 64}, {h.chunk + 1, h.chunk / 16 + 1, h.chunk / 64 + 1},
                              {32768, 2048, 512}};
        for (const Case& c : cases) {
            const AttnTiledPlan p = attn_bf16_tiled_plan(3, c.seq, 5, h.hd);
            CHECK(p.ok && p.tiles == c.tiles && p.qblocks == c.qblocks, "head %d seq %d: ok %d T %d blocks %d", h.hd, c.seq, p.ok, p.tiles, p.qblocks);
            CHECK(p.grid == 15u * (unsigned)c.qblocks && p.block == 256 && p.lds == h.lds, "head %d seq %d: grid %u block %u lds %d", h.hd, c.seq, p.grid, p.block, p.lds);
        }
        // every length: the re-stated formulas
        for (int seq = 1; seq <= 32768; seq += (seq < 300 ? 1 : 61)) {
            const AttnTiledPlan p = attn_bf16_tiled_plan(2, seq, 3, h.hd);
            const int tiles = (seq + 15) / 16, qblocks = (seq + 63) / 64;
            CHECK(p.ok && p.tiles == tiles && p.qblocks == qblocks && p.grid == 6u * (unsigned)qblocks && p.block == 256 && p.lds == h.lds,
                  "head %d seq %d", h.hd, seq);
        }
        // no token, one token past the limit, and far past it
        CHECK(!attn_bf16_tiled_plan(3, 0, 5, h.hd).ok && !attn_bf16_tiled_plan(3, -1, 5, h.hd).ok, "head %d: seq < 1", h.hd);
        CHECK(!attn_bf16_tiled_plan(3, 32769, 5, h.hd).ok && !attn_bf16_tiled_plan(1, INT_MAX, 1, h.hd).ok, "head %d past the limit", h.hd);
        CHECK(!attn_bf16_tiled_plan(-1, 16, 5, h.hd).ok && !attn_bf16_tiled_plan(3, 16, 0, h.hd).ok, "head %d: bad counts", h.hd);
        // the grid must fit 31 bits: 2^22 x 512 blocks = 2^31 is refused, one (sequence, head) less is served
        CHECK(!attn_bf16_tiled_plan(1 << 20, 32768, 4, h.hd).ok, "head %d: 2^31 blocks", h.hd);
        const AttnTiledPlan big = attn_bf16_tiled_plan((1 << 22) - 1, 32768, 1, h.hd);
        CHECK(big.ok && big.grid == 2147483136u, "head %d: %u", h.hd, big.grid);
        const AttnTiledPlan edge = attn_bf16_tiled_plan(INT_MAX, 64, 1, h.hd);
        CHECK(edge.ok && edge.grid == 2147483647u && !attn_bf16_tiled_plan(INT_MAX, 65, 1, h.hd).ok, "head %d: 2^31 - 1 blocks", h.hd);
        CHECK(attn_bf16_tiled_plan(0, 100, 4, h.hd).ok && attn_bf16_tiled_plan(0, 100, 4, h.hd).grid == 0, "head %d: an empty batch", h.hd);
    }
    for (int hd : {0, 32, 96, 512}) {
        CHECK(!attn_bf16_tiled_plan(1, 16, 1, hd).ok && !attn_bf16_tiled_plan(1, 1000, 1, hd).ok, "head %d", hd);
        CHECK(attn_bf16_tiled_chunk(hd) == 0, "head %d", hd);
    }
}

// attention_bf16_tiled_kernel's walk, re-stated: what a block and each of its four waves execute.  THE BARRIER RULE: the chunk count
// (barriers = nchunk + 1) is a function of (block, S) alone - no wave's own state enters it - and every wave's key tiles lie inside
// the chunks its block walks.
static int nchunk_of(int hd, bool causal, int seq, int qblk) {
    const int ct = attn_bf16_tiled_chunk(hd) / 16, T = (seq + 15) / 16;
    const int kt_blk = causal ? std::min(4 * qblk + 4, T) : T;
    return (kt_blk + ct - 1) / ct;
}

static void barriers() {
    for (const Head& h : kHeads) {
        const int ct = h.chunk / 16;
        for (int causal = 0; causal < 2; ++causal)
            for (int seq = 1; seq <= 2200; seq += (seq < 600 ? 1 : 37)) {
                const AttnTiledPlan p = attn_bf16_tiled_plan(1, seq, 1, h.hd);
                const int T = p.tiles;
                int64_t multiplied = 0;
                for (int qblk = 0; qblk < p.qblocks; ++qblk) {
                    const int nchunk = nchunk_of(h.hd, causal != 0, seq, qblk);
                    CHECK(nchunk >= 1 && nchunk <= (T + ct - 1) / ct, "head %d causal %d seq %d block %d: %d chunks", h.hd, causal, seq, qblk, nchunk);
                    if (!causal) CHECK(nchunk == (seq + h.chunk - 1) / h.chunk, "head %d seq %d block %d", h.hd, seq, qblk);
                    // causal: the chunk that holds the block's last query's key (or the sequence's last key) is the last one walked
                    if (causal) CHECK(nchunk == std::min(64 * qblk + 63, seq - 1) / h.chunk + 1, "head %d seq %d block %d: %d", h.hd, seq, qblk, nchunk);
                    for (int wave = 0; wave < 4; ++wave) {
                        const int qi = 4 * qblk + wave;
                        const int kt_end = qi < T ? (causal ? qi + 1 : T) : 0;
                        CHECK(kt_end <= nchunk * ct, "head %d causal %d seq %d block %d wave %d: key tiles past the block's chunks", h.hd, causal, seq, qblk, wave);
                        // the tiles the wave multiplies chunk by chunk add up to kt_end: none skipped, none twice
                        int walked = 0;
                        for (int c = 0; c < nchunk; ++c) walked += std::max(0, std::min(ct, kt_end - c * ct));
                        CHECK(walked == kt_end, "head %d causal %d seq %d block %d wave %d: %d of %d", h.hd, causal, seq, qblk, wave, walked, kt_end);
                        multiplied += walked;
                    }
                }
                const int64_t want = causal ? (int64_t)T * (T + 1) / 2 : (int64_t)T * T;
                CHECK(multiplied == want, "head %d causal %d seq %d: %lld tile products", h.hd, causal, seq, (long long)multiplied);
            }
    }
}

int main() {
    shapes();
    barriers();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    for (int hd : {64, 128, 256}) printf("chunk %d %d\n", hd, attn_bf16_tiled_chunk(hd));
    printf("max_seq %d\n", kAttnBf16TiledMaxSeq);
    printf("all checks passed\n");
    return 0;
}
