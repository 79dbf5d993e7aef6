// Ranks of many target rows per query (ts_rank_many, ts_count_above_many) at the k-chunked row widths (rank_wide_plan.h:
// d % 256 == 0, a row of more than 4,096 and at most 16,384 bytes - bf16 d = 2,304 .. 8,192, fp32 d = 1,280 .. 4,096):
// mfma_wide_kernel's chunk loop (kernels_mfma_wide.h) with rank_many_kernel's two epilogues (kernels_rank_mfma.h).
//
// From the k-chunked search, unchanged: a staging tile is 64 rows x ONE k-chunk of 1,024 bytes (the last chunk of a bf16 row
// with d % 512 == 256 is 512 bytes, the upper 32 lanes of its DMA instructions masked off), a chunk of a row is one LDS-DMA wave
// instruction (lds_dma16), LDS pitch 1,040; two LDS buffers used in turn by consecutive chunks, the turn carrying on across
// tiles (bf16 2,304 / 2,560 and fp32 1,280 have an odd number of chunks); per chunk DMA, s_waitcnt vmcnt(0), ONE barrier,
// MFMAs - behind the barrier every wave's pieces of this chunk have landed and every wave has consumed its fragment reads of
// the previous chunk, whose buffer the next chunk's DMA writes.  Loop order tile -> chunk -> query block, acc[2][4] carried
// across the chunks of a tile, the epilogue once per tile behind the last chunk.  A score is ONE chain of MFMAs over the
// k-steps in ascending order across the chunk boundaries, by the same builtins at the same fragment lanes with the same query
// addressing as the search's pass: the bits of a score are those the search returns for that row.
//
// From the rank pass, unchanged: RankManyArgs; GATHER fills LDS row r of the tile from grow[p0 + r] (a slot past nslots reads
// row 0, its score is dropped) and writes gscore[s] where gquery[s] is the lane's query - only which rows fill the tile
// differs from the counting pass, so a target's score is bit-identical to the score counted for that row; counting: fast
// reject against the worst target's score, row < n, make_key, kRankT compares into register counters carried across the
// workgroup's whole range of tiles, a shuffle-sum over the four lanes of a query and one atomicAdd per (workgroup, query,
// target) at the end.  NaN scores and padding rows never count.  One difference in form, none in result: the compares run
// over all kRankT keys without the j < tcount test (the padding keys are ~0, which no key beats), so no SGPR is spilled.
//
// Barriers: every wave of a workgroup executes nchunks barriers per tile of its range, whatever its query blocks: the
// wave-uniform blk >= nblocks test skips MFMAs and the epilogue, never a barrier.  A counting workgroup without a tile returns
// before the first one (a gather workgroup always has its one tile).  The counting pass covers whole 64-row tiles of an
// allocation padded to 256 rows; the gather pass reads real rows only.
#pragma once
#include "kernels_mfma_wide.h"
#include "kernels_rank_mfma.h"
#include "rank_wide_plan.h"

namespace ts {

static_assert(kRankThreads == kWideThreads && kRankNBW == kWideNBW, "the rank pass's waves and query blocks are the k-chunked search's");

template <bool F32, bool GATHER>
__global__ void __launch_bounds__(kWideThreads) rank_wide_kernel(RankManyArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char srows[];
    constexpr int RB = kWideRB;
    constexpr int kElem = F32 ? 4 : 2;
    constexpr int kRowsPerWave = kWideTileRows / kWideWaves;      // 8: wave w moves rows w, w + 8, ...
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int row_bytes = a.ld * kElem;
    const int nchunks = wide_chunks(row_bytes);
    const int nblocks = (a.nq + 15) / 16;

    // this workgroup's tiles
    int64_t t0, t1;
    if constexpr (GATHER) {
        t0 = blockIdx.x;
        t1 = t0 + 1;
    } else {
        t0 = a.ntiles * (int64_t)blockIdx.x / gridDim.x;
        t1 = a.ntiles * (int64_t)(blockIdx.x + 1) / gridDim.x;
        if (t0 >= t1) return;                                     // before the first barrier; nothing counted, nothing to flush
    }

    // per (block, lane): the query, the fast-reject threshold, the counters
    int qid[kWideNBW];
    float thr[kWideNBW];
    int tc[kWideNBW];
    u32 cnt[kWideNBW][kRankT];
#pragma unroll
    for (int b = 0; b < kWideNBW; ++b) {
        qid[b] = (wave + kWideWaves * b) * 16 + r16;
        const bool real = qid[b] < a.nq;
        thr[b] = (!GATHER && real) ? a.tworst[qid[b]] : __builtin_nanf("");
        tc[b] = (!GATHER && real) ? a.tcount[qid[b]] : 0;
#pragma unroll
        for (int j = 0; j < kRankT; ++j) cnt[b][j] = 0;
    }

    const unsigned lds_base = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)srows;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int frag_off[RB];                                             // this lane's fragment of k-step 0 in row block rb of a buffer
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) frag_off[rb] = (16 * rb + r16) * kWidePitch + kq * 16;
    int buf = 0;                                                  // the buffer of the chunk at hand: workgroup-uniform

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t p0 = t * kWideTileRows;                     // first row (counting) or slot (gather) of the tile
        // the rows this wave moves, once per tile (wave-uniform): LDS row wv + 8 i <- corpus row rowi[i]
        int64_t rowi[kRowsPerWave];
#pragma unroll
        for (int i = 0; i < kRowsPerWave; ++i) {
            const int64_t s = p0 + wv + i * kWideWaves;
            if constexpr (GATHER) rowi[i] = s < a.nslots ? a.grow[s] : 0;   // slots past the list read row 0; their scores are dropped
            else rowi[i] = s;                                     // < n_pad: the allocation is padded to kRowPad rows
        }
        f32x4 acc[kWideNBW][RB];
#pragma unroll
        for (int b = 0; b < kWideNBW; ++b)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) acc[b][rb] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int c = 0; c < nchunks; ++c) {
            const int cbytes = wide_chunk_bytes(row_bytes, c);    // 1,024, or 512 for a ragged last chunk
            // chunk c of the tile's rows -> LDS, one instruction a row (1,024 c + 16 lane + 16 <= row_bytes for the lanes that
            // take part)
            {
                const unsigned char* src = (const unsigned char*)a.corpus + c * kWideChunkBytes + lane * 16;
                const unsigned dst = lds_base + buf * kWideBufBytes + wv * kWidePitch;
                if (lane * 16 < cbytes) {
#pragma unroll
                    for (int i = 0; i < kRowsPerWave; ++i) lds_dma16(src + rowi[i] * row_bytes, dst + i * kWideWaves * kWidePitch);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();

            const unsigned char* tile = srows + buf * kWideBufBytes;
            const int steps = cbytes / 64;                        // 16 or 8: whole groups of four
#pragma unroll
            for (int b = 0; b < kWideNBW; ++b) {
                const int blk = wave + kWideWaves * b;
                if (blk >= nblocks) continue;                     // wave-uniform; skips no barrier
                const unsigned char* brow =
                    (const unsigned char*)a.q + ((int64_t)qid[b] * a.ld + (F32 ? 4 : 8) * kq) * kElem + c * kWideChunkBytes;
                uint4 bv[kWideSteps];
#pragma unroll
                for (int s = 0; s < kWideSteps; ++s)
                    if (s < steps) bv[s] = *(const uint4*)(brow + s * 64);
#pragma unroll
                for (int g4 = 0; g4 < kWideSteps; g4 += 4) {
                    if (g4 < steps) {
                        uint4 av[4][RB];
#pragma unroll
                        for (int s = 0; s < 4; ++s)
#pragma unroll
                            for (int rb = 0; rb < RB; ++rb) av[s][rb] = *(const uint4*)(tile + frag_off[rb] + (g4 + s) * 64);
#pragma unroll
                        for (int s = 0; s < 4; ++s)
#pragma unroll
                            for (int rb = 0; rb < RB; ++rb) {
                                if constexpr (F32) {
                                    const float* af = reinterpret_cast<const float*>(&av[s][rb]);
                                    const float* bf = reinterpret_cast<const float*>(&bv[g4 + s]);
#pragma unroll
                                    for (int i = 0; i < 4; ++i)
                                        acc[b][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[i], acc[b][rb], 0, 0, 0);
                                } else {
                                    acc[b][rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(reinterpret_cast<const bf16x8&>(av[s][rb]),
                                                                                         reinterpret_cast<const bf16x8&>(bv[g4 + s]),
                                                                                         acc[b][rb], 0, 0, 0);
                                }
                            }
                    }
                }
            }
            buf ^= 1;
        }

        // lane holds rows (slots) p0 + 16 rb + 4 kq + {0..3} for query qid[b]
#pragma unroll
        for (int b = 0; b < kWideNBW; ++b) {
            const int blk = wave + kWideWaves * b;
            if (blk >= nblocks) continue;
            if constexpr (GATHER) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int64_t s = p0 + 16 * rb + 4 * kq + g;
                        if (s < a.nslots && a.gquery[s] == qid[b]) a.gscore[s] = acc[b][rb][g];
                    }
            } else {
                // fast reject: below the worst target's score (NaN scores and an empty list fail every comparison)
                bool any = false;
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) any |= acc[b][rb][g] >= thr[b];
                if (__ballot(any)) {
                    const u64* tk = a.tkeys + (int64_t)qid[b] * kRankT;
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const float s = acc[b][rb][g];
                            const int64_t row = p0 + 16 * rb + 4 * kq + g;
                            if (s >= thr[b] && row < a.n) {
                                const u64 key = make_key(s, (u32)row);
                                // every one of the kRankT keys: the host pads the list with ~0, a key nothing beats, so no
                                // j < tc[b] test here (its sixteen lane masks per block, hoisted out of the tile loop, are
                                // what spills SGPRs in rank_many_kernel); the flush below still looks at real targets only
#pragma unroll
                                for (int j = 0; j < kRankT; ++j) cnt[b][j] += key > tk[j] ? 1u : 0u;
                            }
                        }
                }
            }
        }
    }

    if constexpr (!GATHER) {
        // the four lanes of a query (l, l + 16, l + 32, l + 48) -> one atomic per (query, target) with a non-zero count
#pragma unroll
        for (int b = 0; b < kWideNBW; ++b) {
#pragma unroll
            for (int j = 0; j < kRankT; ++j) {
                u32 c = cnt[b][j];
                c += __shfl_xor(c, 16, 64);
                c += __shfl_xor(c, 32, 64);
                if (kq == 0 && j < tc[b] && c) atomicAdd(a.counts + (int64_t)qid[b] * kRankT + j, c);
            }
        }
    }
}

}  // namespace ts
