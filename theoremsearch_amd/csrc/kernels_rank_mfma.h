// Ranks of many target rows per query (ts_rank_many): one matrix pass over the corpus for a block of up to 256 queries,
// with a counting epilogue in place of the top-k epilogue of kernels_mfma16.h.
//
// The pass is a GEMM with M = corpus rows, N = queries, K = d:
//   * a tile is kRankRows(RB) = 16 RB corpus rows, brought HBM -> LDS by LDS-DMA (global_load_lds_dwordx4, 16 bytes per
//     lane) and read from HBM once; persistent workgroups (one per CU) walk contiguous tile ranges;
//   * 8 waves per workgroup, two to a SIMD; the batch is cut into blocks of 16 queries, block j belongs to wave j % 8, so a
//     wave holds at most two blocks.  Per block the wave reads the query fragments from L2 (the whole batch is 393 KB at
//     d = 768 bf16; every workgroup reads the same bytes) in segments of kRankSeg k-steps, all of a segment in flight at
//     once, and chains the MFMAs over the RB row blocks of the tile in LDS;
//   * arithmetic: v_mfma_f32_16x16x32_bf16 (bf16 rows) or v_mfma_f32_16x16x4_f32 (fp32 rows: float i of a 16-byte chunk times
//     float i of the matching query chunk, as sample_scores_kernel in kernels_sample.h).  D[i][j] = <row i, query j>:
//     lane l holds rows 4 (l >> 4) + {0..3} of each row block for query (l & 15) of the block.
//
// Two modes of the same code (GATHER template flag), so that a target's score is bit-identical to the score the counting
// pass computes for that row (same query fragments at the same lanes, same K loop, same MFMA chain; only which rows fill
// the A tile differs):
//   * GATHER: the A tile is filled from a list of local row ids (one slot per target, the DMA addresses are per lane) and
//     the score of slot s for its own query is written to gscore[s];
//   * counting: per query the host hands in up to kRankT target keys (make_key, common.h), sorted best-first and padded
//     with ~0 (a key nothing beats), and the score of the worst one.  A score below that is rejected at once (the common
//     case for shallow targets); a score that passes compares its key with every target key and adds 1 to a per-lane
//     counter per target it beats.  counts[q][j] = the number of rows whose key beats target j = its rank.  The counters
//     live in registers (no atomics per score, so a target at depth N / 2, which sends every score down the slow path,
//     costs kRankT compares per score), are summed over the four lanes of a query by shuffles and flushed with one global
//     atomic per (workgroup, query, target) at the end.  NaN scores and padding rows never count.
#pragma once
#include "kernels_mfma16_ops.h"
#include "rank_plan.h"

namespace ts {

// kRankT, kRankRowPad, the served widths, RB and the LDS bytes of a launch: rank_plan.h
constexpr int kRankThreads = 512;    // 8 waves
constexpr int kRankWaves = kRankThreads / 64;
constexpr int kRankNBW = kRankQueries / 16 / kRankWaves;   // query blocks per wave (2)
constexpr int kRankSeg = 16;         // k-steps whose query fragments are in flight together

struct RankManyArgs {
    const void* corpus;       // [n_pad x ld] storage dtype
    int64_t n;                // real rows
    int ld;                   // elements per row = d (rank_many_served: a multiple of 64)
    const void* q;            // prepared queries in the storage dtype, [256 x ld]
    int nq;                   // queries of this block (<= 256)
    // counting pass
    int64_t ntiles;           // tiles covering [0, n)
    const u64* tkeys;         // [nq][kRankT] target keys, best first, padded with ~0
    const int* tcount;        // [nq] real targets
    const float* tworst;      // [nq] score of the worst target (NaN: no target)
    u32* counts;              // [nq][kRankT] rows beating each target (zeroed by the caller)
    // gather pass
    const int64_t* grow;      // [nslots] local row of each slot
    const int* gquery;        // [nslots] query (within the block) of each slot
    int64_t nslots;
    float* gscore;            // [nslots]
};

// TAIL: a bf16 width with d % 128 == 64, whose k-steps end in a group of two (rank_tail, rank_plan.h).  A template flag and
// not a test of `steps` alone: the test in every group costs the widths without a tail 57 VGPRs and 8 % of the pass
// (3M x 768 bf16, 256 queries: 3.37 against 3.13 ms); with TAIL = false their kernels are the ones they always had.
template <bool F32, int RB, bool GATHER, bool TAIL = false>
__global__ void __launch_bounds__(kRankThreads) rank_many_kernel(RankManyArgs a) {
    static_assert(!(F32 && TAIL), "fp32: d / 16 steps, a multiple of 4");
    extern __shared__ __attribute__((aligned(16))) unsigned char srows[];
    constexpr int kRows = 16 * RB;
    constexpr int kElem = F32 ? 4 : 2;
    constexpr int kStepElems = F32 ? 16 : 32;                     // elements per k-step (16 bytes per lane and quarter)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int row_bytes = a.ld * kElem;
    const int pitch = row_bytes + kRankRowPad;
    const int steps = a.ld / kStepElems;                          // even; fp32: a multiple of 4
    const int nblocks = (a.nq + 15) / 16;

    // this workgroup's tiles
    int64_t t0, t1;
    if constexpr (GATHER) {
        t0 = blockIdx.x;
        t1 = t0 + 1;
    } else {
        t0 = a.ntiles * (int64_t)blockIdx.x / gridDim.x;
        t1 = a.ntiles * (int64_t)(blockIdx.x + 1) / gridDim.x;
    }

    // per (block, lane): the query, the fast-reject threshold, the counters
    int qid[kRankNBW];
    float thr[kRankNBW];
    int tc[kRankNBW];
    u32 cnt[kRankNBW][kRankT];
#pragma unroll
    for (int b = 0; b < kRankNBW; ++b) {
        qid[b] = (wave + kRankWaves * b) * 16 + r16;
        const bool real = qid[b] < a.nq;
        thr[b] = (!GATHER && real) ? a.tworst[qid[b]] : __builtin_nanf("");
        tc[b] = (!GATHER && real) ? a.tcount[qid[b]] : 0;
#pragma unroll
        for (int j = 0; j < kRankT; ++j) cnt[b][j] = 0;
    }

    const unsigned lds_base = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)srows;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int per_row = row_bytes / 16;
    const unsigned char* arow[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) arow[rb] = srows + (16 * rb + r16) * pitch + kq * 16;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t p0 = t * kRows;                             // first row (counting) or slot (gather) of the tile
        __syncthreads();                                          // the previous tile's fragment reads are done
        // rows -> LDS: wave w moves rows w, w + 8, ... in pieces of 64 lanes x 16 bytes, all in flight before one wait
        for (int r = wv; r < kRows; r += kRankWaves) {
            int64_t row;
            if constexpr (GATHER) {
                const int64_t s = p0 + r;
                row = s < a.nslots ? a.grow[s] : 0;               // slots past the list read row 0; their scores are dropped
            } else {
                row = p0 + r;                                     // < n_pad: the allocation is padded to kRowPad rows
            }
            const unsigned char* src = (const unsigned char*)a.corpus + row * row_bytes;
            for (int pc = 0; pc * 64 < per_row; ++pc) {
                const int c = pc * 64 + lane;
                if (c < per_row) lds_dma16(src + c * 16, lds_base + r * pitch + pc * 1024);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

#pragma unroll
        for (int b = 0; b < kRankNBW; ++b) {
            const int blk = wave + kRankWaves * b;
            if (blk >= nblocks) continue;                         // wave-uniform
            const unsigned char* brow = (const unsigned char*)a.q + ((int64_t)qid[b] * a.ld + (F32 ? 4 : 8) * kq) * kElem;
            f32x4 acc[RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int s0 = 0; s0 < steps; s0 += kRankSeg) {
                uint4 bv[kRankSeg];
#pragma unroll
                for (int s = 0; s < kRankSeg; ++s)
                    if (s0 + s < steps) bv[s] = *(const uint4*)(brow + (int64_t)(s0 + s) * 64);
#pragma unroll
                for (int g4 = 0; g4 < kRankSeg; g4 += 4) {
                    if (s0 + g4 < steps) {
                        // TAIL (bf16, d % 128 == 64): the last group has two steps (as kernels_mfma_anyd_pass.inc).  Nothing past the
                        // row end is read - behind the tile's last row lies the end of the LDS allocation - or multiplied
                        const bool full = !TAIL || s0 + g4 + 4 <= steps;
                        uint4 av[4][RB];
#pragma unroll
                        for (int s = 0; s < 4; ++s)
#pragma unroll
                            for (int rb = 0; rb < RB; ++rb)
                                if (s < 2 || full) av[s][rb] = *(const uint4*)(arow[rb] + (s0 + g4 + s) * 64);
#pragma unroll
                        for (int s = 0; s < 4; ++s)
#pragma unroll
                            for (int rb = 0; rb < RB; ++rb) {
                                if constexpr (F32) {
                                    const float* af = reinterpret_cast<const float*>(&av[s][rb]);
                                    const float* bf = reinterpret_cast<const float*>(&bv[g4 + s]);
#pragma unroll
                                    for (int i = 0; i < 4; ++i)
                                        acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[i], acc[rb], 0, 0, 0);
                                } else {
                                    if (s < 2 || full)
                                        acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(reinterpret_cast<const bf16x8&>(av[s][rb]),
                                                                                          reinterpret_cast<const bf16x8&>(bv[g4 + s]),
                                                                                          acc[rb], 0, 0, 0);
                                }
                            }
                    }
                }
            }
            if constexpr (GATHER) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int64_t s = p0 + 16 * rb + 4 * kq + g;
                        if (s < a.nslots && a.gquery[s] == qid[b]) a.gscore[s] = acc[rb][g];
                    }
            } else {
                // fast reject: below the worst target's score (NaN scores and an empty list fail every comparison)
                bool any = false;
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) any |= acc[rb][g] >= thr[b];
                if (__ballot(any)) {
                    const u64* tk = a.tkeys + (int64_t)qid[b] * kRankT;
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const float s = acc[rb][g];
                            const int64_t row = p0 + 16 * rb + 4 * kq + g;
                            if (s >= thr[b] && row < a.n) {
                                const u64 key = make_key(s, (u32)row);
#pragma unroll
                                for (int j = 0; j < kRankT; ++j)
                                    if (j < tc[b]) cnt[b][j] += key > tk[j] ? 1u : 0u;
                            }
                        }
                }
            }
        }
    }

    if constexpr (!GATHER) {
        // the four lanes of a query (l, l + 16, l + 32, l + 48) -> one atomic per (query, target) with a non-zero count
#pragma unroll
        for (int b = 0; b < kRankNBW; ++b) {
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
