// The full pass of the batched search for any row width the hand-laid kernels do not serve (anyd_plan.h: a multiple of 64
// from 128 up to a 4,096-byte row, other than 384 / 512 / 768 / 1024): rank_many_kernel's matrix pass (kernels_rank_mfma.h)
// with the threshold epilogue of the 16x16 full pass in place of the counting one.  The row length is a run-time value.
//
// The pass is a GEMM with M = corpus rows, N = queries, K = d:
//   * a staging tile is 16 RB corpus rows (RB = 4 while a row is at most 2,048 bytes, else 2), brought HBM -> LDS by LDS-DMA
//     (global_load_lds_dwordx4, 16 bytes per lane) and read from HBM once per launch; persistent workgroups walk contiguous
//     ranges of staging tiles;
//   * 8 waves per workgroup, two to a SIMD; the batch is cut into blocks of 16 queries, block j belongs to wave j % 8, so a
//     wave holds at most two blocks (256 queries per launch).  Per block the wave reads the query fragments from L2 in
//     segments of kAnydSeg k-steps, all of a segment in flight at once, and chains the MFMAs over the RB row blocks in LDS;
//   * arithmetic: v_mfma_f32_16x16x32_bf16 (bf16 rows) or v_mfma_f32_16x16x4_f32 (fp32 rows: float i of a 16-byte chunk times
//     float i of the matching query chunk, as sample_scores_kernel and rank_many_kernel).  D[i][j] = <row i, query j>: lane l
//     holds rows 4 (l >> 4) + {0..3} of each row block for query (l & 15) of its block.  A score is ONE chain of MFMAs over
//     the k-steps in ascending order, whatever the batch, the grid, the workgroup or the tile: the score bits of a (query,
//     row) pair depend on the width and the storage type only;
//   * k-steps come in groups of four (the 4 RB fragment reads of a group are issued before its MFMAs); a bf16 width with
//     d % 128 == 64 ends in a group of two - the steps past the row end are never multiplied (the row fragment there is the
//     next row's bytes or the padding, the query fragment a register nobody wrote);
//   * epilogue: a score s of row r is a candidate of query q when s >= thr[q], r < n and the filter (if any) allows r.  It is
//     appended to the query's shared list (count / cand of MfmaArgs) with one atomic - the direct form of
//     mfma16_append_block; the count may run past the cap, the final select then sends the query to the exact re-run.
//     Lane-private lists are not used (the select is told nwriters = 0).  NaN scores never pass.
//
// Full pass only: tile_stride == 1 and run == 1 (the host guarantees it); the kernel covers rows [0, 32 * ntiles), the
// allocation is padded to 256 rows, so whole staging tiles are in bounds.  It may be the first level of a search (a tiny
// index under algo = mfma): thresholds -inf, every real row a candidate.
#pragma once
#include "anyd_plan.h"
#include "kernels_mfma16_ops.h"

namespace ts {

constexpr int kAnydThreads = 512;    // 8 waves
constexpr int kAnydWaves = kAnydThreads / 64;
constexpr int kAnydNBW = kAnydQueries / 16 / kAnydWaves;   // query blocks per wave (2)
constexpr int kAnydSeg = 16;         // k-steps whose query fragments are in flight together

struct AnydArgs {
    MfmaArgs m;                      // the full pass's arguments as every matrix kernel takes them (m.q: storage dtype, row stride ld)
    int ld;                          // elements per row = d
};

template <bool F32, int RB>
__global__ void __launch_bounds__(kAnydThreads) mfma_anyd_kernel(AnydArgs aa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char srows[];
    const MfmaArgs& a = aa.m;
    constexpr int kRows = 16 * RB;
    constexpr int kElem = F32 ? 4 : 2;
    constexpr int kStepElems = F32 ? 16 : 32;                     // elements per k-step (16 bytes per lane and quarter)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int row_bytes = aa.ld * kElem;
    const int pitch = row_bytes + kAnydRowPad;
    const int steps = aa.ld / kStepElems;                         // even; fp32: a multiple of 4
    const int nblocks = (a.nq + 15) / 16;

    mfma_level_begin(a);
    // this workgroup's staging tiles of the rows [0, 32 * ntiles)
    const int64_t tiles = (a.ntiles * kTileRows + kRows - 1) / kRows;
    const int64_t t0 = tiles * (int64_t)blockIdx.x / gridDim.x;
    const int64_t t1 = tiles * (int64_t)(blockIdx.x + 1) / gridDim.x;
    if (t0 >= t1) return;

    int qid[kAnydNBW];
    float thr[kAnydNBW];
#pragma unroll
    for (int b = 0; b < kAnydNBW; ++b) {
        qid[b] = (wave + kAnydWaves * b) * 16 + r16;
        thr[b] = mfma_level_thr(a, qid[b]);
    }

    const unsigned lds_base = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)srows;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int per_row = row_bytes / 16;
    const unsigned char* arow[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) arow[rb] = srows + (16 * rb + r16) * pitch + kq * 16;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t p0 = t * kRows;                             // first row of the tile
        __syncthreads();                                          // the previous tile's fragment reads are done
        // rows -> LDS: wave w moves rows w, w + 8, ... in pieces of 64 lanes x 16 bytes, all in flight before one wait
        for (int r = wv; r < kRows; r += kAnydWaves) {
            const unsigned char* src = (const unsigned char*)a.corpus + (p0 + r) * row_bytes;   // < n_pad: padded to kRowPad rows
            for (int pc = 0; pc * 64 < per_row; ++pc) {
                const int c = pc * 64 + lane;
                if (c < per_row) lds_dma16(src + c * 16, lds_base + r * pitch + pc * 1024);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

#pragma unroll
        for (int b = 0; b < kAnydNBW; ++b) {
            const int blk = wave + kAnydWaves * b;
            if (blk >= nblocks) continue;                         // wave-uniform
            const unsigned char* brow = (const unsigned char*)a.q + ((int64_t)qid[b] * aa.ld + (F32 ? 4 : 8) * kq) * kElem;
            f32x4 acc[RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int s0 = 0; s0 < steps; s0 += kAnydSeg) {
                uint4 bv[kAnydSeg];
#pragma unroll
                for (int s = 0; s < kAnydSeg; ++s)
                    if (s0 + s < steps) bv[s] = *(const uint4*)(brow + (int64_t)(s0 + s) * 64);
#pragma unroll
                for (int g4 = 0; g4 < kAnydSeg; g4 += 4) {
                    if (s0 + g4 < steps) {
                        const bool full = F32 || s0 + g4 + 4 <= steps;        // bf16, d % 128 == 64: the last group has two steps
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
            // lane holds rows p0 + 16 rb + 4 kq + {0..3} for query qid[b]
            bool any = false;
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int g = 0; g < 4; ++g) any |= acc[rb][g] >= thr[b];
            if (__ballot(any)) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float s = acc[rb][g];
                        const int64_t row = p0 + 16 * rb + 4 * kq + g;
                        // padding rows of the last tile, and the metadata filter: tested only for scores that pass the threshold
                        if (s >= thr[b] && row < a.n && (!a.row_mask || ((a.row_mask[row >> 5] >> (row & 31)) & 1u))) {
                            const u32 pos = atomicAdd(&a.count[qid[b]], 1u);
                            if (pos < (u32)a.cap) a.cand[(int64_t)qid[b] * a.cap + pos] = make_key(s, (u32)row);
                        }
                    }
            }
        }
    }
}

}  // namespace ts
