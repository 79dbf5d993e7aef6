// The full pass of the batched search for rows wider than the general-width kernel stages whole (wide_plan.h: d % 256 == 0, a
// row of more than 4,096 and at most 16,384 bytes - bf16 d = 2,304 .. 8,192, fp32 d = 1,280 .. 4,096): mfma_anyd_kernel's pass
// (kernels_mfma_anyd.h) with the rows staged k-chunk by k-chunk and the accumulators carried across the chunks of a tile.
//
// What it keeps of that kernel: persistent workgroups of 8 waves over contiguous ranges of staging tiles; rows HBM -> LDS by
// LDS-DMA (lds_dma16: inline asm, the compiler counts no wait for it) with 16 bytes of padding a row; block j of 16 queries
// belongs to wave j % 8, two blocks a wave, 256 queries a launch; query fragments from L2; the compiler's MFMA builtins
// (v_mfma_f32_16x16x32_bf16, or v_mfma_f32_16x16x4_f32 on float i of a 16-byte chunk times float i of the query's); the
// epilogue - s >= thr, row < n, the mask bit, one atomicAdd per candidate into the query's shared list while pos < cap, NaN
// never passes, lane-private lists unused (the select is told nwriters = 0); BIAS: s = fmaf(w, bias[clamped row], <row, query>)
// before the test.
//
// What is new:
//   * a staging tile is 64 rows x ONE k-chunk of 1,024 bytes (16 k-steps; the last chunk of a bf16 row with d % 512 == 256 is
//     512 bytes: 8 k-steps, the upper 32 lanes of its DMA instructions masked off).  A chunk of a row is exactly one LDS-DMA
//     wave instruction, so no instruction's bytes cross an LDS row (pitch 1,040);
//   * the loop order is tile -> k-chunk -> query block: acc[2][4] (32 VGPRs) lives across the chunks of a tile, the epilogue
//     runs once per tile behind the last chunk.  A score is still ONE chain of MFMAs over the k-steps in ascending order,
//     across the chunk boundaries: its bits depend on the width and the storage type only, not on the batch, the grid, the
//     workgroup or the tile;
//   * two LDS buffers, used in turn by consecutive chunks (the turn carries on across tiles).  Per chunk: DMA into this
//     chunk's buffer, s_waitcnt vmcnt(0), barrier, MFMAs.  The ONE barrier orders both ways: behind it every wave's pieces
//     of this chunk have landed (each wave waited for its own before it arrived), and every wave has consumed its fragment
//     reads of the PREVIOUS chunk (they feed MFMAs issued before the barrier), whose buffer is the one the NEXT chunk's DMA
//     writes - so a wave that is through with a chunk starts the next chunk's DMA while the others still multiply.
//     WideArgs::serial = 1 selects the plain form (barrier, DMA, wait, barrier, MFMAs), the A/B partner (TS_MFMA_WIDE_SERIAL).
//   * barriers: every wave of a workgroup executes nchunks (x 2 if serial) barriers per tile of its range, whatever its query
//     blocks: the wave-uniform blk >= nblocks test skips MFMAs and the epilogue, never a barrier.  A workgroup without a
//     tile returns before the first one.
//
// Full pass only: tile_stride == 1 and run == 1 (the host guarantees it); the kernel covers rows [0, 32 * ntiles) rounded up
// to whole 64-row tiles, the allocation is padded to 256 rows, so whole staging tiles are in bounds.  It may be the first
// level of a search (a tiny index under algo = mfma): thresholds -inf, every real row a candidate.
#pragma once
#include "wide_plan.h"
#include "kernels_mfma16_ops.h"

namespace ts {

constexpr int kWideThreads = 512;    // 8 waves
constexpr int kWideWaves = kWideThreads / 64;
constexpr int kWideNBW = kWideQueries / 16 / kWideWaves;      // query blocks per wave (2)
constexpr int kWideRB = kWideTileRows / 16;                   // row blocks of 16 per tile (4)
constexpr int kWideSteps = kWideChunkBytes / 64;              // k-steps of a full chunk (16)
constexpr int kWideBufBytes = kWideTileRows * kWidePitch;

struct WideArgs {
    MfmaArgs m;                      // the full pass's arguments as every matrix kernel takes them (m.q: storage dtype, row stride ld)
    int ld;                          // elements per row = d
    int serial;                      // 1: two barriers per chunk (the plain form)
    const float* bias;               // BIAS: [n] floats, exactly - every read is clamped to row < n
    float w;
};

template <bool F32, bool BIAS>
__global__ void __launch_bounds__(kWideThreads) mfma_wide_kernel(WideArgs wa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char srows[];
    const MfmaArgs& a = wa.m;
    constexpr int RB = kWideRB;
    constexpr int kElem = F32 ? 4 : 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int row_bytes = wa.ld * kElem;
    const int nchunks = wide_chunks(row_bytes);
    const int nblocks = (a.nq + 15) / 16;

    mfma_level_begin(a);
    // this workgroup's staging tiles of the rows [0, 32 * ntiles)
    const int64_t tiles = (a.ntiles * kTileRows + kWideTileRows - 1) / kWideTileRows;
    const int64_t t0 = tiles * (int64_t)blockIdx.x / gridDim.x;
    const int64_t t1 = tiles * (int64_t)(blockIdx.x + 1) / gridDim.x;
    if (t0 >= t1) return;

    int qid[kWideNBW];
    float thr[kWideNBW];
#pragma unroll
    for (int b = 0; b < kWideNBW; ++b) {
        qid[b] = (wave + kWideWaves * b) * 16 + r16;
        thr[b] = mfma_level_thr(a, qid[b]);
    }

    const unsigned lds_base = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)srows;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int frag_off[RB];                                             // this lane's fragment of k-step 0 in row block rb of a buffer
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) frag_off[rb] = (16 * rb + r16) * kWidePitch + kq * 16;
    int buf = 0;                                                  // the buffer of the chunk at hand: workgroup-uniform

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t p0 = t * kWideTileRows;                     // first row of the tile
        f32x4 acc[kWideNBW][RB];
#pragma unroll
        for (int b = 0; b < kWideNBW; ++b)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) acc[b][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
        float bterm[BIAS ? RB : 1][4];
        if constexpr (BIAS) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    // bias holds exactly n floats: a padding row of the last tile reads the last real row's (n >= 1) and is
                    // dropped by row < n below
                    const int64_t row = p0 + 16 * rb + 4 * kq + g;
                    bterm[rb][g] = wa.bias[row < a.n ? row : a.n - 1];
                }
        }

        for (int c = 0; c < nchunks; ++c) {
            const int cbytes = wide_chunk_bytes(row_bytes, c);    // 1,024, or 512 for a ragged last chunk
            if (wa.serial) __syncthreads();                       // argument-uniform: every wave of every workgroup takes it or none
            // chunk c of the tile's rows -> LDS: wave w moves rows w, w + 8, ..., one instruction a row (p0 + r < n_pad: the
            // allocation is padded to kRowPad rows; 1,024 c + 16 lane + 16 <= row_bytes for the lanes that take part)
            {
                const unsigned char* src = (const unsigned char*)a.corpus + (p0 + wv) * row_bytes + c * kWideChunkBytes + lane * 16;
                const unsigned dst = lds_base + buf * kWideBufBytes + wv * kWidePitch;
                if (lane * 16 < cbytes) {
#pragma unroll
                    for (int i = 0; i < kWideTileRows / kWideWaves; ++i)
                        lds_dma16(src + (int64_t)i * kWideWaves * row_bytes, dst + i * kWideWaves * kWidePitch);
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
                    (const unsigned char*)a.q + ((int64_t)qid[b] * wa.ld + (F32 ? 4 : 8) * kq) * kElem + c * kWideChunkBytes;
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

        // lane holds rows p0 + 16 rb + 4 kq + {0..3} for query qid[b]
#pragma unroll
        for (int b = 0; b < kWideNBW; ++b) {
            const int blk = wave + kWideWaves * b;
            if (blk >= nblocks) continue;
            if constexpr (BIAS) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[b][rb][g] = fmaf(wa.w, bterm[rb][g], acc[b][rb][g]);
            }
            bool any = false;
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int g = 0; g < 4; ++g) any |= acc[b][rb][g] >= thr[b];
            if (__ballot(any)) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float s = acc[b][rb][g];
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
