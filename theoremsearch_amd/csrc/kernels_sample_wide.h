// The threshold sample of the batched search at the k-chunked widths (wide_plan.h): sample_scores_kernel's contract
// (kernels_sample.h: SampleArgs in, a dense [query][sample position] fp32 matrix out, -inf at masked / out-of-range positions,
// *fb_count = 0) and its workgroup shape - 32 sample rows x one 64-query chunk, 256 threads, wave w holds queries 16 w ..
// 16 w + 15 of the chunk - with the rows staged k-chunk by k-chunk (1,024 bytes of each row, a ragged 512-byte last chunk on
// bf16 d % 512 == 256) and the accumulators carried across the chunks.  Two LDS buffers used in turn, one barrier per chunk,
// as mfma_wide_kernel does it (kernels_mfma_wide.h says why one barrier orders both ways); a chunk's query fragments are
// requested before its rows.
// The riders of the narrower sample's launch (last search's rebalance, the int8 screen's query image) do not exist at these
// widths: grid.y is the number of query chunks, and the host refuses a launch that asks for either.
// The sums are the full pass's chain (ascending k-steps), but nothing downstream depends on bit-equal sample scores: the
// thresholds are estimates that the full pass verifies.
#pragma once
#include "wide_plan.h"
#include "kernels_sample.h"

namespace ts {

constexpr int kWideSampleThreads = 256;
constexpr int kWideSampleBufBytes = kWideSampleRows * kWidePitch;

template <bool F32>
__global__ void __launch_bounds__(kWideSampleThreads) sample_scores_wide_kernel(SampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char srows[];
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *a.fb_count = 0;
    constexpr int RB = kWideSampleRows / 16;
    constexpr int kElem = F32 ? 4 : 2;
    constexpr int kSteps = kWideChunkBytes / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * kWideSampleRows;     // first sample position of this workgroup
    const int64_t npos = a.ntiles * kTileRows;
    const int row_bytes = a.ld * kElem;
    const int nchunks = wide_chunks(row_bytes);
    // global row of sample position p (rows of positions past the sample are clamped; their scores are never used)
    auto row_of = [&](int64_t p) -> int64_t {
        const int64_t j = min(p >> 5, a.ntiles - 1);
        const int64_t gt = (a.run == 1) ? j * a.tile_stride : (j / a.run) * a.run * a.tile_stride + j % a.run;
        return gt * kTileRows + (p & 31);
    };
    const int qrow = (int)blockIdx.y * 64 + wave * 16 + r16;      // this lane's query (B operand) and output column
    const unsigned char* brow = (const unsigned char*)a.q + ((int64_t)qrow * a.ld + (F32 ? 4 : 8) * kq) * kElem;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned lds_base = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)srows;
    // wave w moves rows w, w + 4, ...: their first bytes (every row below n_pad: the tile index is clamped to the sample's)
    const unsigned char* src[kWideSampleRows / 4];
#pragma unroll
    for (int i = 0; i < kWideSampleRows / 4; ++i)
        src[i] = (const unsigned char*)a.corpus + row_of(p0 + wv + 4 * i) * row_bytes + lane * 16;
    int frag_off[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) frag_off[rb] = (16 * rb + r16) * kWidePitch + kq * 16;
    // validity of this lane's output positions
    bool ok[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t p = p0 + 16 * rb + 4 * kq + g;
            const int64_t row = row_of(p);
            ok[rb][g] = p < npos && row < a.n && (!a.row_mask || ((a.row_mask[row >> 5] >> (row & 31)) & 1u));
        }
    f32x4 acc[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};

    int buf = 0;
    for (int c = 0; c < nchunks; ++c) {
        const int cbytes = wide_chunk_bytes(row_bytes, c);        // 1,024, or 512 for a ragged last chunk
        const int steps = cbytes / 64;                            // 16 or 8: whole groups of four
        uint4 bv[kSteps];
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
            if (s < steps) bv[s] = *(const uint4*)(brow + c * kWideChunkBytes + s * 64);
        if (lane * 16 < cbytes) {
#pragma unroll
            for (int i = 0; i < kWideSampleRows / 4; ++i)
                lds_dma16(src[i] + c * kWideChunkBytes, lds_base + buf * kWideSampleBufBytes + (wv + 4 * i) * kWidePitch);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const unsigned char* tile = srows + buf * kWideSampleBufBytes;
#pragma unroll
        for (int g4 = 0; g4 < kSteps; g4 += 4) {
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
                            for (int i = 0; i < 4; ++i) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[i], acc[rb], 0, 0, 0);
                        } else {
                            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(reinterpret_cast<const bf16x8&>(av[s][rb]),
                                                                              reinterpret_cast<const bf16x8&>(bv[g4 + s]), acc[rb], 0, 0, 0);
                        }
                    }
            }
        }
        buf ^= 1;
    }
    // lane holds sample positions p0 + 16 rb + 4 kq + {0..3} for query qrow
    float* out = a.scores + (int64_t)qrow * a.row_stride + p0 + 4 * kq;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
        *(float4*)(out + 16 * rb) = make_float4(ok[rb][0] ? acc[rb][0] : -INFINITY, ok[rb][1] ? acc[rb][1] : -INFINITY,
                                                ok[rb][2] ? acc[rb][2] : -INFINITY, ok[rb][3] ? acc[rb][3] : -INFINITY);
}

}  // namespace ts
