// The threshold sample's score kernel (kernels_sample.h), the text of its body: included inside sample_scores_kernel and
// sample_scores_rowsets_kernel (kernels_rowsets.h), which define   F32, RB (template parameters) and a (SampleArgs).  Text and
// not a function template for the reason kernels_mfma_anyd_pass.inc gives: the existing kernel's instructions stay what they are.
    extern __shared__ __attribute__((aligned(16))) unsigned char srows[];
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        *a.fb_count = 0;
    }
    const int nchunks = (a.nq + 63) / 64;
    if ((int)blockIdx.y >= nchunks) {
        if (blockIdx.x == 0 && a.part) rebalance_tiles(a.part, a.wg_ticks, a.part_g, a.part_gain, (double*)srows);
        if constexpr (!F32) {
            if (a.scr_qimg)
                for (int r = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); r < kMfmaQ; r += (int)gridDim.x * 4) {
                    // (the screen's width is the row length: it serves ld = d = 768 and 1024)
                    if (a.ld == 1024) screen_quantize_query<1024>((const unsigned short*)a.q, a.scr_nrows, r, (int)(threadIdx.x & 63), a.scr_qimg, a.scr_qmeta, a.scr_count);
                    else screen_quantize_query<768>((const unsigned short*)a.q, a.scr_nrows, r, (int)(threadIdx.x & 63), a.scr_qimg, a.scr_qmeta, a.scr_count);
                }
        }
        return;
    }
    constexpr int kRows = 16 * RB;
    constexpr int kElem = F32 ? 4 : 2;
    constexpr int kStepElems = F32 ? 16 : 32;                     // elements per k-step (16 bytes per lane and quarter)
    constexpr int kSeg = 32;                                      // k-steps whose query fragments are in flight together
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * kRows;               // first sample position of this workgroup
    const int64_t npos = a.ntiles * kTileRows;
    const int row_bytes = a.ld * kElem;
    const int pitch = row_bytes + kSampleRowPad;
    const int steps = a.ld / kStepElems;
    // global row of sample position p (rows of positions past the sample are clamped; their scores are never used)
    auto row_of = [&](int64_t p) -> int64_t {
        const int64_t j = min(p >> 5, a.ntiles - 1);
        const int64_t gt = (a.run == 1) ? j * a.tile_stride : (j / a.run) * a.run * a.tile_stride + j % a.run;
        return gt * kTileRows + (p & 31);
    };
    // the query fragments of the first segment (bf16: all of them up to d = 1024, half of them at d = 2048) are requested BEFORE the rows: they come
    // from L2 and do not depend on anything, so their round trip runs beside the rows' trip to HBM instead of behind it
    const int qrow = (int)blockIdx.y * 64 + wave * 16 + r16;      // this lane's query (B operand) and output column
    const unsigned char* brow = (const unsigned char*)a.q + ((int64_t)qrow * a.ld + (F32 ? 4 : 8) * kq) * kElem;
    uint4 bv[kSeg];
#pragma unroll
    for (int s = 0; s < kSeg; ++s)
        if (s < steps) bv[s] = *(const uint4*)(brow + (int64_t)s * 64);
    // rows -> LDS by LDS-DMA (no registers, no compiler-made waits): wave w moves rows w, w + 4, ... in pieces of 64 lanes x
    // 16 bytes - whole 128-byte lines per request, every piece of every row in flight before the single wait below
    {
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const unsigned lds_base = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)srows;
        const int per_row = row_bytes / 16;
        for (int rr = 0; rr < kRows / 4; ++rr) {
            const int r = wv + 4 * rr;
            const unsigned char* src = (const unsigned char*)a.corpus + row_of(p0 + r) * row_bytes;
            for (int pc = 0; pc * 64 < per_row; ++pc) {
                const int c = pc * 64 + lane;
                if (c < per_row) lds_dma16(src + c * 16, lds_base + r * pitch + pc * 1024);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    const unsigned char* arow[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) arow[rb] = srows + (16 * rb + r16) * pitch + kq * 16;
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
    // k in segments of at most kSeg k-steps (bf16: one segment up to d = 1024, two up to 2048; fp32: one up to d = 512, two up
    // to 1024): a segment's query fragments are all requested before its first MFMA
    for (int s0 = 0; s0 < steps; s0 += kSeg) {
        if (s0 > 0) {
#pragma unroll
            for (int s = 0; s < kSeg; ++s)
                if (s0 + s < steps) bv[s] = *(const uint4*)(brow + (int64_t)(s0 + s) * 64);
        }
        // groups of 4 k-steps: the 4 RB fragment reads of a group are issued before its MFMAs, so the LDS latency is paid once
        // per group, not once per MFMA.  The step count is even (ld % 64 == 0) and a multiple of 4 at the hand-laid widths and
        // on fp32; a bf16 width with ld % 128 == 64 ends in a group of TWO: the steps past the row end are never multiplied
        // (their row fragment is the next row's bytes, their query fragment a register nobody wrote)
#pragma unroll
        for (int g4 = 0; g4 < kSeg; g4 += 4) {
            if (s0 + g4 < steps) {
                const bool full = F32 || s0 + g4 + 4 <= steps;
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
                            for (int i = 0; i < 4; ++i) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[i], acc[rb], 0, 0, 0);
                        } else {
                            if (s < 2 || full)
                                acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(reinterpret_cast<const bf16x8&>(av[s][rb]),
                                                                                  reinterpret_cast<const bf16x8&>(bv[g4 + s]), acc[rb], 0, 0, 0);
                        }
                    }
            }
        }
    }
    // lane holds sample positions p0 + 16 rb + 4 kq + {0..3} for query qrow
    float* out = a.scores + (int64_t)qrow * a.row_stride + p0 + 4 * kq;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
        *(float4*)(out + 16 * rb) = make_float4(ok[rb][0] ? acc[rb][0] : -INFINITY, ok[rb][1] ? acc[rb][1] : -INFINITY,
                                                ok[rb][2] ? acc[rb][2] : -INFINITY, ok[rb][3] ? acc[rb][3] : -INFINITY);
