// The general-width full pass (kernels_mfma_anyd.h), the text of the kernels' bodies: included inside mfma_anyd_kernel,
// mfma_anyd_biased_kernel, mfma_anyd_rowsets_kernel and mfma_anyd_biased_rowsets_kernel, which define   F32, RB (template
// parameters), BIAS, ROWSETS, QWEIGHT (constexpr bool), aa (AnydArgs), bias (const float*, read only where BIAS), bias_w (float),
// rowsets (const RowsetsTable*, read only where ROWSETS), qweight (const float*, read only where QWEIGHT); it declares the dynamic LDS array srows itself and uses the names of
// kernels_mfma_anyd.h (kAnydThreads, kAnydWaves, kAnydNBW, kAnydSeg, kAnydRowPad) and kernels_mfma.h.  Text and not a function
// template: inside a __device__ __forceinline__ function the compiler simplifies the body on its own before it inlines it, and
// the plain kernel comes out with other block placement and register numbers (make devasm + tools/devasm_diff.py show it);
// that kernel's instructions are to stay what they are.
// BIAS: per staging tile a lane loads the bias of its rows p0 + 16 rb + 4 kq + {0..3} once, before the tile's rows have
// landed (the loads' latency lies under the DMA wait), for both of the wave's query blocks.
// ROWSETS: a row set per query (ts_search_rowsets).  A lane keeps the set NUMBER of its query of each block (one register per
// block; the pointer would be two, and this kernel's budget is the plain kernel's: 8 waves per workgroup) and takes the mask
// pointer from the table only behind s >= thr, where a.row_mask is tested otherwise.
// QWEIGHT (with BIAS; ts_search_biased_rowsets): the weight of the bias term is the lane's query's own, qweight[query], one
// register per block beside qset[b], in place of the launch constant bias_w.
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
    int qset[ROWSETS ? kAnydNBW : 1];
    if constexpr (ROWSETS) {
#pragma unroll
        for (int b = 0; b < kAnydNBW; ++b) qset[b] = rowsets->set[qid[b]];     // qid < 256: inside the table
    }
    float qw[QWEIGHT ? kAnydNBW : 1];
    if constexpr (QWEIGHT) {
#pragma unroll
        for (int b = 0; b < kAnydNBW; ++b) qw[b] = qweight[qid[b]];            // [256], as the table's other columns
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
        float bterm[BIAS ? RB : 1][4];
        if constexpr (BIAS) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    // bias holds exactly n floats: a padding row of the last tile reads the last real row's (n >= 1), and is
                    // dropped by row < n below - a clamped address, not a predicated load (16 lane masks held over the MFMAs)
                    const int64_t row = p0 + 16 * rb + 4 * kq + g;
                    bterm[rb][g] = bias[row < a.n ? row : a.n - 1];
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
            if constexpr (BIAS) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        if constexpr (QWEIGHT) acc[rb][g] = fmaf(qw[b], bterm[rb][g], acc[rb][g]);
                        else acc[rb][g] = fmaf(bias_w, bterm[rb][g], acc[rb][g]);
                    }
            }
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
                        if constexpr (ROWSETS) {
                            if (s >= thr[b] && row < a.n) {
                                const u32* const qmask = qset[b] < 0 ? nullptr : rowsets->mask[qset[b]];
                                if (!qmask || ((qmask[row >> 5] >> (row & 31)) & 1u)) {
                                    const u32 pos = atomicAdd(&a.count[qid[b]], 1u);
                                    if (pos < (u32)a.cap) a.cand[(int64_t)qid[b] * a.cap + pos] = make_key(s, (u32)row);
                                }
                            }
                        } else
                        if (s >= thr[b] && row < a.n && (!a.row_mask || ((a.row_mask[row >> 5] >> (row & 31)) & 1u))) {
                            const u32 pos = atomicAdd(&a.count[qid[b]], 1u);
                            if (pos < (u32)a.cap) a.cand[(int64_t)qid[b] * a.cap + pos] = make_key(s, (u32)row);
                        }
                    }
            }
        }
    }
