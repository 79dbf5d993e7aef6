// Corpus moments: a pass over the stored rows that yields X^T X (a SYRK whose summed index is the corpus ROW) and, with an
// indicator block as the left operand, the column sums per group of a metadata column.  moments_plan.h holds every size and
// the LDS image; this file the kernels.
//
// moments_kernel<F32, IND>, 256 threads = four waves, one workgroup per (unit, row range) = (blockIdx.x, blockIdx.y):
//   IND = false  unit = a pair of column panels (pi <= pj).  Wave w owns the 64 x 64 quadrant (w >> 1, w & 1) of the pair's
//                128 x 128 tile: 4 x 4 accumulator blocks of 16 x 16.  On a diagonal pair the quadrant (1, 0) is never read
//                (the finish mirrors the upper half) and its wave only stages.
//   IND = true   unit = (panel, chunk of 64 groups).  Wave w owns columns 32 w .. 32 w + 31 of the panel for all four blocks of
//                16 groups.  Left operand element (group g, row r) = 1 when codes[r] == g and the row counts, else 0;
//                codes == NULL: every counted row has code 0 (the column sums of ts_index_moments).
// Per tile of 64 rows: the workgroup's panels go HBM -> LDS by LDS-DMA, 8 rows x 128 bytes per wave instruction, each lane
// fetching the chunk that mom_lds_off puts in its slot; then
//   bf16  v_mfma_f32_16x16x32_bf16, two k-steps of 32 rows.  BOTH operands are transposed reads of the one image: a lane needs
//         8 rows of one column, so two ds_read_b64_tr_b16 make an operand - lane group g = lane >> 4 takes rows 4 g .. 4 g + 3
//         and 16 + 4 g .. 16 + 4 g + 3 of the step (any assignment of rows to k slots serves, as long as both operands share
//         it).  Every lane address is a multiple of 8 (chunks of 16 bytes, halves of 8); the reads sit in straight-line code of
//         all 256 threads, so EXEC is all ones.
//   fp32  v_mfma_f32_16x16x4_f32, sixteen k-steps of 4 rows; an operand is one float per lane (column lane & 15 of row
//         lane >> 4 of the step), a 32-bit LDS read.
// A row that does not count - disallowed by the row set, at or past n in the padded allocation, or (IND) with a code outside
// [0, ngroups) - is zeroed in BOTH operands, by a select on the fragments (0 x NaN is NaN), never by a branch around a read.
// After kMomFlushRows rows, and at the end of its range, the workgroup adds its fp32 accumulators in double into the partial tile
// it alone owns; moments_finish_* add the ranges' tiles in the order of the ranges.  No atomics on floating-point values
// anywhere: the result has the same bits on every call.
#pragma once
#include "kernels_mfma.h"
#include "kernels_mfma16_ops.h"
#include "moments_plan.h"

namespace ts {

struct MomArgs {
    const void* rows;          // [n_pad][d], storage type of the kernel
    const u32* mask;           // row set's bitmask (whole 256-row blocks, zero past n) or NULL
    const int32_t* codes;      // IND: [n] group codes or NULL (one group: every counted row)
    double* partial;           // [ranges][units][tile]
    int64_t n;
    int d;
    int ngroups;               // IND
};

typedef __attribute__((ext_vector_type(4))) __bf16 mom_bf16x4;
typedef __attribute__((address_space(3))) unsigned char* mom_lds_ptr;

__device__ __forceinline__ bf16x8 mom_read_tr(mom_lds_ptr p) {
    const mom_bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) mom_bf16x4*)p);
    const mom_bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) mom_bf16x4*)(p + kMomTrSecond));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// 16-bit lanes of a dword kept where bit 0 / bit 1 of b is set
__device__ __forceinline__ u32 mom_pair_mask(u32 b) { return ((b & 1u) ? 0x0000FFFFu : 0u) | ((b & 2u) ? 0xFFFF0000u : 0u); }
__device__ __forceinline__ bf16x8 mom_and(bf16x8 v, const u32 (&m)[4]) {
    uint4 u = reinterpret_cast<const uint4&>(v);
    u.x &= m[0]; u.y &= m[1]; u.z &= m[2]; u.w &= m[3];
    return reinterpret_cast<const bf16x8&>(u);
}

template <bool F32, bool IND>
__global__ __launch_bounds__(kMomThreads, 2) void moments_kernel(MomArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smom[];
    constexpr int kElem = F32 ? 4 : 2;
    constexpr int kSubs = kMomPanel * kElem / kMomSubBytes;       // sub-images of a panel: 2 / 4
    constexpr int kSubCols = kMomSubBytes / kElem;                // columns of a sub-image: 64 / 32
    constexpr int NA = 4, NB = IND ? 2 : 4;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, kq = lane >> 4;

    int pi = 0, pj = 0, chunk = 0;
    if constexpr (IND) {
        const int chunks = mom_group_chunks(a.ngroups);
        pi = pj = (int)blockIdx.x / chunks;
        chunk = (int)blockIdx.x % chunks;
    } else {
        mom_pair(mom_panels(a.d), (int)blockIdx.x, &pi, &pj);
    }
    const bool one_panel = IND || pi == pj;
    const int cnt_a = one_panel ? 0 : mom_panel_cols(a.d, pi) / kSubCols;     // sub-images staged for the left panel
    const int cnt_b = mom_panel_cols(a.d, pj) / kSubCols;
    const int base_b = one_panel ? 0 : kSubs;                                 // LDS sub-image of the right panel's first
    const int wr = wv >> 1, wc = wv & 1;
    const bool idle = !IND && pi == pj && wr > wc;                            // wave-uniform

    const unsigned lds_base = (unsigned)(unsigned long long)(mom_lds_ptr)smom;
    const mom_lds_ptr lds = (mom_lds_ptr)smom;
    const int64_t row_bytes = (int64_t)a.d * kElem;

    // the lane's fragment addresses at the tile's first k-step
    int off_a[NA], off_b[NB];
#pragma unroll
    for (int i = 0; i < NA; ++i) off_a[i] = mom_frag_off(F32, lane, 0, 4 * wr + i);
#pragma unroll
    for (int j = 0; j < NB; ++j) off_b[j] = mom_frag_off(F32, lane, base_b, IND ? 2 * wv + j : 4 * wc + j);

    f32x4 acc[NA][NB];
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    double* tile = a.partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (IND ? kMomGroupChunk * kMomPanel : kMomPanel * kMomPanel);
    bool first = true;
    auto flush = [&]() {
        if (idle) return;
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int row = IND ? 16 * i + 4 * kq + g : 64 * wr + 16 * i + 4 * kq + g;
                    const int col = IND ? 32 * wv + 16 * j + r16 : 64 * wc + 16 * j + r16;
                    double* t = tile + row * kMomPanel + col;
                    const double v = (double)acc[i][j][g];
                    *t = first ? v : *t + v;
                }
                acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        first = false;
    };

    int64_t r0, r1;
    mom_range_rows(a.n, (int)gridDim.y, (int)blockIdx.y, &r0, &r1);
    int since = 0;
    for (int64_t p0 = r0; p0 < r1; p0 += kMomTileRows) {
        __syncthreads();                                          // the previous tile's fragment reads are done
        // rows -> LDS: one wave instruction moves 8 rows x 128 bytes of one sub-image; rows p0 .. p0 + 63 < n_pad
        for (int u = wv; u < (cnt_a + cnt_b) * 8; u += kMomThreads / 64) {
            const int t = u >> 3, r8 = (u & 7) * 8;
            const bool left = t < cnt_a;
            const int panel = left ? pi : pj, sub = left ? t : t - cnt_a, lsub = left ? t : base_b + t - cnt_a;
            const int r = r8 + (lane >> 3);
            const int ch = mom_stage_chunk(F32, lane, r8);
            const unsigned char* src = (const unsigned char*)a.rows + (p0 + r) * row_bytes + panel * (kMomPanel * kElem) + sub * kMomSubBytes + ch * 16;
            lds_dma16(src, lds_base + (unsigned)((lsub * kMomTileRows + r8) * kMomSubBytes));
        }
        // the rows of this tile that count, one word per 32 rows
        u32 w[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int64_t row = p0 + 32 * k, rem = a.n - row;
            const u32 m = a.mask ? a.mask[row >> 5] : 0xFFFFFFFFu;
            w[k] = rem >= 32 ? m : rem <= 0 ? 0u : (m & ((1u << (int)rem) - 1u));
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        if (!idle) {
            if constexpr (F32) {
#pragma unroll 4
                for (int s = 0; s < kMomTileRows / 4; ++s) {
                    const int row = 4 * s + kq;
                    bool on = (w[s >> 3] >> (row & 31)) & 1u;
                    float fa[NA], fb[NB];
                    if constexpr (IND) {
                        const int64_t cr = p0 + row < a.n ? p0 + row : a.n - 1;
                        const int c = a.codes ? a.codes[cr] : 0;
                        on = on && c >= 0 && c < a.ngroups;          // a row that goes nowhere is zeroed in the right operand too
#pragma unroll
                        for (int i = 0; i < NA; ++i) fa[i] = (on && c == chunk * kMomGroupChunk + 16 * i + r16) ? 1.f : 0.f;
                    } else {
#pragma unroll
                        for (int i = 0; i < NA; ++i) {
                            const float v = *(const __attribute__((address_space(3))) float*)(lds + off_a[i] + s * mom_step_bytes(true));
                            fa[i] = on ? v : 0.f;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < NB; ++j) {
                        const float v = *(const __attribute__((address_space(3))) float*)(lds + off_b[j] + s * mom_step_bytes(true));
                        fb[j] = on ? v : 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < NA; ++i)
#pragma unroll
                        for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    // element e of the lane's fragment is row mom_frag_row(lane, e) of the step: bit e of `bits` says it counts
                    u32 bits = ((w[ks] >> (4 * kq)) & 15u) | (((w[ks] >> (16 + 4 * kq)) & 15u) << 4);
                    int code[IND ? 8 : 1];
                    if constexpr (IND) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int64_t row = p0 + 32 * ks + mom_frag_row(lane, e);
                            code[e] = a.codes ? a.codes[row < a.n ? row : a.n - 1] : 0;
                            if (code[e] < 0 || code[e] >= a.ngroups) bits &= ~(1u << e);     // a row that goes nowhere is zeroed in the right operand too
                        }
                    }
                    const u32 m[4] = {mom_pair_mask(bits), mom_pair_mask(bits >> 2), mom_pair_mask(bits >> 4), mom_pair_mask(bits >> 6)};
                    bf16x8 fa[NA], fb[NB];
                    if constexpr (IND) {
                        u32 hit[NA][4];
#pragma unroll
                        for (int i = 0; i < NA; ++i)
#pragma unroll
                            for (int x = 0; x < 4; ++x) hit[i][x] = 0u;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int c = code[e];
#pragma unroll
                            for (int i = 0; i < NA; ++i)
                                if (c == chunk * kMomGroupChunk + 16 * i + r16) hit[i][e >> 1] |= 0x3F80u << (16 * (e & 1));     // bf16 1.0
                        }
#pragma unroll
                        for (int i = 0; i < NA; ++i) {
                            const uint4 u = {hit[i][0] & m[0], hit[i][1] & m[1], hit[i][2] & m[2], hit[i][3] & m[3]};
                            fa[i] = reinterpret_cast<const bf16x8&>(u);
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < NA; ++i) fa[i] = mom_and(mom_read_tr(lds + off_a[i] + ks * mom_step_bytes(false)), m);
                    }
#pragma unroll
                    for (int j = 0; j < NB; ++j) fb[j] = mom_and(mom_read_tr(lds + off_b[j] + ks * mom_step_bytes(false)), m);
#pragma unroll
                    for (int i = 0; i < NA; ++i)
#pragma unroll
                        for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
                }
            }
        }
        since += kMomTileRows;
        if (since == kMomFlushRows) {
            flush();
            since = 0;
        }
    }
    if (since || first) flush();
}

// out [d][d]: the ranges' tiles of every pair added in the order of the ranges, the upper triangle mirrored into the lower
__global__ __launch_bounds__(256) void moments_finish_gram(const double* partial, double* out, int d, int ranges) {
    const int pair = blockIdx.y, units = gridDim.y;
    const int e = blockIdx.x * 256 + threadIdx.x, ii = e / kMomPanel, jj = e % kMomPanel;
    int pi, pj;
    mom_pair(mom_panels(d), pair, &pi, &pj);
    const int gi = pi * kMomPanel + ii, gj = pj * kMomPanel + jj;
    if (gi >= d || gj >= d || (pi == pj && ii > jj)) return;
    double s = 0.0;
    for (int r = 0; r < ranges; ++r) s += partial[((int64_t)r * units + pair) * (kMomPanel * kMomPanel) + e];
    out[(int64_t)gi * d + gj] = s;
    out[(int64_t)gj * d + gi] = s;
}

// out [ngroups][d]: unit = panel * chunks + chunk
__global__ __launch_bounds__(256) void moments_finish_groups(const double* partial, double* out, int d, int ngroups, int ranges) {
    const int unit = blockIdx.y, units = gridDim.y, chunks = mom_group_chunks(ngroups);
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int g = (unit % chunks) * kMomGroupChunk + e / kMomPanel, col = (unit / chunks) * kMomPanel + e % kMomPanel;
    if (g >= ngroups || col >= d) return;
    double s = 0.0;
    for (int r = 0; r < ranges; ++r) s += partial[((int64_t)r * units + unit) * (kMomGroupChunk * kMomPanel) + e];
    out[(int64_t)g * d + col] = s;
}

// counts [ngroups] (zeroed by the caller): the rows that count, per code; a thread takes one mask word, integers only
__global__ __launch_bounds__(256) void moments_count_kernel(const u32* mask, const int32_t* codes, int64_t n, int ngroups, u64* counts) {
    __shared__ u32 hist[kMomMaxGroups];
    for (int i = threadIdx.x; i < ngroups; i += 256) hist[i] = 0u;
    __syncthreads();
    const int64_t words = (n + 31) / 32;
    for (int64_t wi = (int64_t)blockIdx.x * 256 + threadIdx.x; wi < words; wi += (int64_t)gridDim.x * 256) {
        const int64_t rem = n - wi * 32;
        u32 w = mask ? mask[wi] : 0xFFFFFFFFu;
        if (rem < 32) w &= (1u << (int)rem) - 1u;
        if (!codes) {
            if (w) atomicAdd(&hist[0], (u32)__popc(w));
        } else {
            while (w) {
                const int b = __ffs(w) - 1;
                w &= w - 1;
                const int c = codes[wi * 32 + b];
                if (c >= 0 && c < ngroups) atomicAdd(&hist[c], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ngroups; i += 256)
        if (hist[i]) atomicAdd(&counts[i], (u64)hist[i]);
}

}  // namespace ts
