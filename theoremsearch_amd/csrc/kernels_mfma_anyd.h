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
//   * mfma_anyd_biased_kernel (ts_search_biased_ex) is the same pass with s = fmaf(w, bias[row], <row, query>) in the epilogue; it
//     also runs the four hand-laid widths (bias_plan.h: bias_served), since the row length is a run-time value.
//   * mfma_anyd_rowsets_kernel (ts_search_rowsets) is the same pass with the filter of the epilogue taken per query, at the same widths.
//   * mfma_anyd_biased_rowsets_kernel (ts_search_biased_rowsets) has both: s = fmaf(w[query], bias[row], <row, query>) with a
//     weight per query, and the filter per query.
//
// Full pass only: tile_stride == 1 and run == 1 (the host guarantees it); the kernel covers rows [0, 32 * ntiles), the
// allocation is padded to 256 rows, so whole staging tiles are in bounds.  It may be the first level of a search (a tiny
// index under algo = mfma): thresholds -inf, every real row a candidate.
#pragma once
#include "anyd_plan.h"
#include "rowsets_plan.h"
#include "biased_rowsets_plan.h"
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

// The biased search (ts_search_biased_ex): the same pass with the per-row additive term in the epilogue.  A row's key score
// is fmaf(w, bias[row], <row, query>): that value is tested against thr, written into the key and returned.
struct AnydBiasArgs {
    AnydArgs a;
    const float* bias;               // [n] floats, exactly: every read is guarded by row < n
    float w;
};

// One body for both kernels (kernels_mfma_anyd_pass.inc, which says why it is text): the plain kernel compiles it with BIAS =
// false, to the instructions it had before the biased one existed.
template <bool F32, int RB>
__global__ void __launch_bounds__(kAnydThreads) mfma_anyd_kernel(AnydArgs aa) {
    constexpr bool BIAS = false;
    constexpr bool ROWSETS = false;
    const float* const bias = nullptr;
    const float bias_w = 0.0f;
    const RowsetsTable* const rowsets = nullptr;
    constexpr bool QWEIGHT = false;
    const float* const qweight = nullptr;
#include "kernels_mfma_anyd_pass.inc"
}

template <bool F32, int RB>
__global__ void __launch_bounds__(kAnydThreads) mfma_anyd_biased_kernel(AnydBiasArgs ba) {
    constexpr bool BIAS = true;
    constexpr bool ROWSETS = false;
    const AnydArgs& aa = ba.a;
    const float* const bias = ba.bias;
    const float bias_w = ba.w;
    const RowsetsTable* const rowsets = nullptr;
    constexpr bool QWEIGHT = false;
    const float* const qweight = nullptr;
#include "kernels_mfma_anyd_pass.inc"
}

// A row set per query (ts_search_rowsets): the plain pass with the mask of the epilogue's test taken per query from the
// block's table (rowsets_plan.h: RowsetsTable; m.row_mask is not read).  Thresholds are per query already.
struct AnydRowsetsArgs {
    AnydArgs a;
    const RowsetsTable* table;       // device
};
template <bool F32, int RB>
__global__ void __launch_bounds__(kAnydThreads) mfma_anyd_rowsets_kernel(AnydRowsetsArgs ra) {
    constexpr bool BIAS = false;
    constexpr bool ROWSETS = true;
    const AnydArgs& aa = ra.a;
    const float* const bias = nullptr;
    const float bias_w = 0.0f;
    const RowsetsTable* const rowsets = ra.table;
    constexpr bool QWEIGHT = false;
    const float* const qweight = nullptr;
#include "kernels_mfma_anyd_pass.inc"
}

// A weight and a row set per query (ts_search_biased_rowsets): both epilogues at once, the weight of the bias term taken per
// query from the block's table (biased_rowsets_plan.h: BiasedRowsetsTable, whose first member is the row-set table).
struct AnydBiasedRowsetsArgs {
    AnydArgs a;
    const float* bias;               // [n] floats, exactly
    const BiasedRowsetsTable* table; // device
};
template <bool F32, int RB>
__global__ void __launch_bounds__(kAnydThreads) mfma_anyd_biased_rowsets_kernel(AnydBiasedRowsetsArgs ba) {
    constexpr bool BIAS = true;
    constexpr bool ROWSETS = true;
    constexpr bool QWEIGHT = true;
    const AnydArgs& aa = ba.a;
    const float* const bias = ba.bias;
    const float bias_w = 0.0f;
    const RowsetsTable* const rowsets = &ba.table->r;
    const float* const qweight = ba.table->weight;
#include "kernels_mfma_anyd_pass.inc"
}

}  // namespace ts
