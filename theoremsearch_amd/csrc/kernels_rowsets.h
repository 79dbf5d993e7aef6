// The kernels of ts_search_rowsets beside the full pass (mfma_anyd_rowsets_kernel, kernels_mfma_anyd.h): the threshold sample,
// its select and the final select of a batch whose queries sit behind different row sets.  Each is the existing kernel's own
// text (the .inc files) behind a prologue that takes what the call fixes once - the mask, the estimate's inputs, min_fill -
// from the block's table (rowsets_plan.h: RowsetsTable) for THIS lane's or THIS workgroup's query:
//   * sample_scores_rowsets_kernel: sample_scores_kernel's computation; a lane's output column is one query, so the liveness
//     of its (sample position, query) pairs is read from that query's mask.  A dead pair stores -inf, as a masked row does
//     there.  No riders: the launch has no extra grid row (no rebalance, no screen image);
//   * sample_select_rowsets_kernel: sample_select_fast_kernel's rule - the k-th best of the live scores, the Gaussian tail
//     from 256 live scores on, the tail fit from 1,024 on - with z_tail, tail_p and the first cut z_sel of its query (the
//     live scores of a query are those of its own set's sample rows, so count, mean and sd are the set's);
//   * level_select_rowsets_kernel: level_select_kernel's final level with min_fill = min(k, rows the query's set allows).
#pragma once
#include "kernels_level.h"
#include "kernels_sample.h"
#include "rowsets_plan.h"

namespace ts {

// grid = (row_stride / (16 RB), query chunks of 64): no extra row, so every workgroup scores
template <bool F32, int RB>
__global__ void __launch_bounds__(256) sample_scores_rowsets_kernel(SampleArgs a0, const RowsetsTable* table) {
    SampleArgs a = a0;
    // this lane's query, as the body numbers it (qrow); the table has kRowsetsBlock entries, whatever nq
    const int qs = table->set[((int)blockIdx.y * 64 + (int)(threadIdx.x >> 6) * 16 + (int)(threadIdx.x & 15)) & (kRowsetsBlock - 1)];
    a.row_mask = qs < 0 ? nullptr : table->mask[qs];
#include "kernels_sample_scores.inc"
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS) sample_select_rowsets_kernel(LevelArgs a0, const float* scores, int row_stride,
                                                                        const RowsetsTable* table) {
    LevelArgs a = a0;
    a.z_tail = table->z_tail[blockIdx.x];
    a.tail_p = table->tail_p[blockIdx.x];
    const float z_sel = table->z_sel[blockIdx.x];
#include "kernels_sample_select.inc"
}

template <int KR>
__global__ void __launch_bounds__(kLevelThreads) level_select_rowsets_kernel(LevelArgs a0, const RowsetsTable* table) {
    LevelArgs a = a0;
    a.min_fill = table->min_fill[blockIdx.x];
#include "kernels_level_select.inc"
}

}  // namespace ts
