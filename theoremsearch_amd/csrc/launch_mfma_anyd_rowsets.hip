// Launches of the shared pass of ts_search_rowsets (a row set per query): the general-width full pass with the per-query mask
// (kernels_mfma_anyd.h, ROWSETS), one instantiation per (storage type, row blocks per tile), and the sample, sample select and
// final select beside it (kernels_rowsets.h).  It serves every width of bias_plan.h's bias_served(), the four hand-laid ones
// included.  `table`: the block's RowsetsTable on the device (ix->rowsets_dev).
#include "host.h"
#include "rowsets_plan.h"
#include "kernels_mfma.h"
#include "kernels_mfma_anyd.h"
#include "kernels_rowsets.h"

static int rowsets_table_check(const ts_index* ix) {
    if (!bias_served(ix->dtype, ix->d, true) || ix->ld != ix->d)
        return fail(TS_ERR_INTERNAL, "no row-set matrix kernel for d = %d (ld = %lld)", ix->d, (long long)ix->ld);
    if (!ix->rowsets_dev || ix->rowsets_dev.bytes() < sizeof(RowsetsTable))
        return fail(TS_ERR_INTERNAL, "the row-set matrix kernels need the block's table on the device");
    return TS_OK;
}

int launch_pass_mfma_anyd_rowsets(const ts_index* ix, int grid, hipStream_t st, const MfmaArgs& m) {
    TS_TRY(rowsets_table_check(ix));
    if (m.tile_stride != 1 || m.run != 1) return fail(TS_ERR_INTERNAL, "the row-set matrix kernel is a full pass only");
    AnydRowsetsArgs a;
    a.a.m = m;
    a.a.m.row_mask = nullptr;
    a.a.ld = (int)ix->ld;
    a.table = ix->rowsets_dev.as<const RowsetsTable>();
    const int row_bytes = anyd_row_bytes(ix->dtype, ix->d);
    const int lds = anyd_lds_bytes(row_bytes);
    const bool f32 = ix->dtype == TS_F32;
    if (anyd_row_blocks(row_bytes) == 4) {
        if (f32) return launch_lds<mfma_anyd_rowsets_kernel<true, 4>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
        return launch_lds<mfma_anyd_rowsets_kernel<false, 4>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
    }
    if (f32) return launch_lds<mfma_anyd_rowsets_kernel<true, 2>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
    return launch_lds<mfma_anyd_rowsets_kernel<false, 2>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
}

// grid: (sample rows / 32, query chunks of 64) - no rider row; lds: sample_lds_bytes(32, row bytes) <= lds_max
int launch_sample_rowsets(const ts_index* ix, dim3 grid, int lds, hipStream_t st, const SampleArgs& sa) {
    TS_TRY(rowsets_table_check(ix));
    constexpr int kSampleLdsMax = 144 * 1024;
    if (lds > kSampleLdsMax) return fail(TS_ERR_INTERNAL, "threshold sample: rows of %lld bytes do not fit the LDS", (long long)(ix->ld * ix->elem()));
    if (sa.part || sa.scr_qimg || (int)grid.y != (sa.nq + 63) / 64) return fail(TS_ERR_INTERNAL, "the row-set threshold sample carries no riders");
    const RowsetsTable* table = ix->rowsets_dev.as<const RowsetsTable>();
    if (ix->dtype == TS_F32) return launch_lds<sample_scores_rowsets_kernel<true, 2>, kSampleLdsMax>(ix->device, grid, 256, lds, st, sa, table);
    return launch_lds<sample_scores_rowsets_kernel<false, 2>, kSampleLdsMax>(ix->device, grid, 256, lds, st, sa, table);
}

int launch_sample_select_rowsets(const ts_index* ix, int nq, hipStream_t st, const LevelArgs& l, const float* scores, int row_stride) {
    TS_TRY(rowsets_table_check(ix));
    if (nq > kRowsetsBlock) return fail(TS_ERR_INTERNAL, "a block of the row-set pass holds %d queries", kRowsetsBlock);
    sample_select_rowsets_kernel<kSelThreads><<<nq, kSelThreads, 0, st>>>(l, scores, row_stride, ix->rowsets_dev.as<const RowsetsTable>());
    HIP_TRY(hipGetLastError());
    return TS_OK;
}

int launch_level_select_rowsets(const ts_index* ix, int nq, hipStream_t st, const LevelArgs& l) {
    TS_TRY(rowsets_table_check(ix));
    if (nq > kRowsetsBlock) return fail(TS_ERR_INTERNAL, "a block of the row-set pass holds %d queries", kRowsetsBlock);
    const RowsetsTable* table = ix->rowsets_dev.as<const RowsetsTable>();
    if (l.kk <= 64) return launch_lds<level_select_rowsets_kernel<1>>(ix->device, nq, kLevelThreads, kLevelLds, st, l, table);
    return launch_lds<level_select_rowsets_kernel<4>>(ix->device, nq, kLevelThreads, kLevelLds, st, l, table);
}
