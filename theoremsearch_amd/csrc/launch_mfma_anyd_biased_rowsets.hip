// Launches of the shared pass of ts_search_biased_rowsets (a weight and a row set per query): the general-width full pass with the
// per-query mask and the per-query weight (kernels_mfma_anyd.h, BIAS + ROWSETS), one instantiation per (storage type, row blocks
// per tile).  The histogram stage, the sample select and the unbias step beside it (kernels_biased_rowsets.h) are launched by
// search_mfma.hip; the threshold sample and the final select are launch_mfma_anyd_rowsets.hip's: ix->rowsets_dev holds the block's
// BiasedRowsetsTable, whose first member is the table they read.  It serves every width of bias_plan.h's bias_served().
#include "host.h"
#include "biased_rowsets_plan.h"
#include "kernels_mfma.h"
#include "kernels_mfma_anyd.h"

static int biased_rowsets_check(const ts_index* ix) {
    if (!bias_served(ix->dtype, ix->d, true) || ix->ld != ix->d)
        return fail(TS_ERR_INTERNAL, "no biased row-set matrix kernel for d = %d (ld = %lld)", ix->d, (long long)ix->ld);
    if (!ix->rowsets_dev || ix->rowsets_dev.bytes() < sizeof(BiasedRowsetsTable))
        return fail(TS_ERR_INTERNAL, "the biased row-set matrix kernels need the block's table on the device");
    if (!ix->active_bias) return fail(TS_ERR_INTERNAL, "the biased row-set matrix kernels need the call's bias on the device");
    return TS_OK;
}

int launch_pass_mfma_anyd_biased_rowsets(const ts_index* ix, int grid, hipStream_t st, const MfmaArgs& m) {
    TS_TRY(biased_rowsets_check(ix));
    if (m.tile_stride != 1 || m.run != 1) return fail(TS_ERR_INTERNAL, "the biased row-set matrix kernel is a full pass only");
    AnydBiasedRowsetsArgs a;
    a.a.m = m;
    a.a.m.row_mask = nullptr;
    a.a.ld = (int)ix->ld;
    a.bias = ix->active_bias;
    a.table = ix->rowsets_dev.as<const BiasedRowsetsTable>();
    const int row_bytes = anyd_row_bytes(ix->dtype, ix->d);
    const int lds = anyd_lds_bytes(row_bytes);
    const bool f32 = ix->dtype == TS_F32;
    if (anyd_row_blocks(row_bytes) == 4) {
        if (f32) return launch_lds<mfma_anyd_biased_rowsets_kernel<true, 4>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
        return launch_lds<mfma_anyd_biased_rowsets_kernel<false, 4>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
    }
    if (f32) return launch_lds<mfma_anyd_biased_rowsets_kernel<true, 2>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
    return launch_lds<mfma_anyd_biased_rowsets_kernel<false, 2>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
}
