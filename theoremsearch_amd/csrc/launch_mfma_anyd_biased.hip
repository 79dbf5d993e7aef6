// Launches of the biased general-width full pass (kernels_mfma_anyd.h, BIAS): one instantiation per (storage type, row blocks
// per tile).  It serves every width of bias_plan.h's bias_served(), the four hand-laid ones included.
#include "host.h"
#include "bias_plan.h"
#include "kernels_mfma.h"
#include "kernels_mfma_anyd.h"

int launch_pass_mfma_anyd_biased(const ts_index* ix, int grid, hipStream_t st, const MfmaArgs& m) {
    if (!bias_served(ix->dtype, ix->d, true) || ix->ld != ix->d)
        return fail(TS_ERR_INTERNAL, "no biased matrix kernel for d = %d (ld = %lld)", ix->d, (long long)ix->ld);
    if (m.tile_stride != 1 || m.run != 1) return fail(TS_ERR_INTERNAL, "the biased matrix kernel is a full pass only");
    if (!ix->active_bias) return fail(TS_ERR_INTERNAL, "the biased matrix kernel needs the call's bias on the device");
    AnydBiasArgs a;
    a.a.m = m;
    a.a.ld = (int)ix->ld;
    a.bias = ix->active_bias;
    a.w = ix->active_bias_w;
    const int row_bytes = anyd_row_bytes(ix->dtype, ix->d);
    const int lds = anyd_lds_bytes(row_bytes);
    const bool f32 = ix->dtype == TS_F32;
    if (anyd_row_blocks(row_bytes) == 4) {
        if (f32) return launch_lds<mfma_anyd_biased_kernel<true, 4>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
        return launch_lds<mfma_anyd_biased_kernel<false, 4>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
    }
    if (f32) return launch_lds<mfma_anyd_biased_kernel<true, 2>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
    return launch_lds<mfma_anyd_biased_kernel<false, 2>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
}
