// Launches of the general-width full pass (kernels_mfma_anyd.h): one instantiation per (storage type, row blocks per tile).
#include "host.h"
#include "kernels_mfma.h"
#include "kernels_mfma_anyd.h"

static_assert(kAnydLdsMax <= kAnydLdsLimit, "the staging tile must fit the CU's LDS");
static_assert(anyd_lds_bytes(kAnydMaxRowBytes) <= kAnydLdsMax && anyd_lds_bytes(2048) == kAnydLdsMax, "kAnydLdsMax is the largest launch");

int launch_pass_mfma_anyd(const ts_index* ix, int grid, hipStream_t st, const MfmaArgs& m) {
    if (!anyd_served(ix->dtype, ix->d, true) || ix->ld != ix->d)
        return fail(TS_ERR_INTERNAL, "no general-width matrix kernel for d = %d (ld = %lld)", ix->d, (long long)ix->ld);
    if (m.tile_stride != 1 || m.run != 1) return fail(TS_ERR_INTERNAL, "the general-width matrix kernel is a full pass only");
    AnydArgs a;
    a.m = m;
    a.ld = (int)ix->ld;
    const int row_bytes = anyd_row_bytes(ix->dtype, ix->d);
    const int lds = anyd_lds_bytes(row_bytes);
    const bool f32 = ix->dtype == TS_F32;
    if (anyd_row_blocks(row_bytes) == 4) {
        if (f32) return launch_lds<mfma_anyd_kernel<true, 4>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
        return launch_lds<mfma_anyd_kernel<false, 4>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
    }
    if (f32) return launch_lds<mfma_anyd_kernel<true, 2>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
    return launch_lds<mfma_anyd_kernel<false, 2>, kAnydLdsMax>(ix->device, grid, kAnydThreads, lds, st, a);
}
