// Launches of the k-chunked matrix kernels (kernels_mfma_wide.h, kernels_sample_wide.h): the full pass, plain and biased, and
// the threshold sample - one instantiation per storage type each.
#include "host.h"
#include "kernels_mfma.h"
#include "kernels_mfma_wide.h"
#include "kernels_sample_wide.h"

static_assert(wide_lds_bytes() == 133120 && wide_lds_bytes() <= kAnydLdsLimit, "the two chunk buffers of a staging tile must fit the CU's LDS");
static_assert(2 * wide_sample_lds_bytes() <= kAnydLdsLimit && wide_sample_lds_bytes() <= kWideSampleLdsLimit, "two workgroups of the sample share a CU");
static_assert(kWideChunkBytes == 64 * 16 && kWideChunkBytes % kWideGroupBytes == 0 && kWidePitch >= kWideChunkBytes,
              "a chunk of a row is one LDS-DMA wave instruction and lies inside its LDS row");
static_assert(kRowPad % kWideTileRows == 0 && kWideTileRows % kTileRows == 0, "whole staging tiles inside the padded allocation");
static_assert(kWideQueries == kQBlock && kWideQueries <= kMfmaQ, "one launch holds one block of the query feed");

static int wide_pass(const ts_index* ix, int grid, hipStream_t st, const MfmaArgs& m, bool biased) {
    if (!wide_index(ix)) return fail(TS_ERR_INTERNAL, "no k-chunked matrix kernel for d = %d (ld = %lld)", ix->d, (long long)ix->ld);
    if (m.tile_stride != 1 || m.run != 1) return fail(TS_ERR_INTERNAL, "the k-chunked matrix kernel is a full pass only");
    if (biased && !ix->active_bias) return fail(TS_ERR_INTERNAL, "the biased matrix kernel needs the call's bias on the device");
    WideArgs a;
    a.m = m;
    a.ld = (int)ix->ld;
    a.serial = ix->knobs.get(K_MFMA_WIDE_SERIAL, 0) != 0;
    a.bias = biased ? ix->active_bias : nullptr;
    a.w = biased ? ix->active_bias_w : 0.0f;
    constexpr int lds = wide_lds_bytes();
    const bool f32 = ix->dtype == TS_F32;
    if (biased) {
        if (f32) return launch_lds<mfma_wide_kernel<true, true>, lds>(ix->device, grid, kWideThreads, lds, st, a);
        return launch_lds<mfma_wide_kernel<false, true>, lds>(ix->device, grid, kWideThreads, lds, st, a);
    }
    if (f32) return launch_lds<mfma_wide_kernel<true, false>, lds>(ix->device, grid, kWideThreads, lds, st, a);
    return launch_lds<mfma_wide_kernel<false, false>, lds>(ix->device, grid, kWideThreads, lds, st, a);
}

int launch_pass_mfma_wide(const ts_index* ix, int grid, hipStream_t st, const MfmaArgs& m) { return wide_pass(ix, grid, st, m, false); }
int launch_pass_mfma_wide_biased(const ts_index* ix, int grid, hipStream_t st, const MfmaArgs& m) { return wide_pass(ix, grid, st, m, true); }

int launch_sample_wide(const ts_index* ix, dim3 grid, hipStream_t st, const SampleArgs& sa) {
    if (!wide_index(ix) || sa.ld != ix->d) return fail(TS_ERR_INTERNAL, "no k-chunked threshold sample for d = %d (ld = %lld)", ix->d, (long long)ix->ld);
    if (sa.part || sa.scr_qimg) return fail(TS_ERR_INTERNAL, "the k-chunked threshold sample carries no rebalance and no screen image");
    constexpr int lds = wide_sample_lds_bytes();
    if (ix->dtype == TS_F32) return launch_lds<sample_scores_wide_kernel<true>, lds>(ix->device, grid, kWideSampleThreads, lds, st, sa);
    return launch_lds<sample_scores_wide_kernel<false>, lds>(ix->device, grid, kWideSampleThreads, lds, st, sa);
}
