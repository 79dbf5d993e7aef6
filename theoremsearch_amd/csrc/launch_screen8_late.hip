// The late-test form of the int8 screen (TS_MFMA_SCREEN_LATE; kVariantScreenLate, kernels_mfma16.h): the unmasked screen of the
// d = 768 bf16 full pass with four query blocks per wave (193 .. 256 queries per launch) - mfma16_topk_kernel<384, 4, 15>.  A unit
// of its own: the kernels of launch_screen8.hip come out of hipcc as they did before this form existed.
#include "host.h"
#include "kernels_screen8.h"

// `a`: the screen's argument block (screen_tile_pass_w, launch_screen8_impl.h: image, int8 queries, the screen's lists); no row mask
int launch_screen8_late(int dev, int grid, hipStream_t st, const MfmaArgs& a) {
    constexpr int lds = Mfma16Dims<384>::kLds + kMfma16StageBytes;
    static_assert(lds <= 160 * 1024, "DMA ring + staged candidates must fit the CU's LDS");
    if (a.row_mask != nullptr) return fail(TS_ERR_INTERNAL, "the late-test screen holds no code that reads a row mask");
    return launch_lds<mfma16_topk_kernel<384, 4, kVariantScreenLate, false>>(dev, grid, kMfmaThreads, lds, st, a);
}
