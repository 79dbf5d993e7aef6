// The int8 screen of the bf16 full pass (kernels_screen8.h): image upkeep, query quantisation, the screen launch
// (mfma16_topk_kernel over int8 rows, VARIANT 8) and the exact rescore.  This unit holds the kernels of width 768; the opt-in
// width 1024 (TS_MFMA_SCREEN_WIDE) has its own, launch_screen8_wide.hip.
#include "launch_screen8_impl.h"

// Indexes whose rows the library owns (not a view of another handle's rows, not rows attached from the caller - those may
// change behind the library and leave the image stale), bf16 on the 16x16 kernel, at d = 768 - or at d = 1024 when
// TS_MFMA_SCREEN_WIDE is set (default 0: the image costs 1,024 bytes per row); TS_MFMA_SCREEN=0 switches both off.
bool screen_usable(const ts_index* ix) {
    const bool width = ix->d == 768 || (ix->d == 1024 && ix->knobs.get(K_MFMA_SCREEN_WIDE, 0) != 0);
    return ix->dtype == TS_BF16 && width && ix->ld == ix->d && use_shape16(ix) && !ix->borrowed && !ix->attached &&
           ix->knobs.get(K_MFMA_SCREEN, 1) != 0;
}

int screen_prepare(ts_index* ix, const void* qmat, int nq_launch, bool quantize_queries, hipStream_t st) {
    if (ix->d == 1024) return screen_prepare_wide(ix, qmat, nq_launch, quantize_queries, st);
    return screen_prepare_w<768>(ix, qmat, nq_launch, quantize_queries, st);
}

int screen_full_pass(ts_index* ix, int nb, int nq, int grid, int variant, bool ksplit, hipStream_t st, const MfmaArgs& a) {
    if (ix->d == 1024) return screen_full_pass_wide(ix, nb, nq, grid, variant, ksplit, st, a);
    return screen_full_pass_w<768>(ix, nb, nq, grid, variant, ksplit, st, a);
}
