// The int8 screen of the bf16 full pass (kernels_screen8.h): image upkeep, query quantisation, the screen launch
// (mfma16_topk_kernel over int8 rows, VARIANT 8) and the exact rescore.  This unit holds the kernels of width 768; the opt-in
// width 1024 (TS_MFMA_SCREEN_WIDE) has its own, launch_screen8_wide.hip, and so have the quantisers and the rescore of fp32
// indexes (TS_MFMA_SCREEN_F32), launch_screen8_f32.hip.
#include "launch_screen8_impl.h"

// Indexes whose rows the library owns (not a view of another handle's rows, not rows attached from the caller - those may
// change behind the library and leave the image stale), on the 16x16 kernel: bf16 at d = 768 - or at d = 1024 when
// TS_MFMA_SCREEN_WIDE is set (default 0: the image costs 1,024 bytes per row) - and fp32 at d = 768 or 1024 when
// TS_MFMA_SCREEN_F32 is set (default 0: the image adds a quarter to the rows; never the 32x32x2 kernel, TS_MFMA_F32=32) and the
// search is the usual two-level one: a screened fp32 search holds up to 256 queries per launch, and the fp32 matrix kernel that
// would run the sparse levels of the guaranteed chain (TS_MFMA_STAT=0) or a list-form sample (TS_MFMA_SAMPLE=0) holds 64 or 128 -
// as the paired bf16 pass (mfma_pairs), the larger block exists only where every launch of the search can hold it.
// TS_MFMA_SCREEN=0 switches all of them off.
bool screen_usable(const ts_index* ix) {
    bool served = false;
    if (ix->dtype == TS_BF16) served = ix->d == 768 || (ix->d == 1024 && ix->knobs.get(K_MFMA_SCREEN_WIDE, 0) != 0);
    else if (ix->dtype == TS_F32)
        served = (ix->d == 768 || ix->d == 1024) && ix->knobs.get(K_MFMA_SCREEN_F32, 0) != 0 && ix->knobs.get(K_MFMA_F32, 16) != 32 &&
                 two_level_search(ix);
    return served && ix->ld == ix->d && use_shape16(ix) && !ix->borrowed && !ix->attached && ix->knobs.get(K_MFMA_SCREEN, 1) != 0;
}

int screen_prepare(ts_index* ix, const void* qmat, int nq_launch, bool quantize_queries, hipStream_t st) {
    if (ix->dtype == TS_F32) return screen_prepare_f32(ix, qmat, nq_launch, st);     // always quantises its queries itself
    if (ix->d == 1024) return screen_prepare_wide(ix, qmat, nq_launch, quantize_queries, st);
    return screen_prepare_w<768>(ix, qmat, nq_launch, quantize_queries, st);
}

int screen_full_pass(ts_index* ix, int nb, int nq, int grid, int variant, bool ksplit, hipStream_t st, const MfmaArgs& a) {
    if (ix->dtype == TS_F32) return screen_full_pass_f32(ix, nb, nq, grid, variant, st, a);
    if (ix->d == 1024) return screen_full_pass_wide(ix, nb, nq, grid, variant, ksplit, st, a);
    return screen_full_pass_w<768>(ix, nb, nq, grid, variant, ksplit, st, a);
}

// the tile kernel over an image of either width, for the unit that has no instantiation of it (launch_screen8_f32.hip)
int screen_tile_pass(ts_index* ix, int nb, int grid, int variant, hipStream_t st, const MfmaArgs& a) {
    if (ix->d == 1024) return screen_tile_pass_wide(ix, nb, grid, variant, st, a);
    return screen_tile_pass_w<768>(ix, nb, grid, variant, st, a);
}
