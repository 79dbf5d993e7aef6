// The int8 screen of the d = 1024 bf16 full pass (TS_MFMA_SCREEN_WIDE; kernels_screen8.h): the kernels of width 1024 -
// mfma16_topk_kernel<512, NB, 8 / 14> over 1,024-byte int8 rows, the quantisers, both forms of the exact rescore.
#include "launch_screen8_impl.h"

int screen_prepare_wide(ts_index* ix, const void* qmat, int nq_launch, bool quantize_queries, hipStream_t st) {
    return screen_prepare_w<1024>(ix, qmat, nq_launch, quantize_queries, st);
}

int screen_full_pass_wide(ts_index* ix, int nb, int nq, int grid, int variant, bool ksplit, hipStream_t st, const MfmaArgs& a) {
    return screen_full_pass_w<1024>(ix, nb, nq, grid, variant, ksplit, st, a);
}

int screen_tile_pass_wide(ts_index* ix, int nb, int grid, int variant, hipStream_t st, const MfmaArgs& a) {
    return screen_tile_pass_w<1024>(ix, nb, grid, variant, st, a);
}
