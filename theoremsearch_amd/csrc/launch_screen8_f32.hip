// The int8 screen of the fp32 full pass at d = 768 and 1024 (TS_MFMA_SCREEN_F32; kernels_screen8_f32.h): the quantisers that
// read fp32 rows and queries and the exact rescore on v_mfma_f32_16x16x4_f32.  The tile kernel is not instantiated here: an int8
// image is an int8 image, and the launch goes through the units that hold mfma16_topk_kernel<384 / 512, NB, 8 / 14>
// (screen_tile_pass: launch_screen8.hip, launch_screen8_wide.hip).
#include "launch_screen8_impl.h"
#include "kernels_screen8_f32.h"

// The queries are always quantised by a launch of their own: the fp32 threshold sample carries no rider row for them.
template <int W>
static int screen_prepare_f32_w(ts_index* ix, const void* qmat, int nq_launch, hipStream_t st) {
    return screen_prepare_with<W>(
        ix, true,
        [&](int64_t tile0, unsigned nblk) {
            quantize_tiles_f32_kernel<W><<<nblk, 256, 0, st>>>(ix->rows.as<const float>(), ix->scr_rows.as<signed char>(), ix->scr_tile.as<float4>(), tile0);
        },
        [&] {
            quantize_queries_f32_kernel<W><<<kMfmaQ, 64, 0, st>>>((const float*)qmat, std::min(nq_launch, kMfmaQ), ix->scr_q.as<signed char>(),
                                                               ix->scr_qmeta.as<float4>(), ix->scr_count);
        });
}

int screen_prepare_f32(ts_index* ix, const void* qmat, int nq_launch, hipStream_t st) {
    if (ix->d == 1024) return screen_prepare_f32_w<1024>(ix, qmat, nq_launch, st);
    return screen_prepare_f32_w<768>(ix, qmat, nq_launch, st);
}

// `a`: the fp32 pass's argument block (fp32 queries behind a.q, thresholds, row mask, tile table, the final select's lists)
int screen_full_pass_f32(ts_index* ix, int nb, int nq, int grid, int variant, hipStream_t st, const MfmaArgs& a) {
    TS_TRY(screen_tile_pass(ix, nb, grid, variant, st, a));
    ScreenRescoreF32Args r;
    r.rows = ix->rows.as<const float>();
    r.q = (const float*)a.q;
    r.thr = a.thr;
    r.scand = ix->scr_cand;
    r.scount = ix->scr_count;
    r.cand = a.cand;
    r.count = a.count;
    r.cap = a.cap;
    if (ix->d == 1024) screen_rescore_f32_kernel<1024><<<dim3((unsigned)nq, kRescoreY), 256, 0, st>>>(r);
    else screen_rescore_f32_kernel<768><<<dim3((unsigned)nq, kRescoreY), 256, 0, st>>>(r);
    HIP_TRY(hipGetLastError());
    return TS_OK;
}
