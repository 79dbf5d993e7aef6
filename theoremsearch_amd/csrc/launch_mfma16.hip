// Launches of the 16x16x32 bf16 matrix kernel (kernels_mfma16.h): one instantiation per (width, query blocks per wave).
#include "host.h"
#include "kernels_mfma16.h"

template <int D, int NB>
static int launch_mfma16(int dev, bool full_pass, int variant, int grid, hipStream_t st, const MfmaArgs& a) {
    constexpr int lds = Mfma16Dims<D>::kLds + kMfma16StageBytes;
    static_assert(lds <= 160 * 1024, "DMA ring + staged candidates must fit the CU's LDS");
    // d = 384 / 512: the full pass only (the threshold sample has its own kernel; the thresholded sparse levels of the
    // guaranteed chain run the 32x32 kernel for these widths: use_shape16)
    constexpr bool kSparseToo = (D == 768 || D == 1024);
#ifdef TS_DIAG
    constexpr bool kDiag = (D == 768 && NB == 4);     // the timing-only variants exist for the headline shape only
#else
    constexpr bool kDiag = false;                     // ... and in the diagnostic build only (make diag)
#endif
    if (!full_pass) {
        if constexpr (kSparseToo) return launch_lds<mfma16_topk_kernel<D, NB, kVariantProduct, true>>(dev, grid, kMfmaThreads, lds, st, a);
        else return fail(TS_ERR_INTERNAL, "no sparse level of the 16x16 kernel at d = %d", D);
    }
    auto go = [&](auto v) { return launch_lds<mfma16_topk_kernel<D, NB, decltype(v)::value, false>>(dev, grid, kMfmaThreads, lds, st, a); };
    int rc;
    if constexpr (kDiag)
        if (launch_variant<kVariantNoEpilogue, kVariantDmaOnly, kVariantClockProbe, kVariantTestOnly, kVariantNoDma, kVariantStamps, kVariantSleep>(variant, &rc, go)) return rc;
    return go(variant_c<kVariantProduct>{});
}


// The paired full pass of d = 1024 (MfmaArgs::pair): 128 queries per workgroup, two workgroups per tile range.
static int launch_mfma16_pair(int dev, int variant, int grid, hipStream_t st, const MfmaArgs& a) {
    constexpr int lds = Mfma16Dims<1024>::kLds + kMfma16StageBytes + kMfma16PaceBytes;
    static_assert(lds <= 160 * 1024, "DMA ring + staged candidates + the pair's word must fit the CU's LDS");
    // the k-split form: 2 x 2 waves (query column x k half), eight ring slots, one 16 KB exchange buffer for the partial sums
    constexpr int lds_k = MfmaDims<1024, MfmaGeomKsplit<1024>>::kLds + kMfma16StageBytes + kMfma16PaceBytes + 16384;
    static_assert(lds_k <= 160 * 1024, "ring + staged candidates + the pair's word + the exchange buffers must fit the CU's LDS");
    if (grid % 16 != 0) return fail(TS_ERR_INTERNAL, "the paired pass needs a grid of whole groups of 16 workgroups, not %d", grid);
    auto go = [&](auto v) {
        constexpr int V = decltype(v)::value;
        if (a.pair == 2) return launch_lds<mfma16_topk_kernel<1024, 4, V, false, false, true, true>>(dev, grid, kMfmaThreads, lds_k, st, a);
        return launch_lds<mfma16_topk_kernel<1024, 2, V, false, false, true>>(dev, grid, kMfmaThreads, lds, st, a);
    };
#ifdef TS_DIAG
    int rc;
    if (launch_variant<kVariantNoEpilogue, kVariantDmaOnly, kVariantNoDma>(variant, &rc, go)) return rc;
#endif
    return go(variant_c<kVariantProduct>{});
}

// d = 384 / 512 / 768 / 1024, nb = query blocks of 16 per wave (64 * nb queries per launch; d = 1024: at most 3)
int launch_pass_mfma16(int dev, int d, int nb, bool full_pass, int variant, int grid, hipStream_t st, const MfmaArgs& a) {
    if (a.pair) {
        if (d != 1024 || nb != 2 || !full_pass) return fail(TS_ERR_INTERNAL, "paired pass asked for d = %d, %d blocks per wave", d, nb);   // (a.pair == 2: the k-split form, same queries per workgroup)
        return launch_mfma16_pair(dev, variant, grid, st, a);
    }
#define TS_NB_SWITCH(D_)                                                               \
    switch (nb) {                                                                      \
        case 1: return launch_mfma16<D_, 1>(dev, full_pass, variant, grid, st, a);     \
        case 2: return launch_mfma16<D_, 2>(dev, full_pass, variant, grid, st, a);     \
        case 3: return launch_mfma16<D_, 3>(dev, full_pass, variant, grid, st, a);     \
        case 4: if constexpr (D_ != 1024) return launch_mfma16<D_, 4>(dev, full_pass, variant, grid, st, a); break; \
        default: break;                                                                \
    }                                                                                  \
    break
    switch (d) {
        case 384: TS_NB_SWITCH(384);
        case 512: TS_NB_SWITCH(512);
        case 768: TS_NB_SWITCH(768);
        case 1024: TS_NB_SWITCH(1024);
        default: break;
    }
#undef TS_NB_SWITCH
    return fail(TS_ERR_INTERNAL, "no 16x16x32 kernel for d = %d with %d query blocks per wave", d, nb);
}
