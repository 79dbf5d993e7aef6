// Launches of the 32x32x16 bf16 matrix kernel (kernels_mfma.h) and of the 32x32x2 fp32 one (kernels_mfma_f32.h).
#include "host.h"
#include "kernels_mfma.h"
#include "kernels_mfma_f32.h"

template <int D, int GROUPS>
static int launch_mfma(int dev, bool full_pass, int variant, int grid, hipStream_t st, const MfmaArgs& a) {
    constexpr int lds = MfmaDims<D>::kLds;
    if (!full_pass) return launch_lds<mfma_topk_kernel<D, GROUPS, 0, true>>(dev, grid, kMfmaThreads, lds, st, a);
    auto go = [&](auto v) { return launch_lds<mfma_topk_kernel<D, GROUPS, decltype(v)::value, false>>(dev, grid, kMfmaThreads, lds, st, a); };
#ifdef TS_DIAG
    int rc;
    if (launch_variant<1, 2, 3, 4, 5, 6, 7>(variant, &rc, go)) return rc;
#endif
    return go(variant_c<0>{});
}

static int launch_mfma_f32(int dev, bool full_pass, int variant, int grid, hipStream_t st, const MfmaArgs& a) {
    constexpr int lds = MfmaF32Dims::kLds;
    if (!full_pass) return launch_lds<mfma_f32_topk_kernel<0, true>>(dev, grid, kMfmaThreads, lds, st, a);
#ifdef TS_DIAG
    if (variant == 1) return launch_lds<mfma_f32_topk_kernel<1, false>>(dev, grid, kMfmaThreads, lds, st, a);
#endif
    return launch_lds<mfma_f32_topk_kernel<0, false>>(dev, grid, kMfmaThreads, lds, st, a);
}


// groups = 128-query groups per launch (d = 1024: one)
int launch_pass_mfma32(int dev, int d, int groups, bool full_pass, int variant, int grid, hipStream_t st, const MfmaArgs& a) {
    if (d == 1024) return launch_mfma<1024, 1>(dev, full_pass, variant, grid, st, a);
    if (d == 512) return groups == 1 ? launch_mfma<512, 1>(dev, full_pass, variant, grid, st, a) : launch_mfma<512, 2>(dev, full_pass, variant, grid, st, a);
    if (d == 384) return groups == 1 ? launch_mfma<384, 1>(dev, full_pass, variant, grid, st, a) : launch_mfma<384, 2>(dev, full_pass, variant, grid, st, a);
    if (d == 768) return groups == 1 ? launch_mfma<768, 1>(dev, full_pass, variant, grid, st, a) : launch_mfma<768, 2>(dev, full_pass, variant, grid, st, a);
    return fail(TS_ERR_INTERNAL, "no 32x32x16 kernel for d = %d", d);
}

int launch_pass_mfma32_f32(int dev, bool full_pass, int variant, int grid, hipStream_t st, const MfmaArgs& a) {
    return launch_mfma_f32(dev, full_pass, variant, grid, st, a);
}
