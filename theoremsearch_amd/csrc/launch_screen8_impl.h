// The int8 screen's host side for one width W (768 or 1024; kernels_screen8.h), shared by the translation units that hold the
// kernel instantiations of a width: launch_screen8.hip (768) and launch_screen8_wide.hip (1024) - and by launch_screen8_f32.hip
// (fp32 indexes, either width), which brings quantisers and a rescore of its own and launches the tile kernel through those two.
#pragma once
#include "host.h"
#include "kernels_screen8.h"

template <int W, int NB>
static int launch_screen8(int dev, int grid, int variant, hipStream_t st, const MfmaArgs& a) {
    constexpr int D = W / 2;            // the int8 row as a bf16 row of half as many elements
    constexpr int lds = Mfma16Dims<D>::kLds + kMfma16StageBytes;
#ifdef TS_DIAG
    constexpr bool kDiag = NB == 4;     // the timing-only forms (variant_screen_diag) exist for the headline batch only
#else
    constexpr bool kDiag = false;       // ... and in the diagnostic build only (make diag)
#endif
    static_assert(lds <= 160 * 1024, "DMA ring + staged candidates must fit the CU's LDS");
    // a search with a row mask runs the form of the kernel that tests it (kVariantScreenMasked); the unmasked product (kVariantScreen) has no such code
    const bool masked = a.row_mask != nullptr;
    auto go = [&](auto v) { return launch_lds<mfma16_topk_kernel<D, NB, decltype(v)::value, false>>(dev, grid, kMfmaThreads, lds, st, a); };
    int rc;
    if constexpr (kDiag)
        if (launch_variant<kVariantScreenNoEpilogue, kVariantScreenStamps, kVariantScreenClockProbe, kVariantScreenDmaOnly, kVariantScreenTestOnly>(variant, &rc, go)) return rc;
    return masked ? go(variant_c<kVariantScreenMasked>{}) : go(variant_c<kVariantScreen>{});
}

// Before the search's first launch: the image covers every row written so far (allocated with the rows' capacity, made anew
// when an append has grown it), the launch's queries are quantised and the screen's lists emptied - here (quantize_queries),
// or by the caller's threshold sample, whose launch has room for it (SampleArgs::scr_qimg).
// quantize_tiles(tile0, nblk): the launch that quantises tiles tile0 .. tile0 + nblk - 1 from the index's rows;
// quantize_query_rows(): the launch that quantises the queries - both in the storage type of the index.
template <int W, class QuantizeTiles, class QuantizeQueries>
static int screen_prepare_with(ts_index* ix, bool quantize_queries, QuantizeTiles&& quantize_tiles, QuantizeQueries&& quantize_query_rows) {
    const int64_t tiles = ix->n_pad / kTileRows;
    if (ix->scr_pad != ix->n_pad) {
        ix->scr_pad = 0;
        DEV_TRY(remake(ix->scr_rows, (size_t)ix->n_pad * W, ix->scr_tile, (size_t)tiles * 16));
        ix->scr_pad = ix->n_pad;
        ix->scr_lo = 0;
        ix->scr_hi = ix->n_pad;
    }
    if (ix->scr_lo < ix->scr_hi) {
        // whole tiles around the written rows: a tile two uploads share is quantised from both
        const int64_t t0 = ix->scr_lo / kTileRows;
        const int64_t t1 = std::min(tiles, (ix->scr_hi + kTileRows - 1) / kTileRows);
        for (int64_t t = t0; t < t1; t += 1 << 20) {
            quantize_tiles(t, (unsigned)std::min<int64_t>(1 << 20, t1 - t));
            HIP_TRY(hipGetLastError());
        }
        ix->scr_lo = ix->scr_hi = 0;
    }
    DEV_TRY(ix->scr_q.need((size_t)kMfmaQ * W));
    DEV_TRY(ix->scr_qmeta.need((size_t)kMfmaQ * 16));
    DEV_TRY(ix->scr_cand.need((size_t)kMfmaQ * kScreenCap * 8));
    DEV_TRY(ix->scr_count.need((size_t)kMfmaQ * 4));
    if (quantize_queries) {
        quantize_query_rows();
        HIP_TRY(hipGetLastError());
    }
    return TS_OK;
}

template <int W>
static int screen_prepare_w(ts_index* ix, const void* qmat, int nq_launch, bool quantize_queries, hipStream_t st) {
    return screen_prepare_with<W>(
        ix, quantize_queries,
        [&](int64_t tile0, unsigned nblk) {
            quantize_tiles_kernel<W><<<nblk, 256, 0, st>>>(ix->rows.as<const unsigned short>(), ix->scr_rows.as<signed char>(), ix->scr_tile.as<float4>(), tile0);
        },
        [&] {
            quantize_queries_kernel<W><<<kMfmaQ, 64, 0, st>>>((const unsigned short*)qmat, std::min(nq_launch, kMfmaQ), ix->scr_q.as<signed char>(),
                                                           ix->scr_qmeta.as<float4>(), ix->scr_count);
        });
}

// The screen's launch of the full pass: the tile kernel over the image, `a` being the unscreened pass's argument block
// (thresholds, row mask, tile table); its (row, query) pairs go to the screen's lists.
// variant: a timing-only form of the screen (variant_screen_diag; diagnostic build; wrong results), or kVariantProduct.
// late: the bf16 full pass of d = 768 may take the late-test form of the kernel (TS_MFMA_SCREEN_LATE, launch_screen8_late.hip) -
// which exists for four query blocks per wave, no row mask and the product only; every other launch takes the kernels of this unit.
template <int W>
static int screen_tile_pass_w(ts_index* ix, int nb, int grid, int variant, hipStream_t st, const MfmaArgs& a, bool late = false) {
    MfmaArgs s = a;
    s.corpus = ix->scr_rows.as<const unsigned short>();
    s.q = ix->scr_q.as<const unsigned short>();
    s.cand = ix->scr_cand;
    s.count = ix->scr_count;
    s.cap = kScreenCap;
    s.scr_tile = ix->scr_tile.as<const float4>();
    s.scr_q = ix->scr_qmeta.as<const float4>();
    if constexpr (W == 768)
        if (late && nb == 4 && variant == kVariantProduct && s.row_mask == nullptr) return launch_screen8_late(ix->device, grid, st, s);
    switch (nb) {
        case 1: return launch_screen8<W, 1>(ix->device, grid, variant, st, s);
        case 2: return launch_screen8<W, 2>(ix->device, grid, variant, st, s);
        case 3: return launch_screen8<W, 3>(ix->device, grid, variant, st, s);
        case 4: return launch_screen8<W, 4>(ix->device, grid, variant, st, s);
        default: return fail(TS_ERR_INTERNAL, "no int8 screen with %d query blocks per wave", nb);
    }
}

// The full pass, screened: `a` is the bf16 pass's argument block (thresholds, row mask, tile table, the final select's lists).
// ksplit (W = 1024): the unscreened pass of this call would have been the paired k-split form - the rescore adds its two
// half-chains as that form does.
template <int W>
static int screen_full_pass_w(ts_index* ix, int nb, int nq, int grid, int variant, bool ksplit, hipStream_t st, const MfmaArgs& a) {
    TS_TRY(screen_tile_pass_w<W>(ix, nb, grid, variant, st, a, W == 768 && ix->dtype == TS_BF16 && ix->knobs.get(K_MFMA_SCREEN_LATE, 1) != 0));
    ScreenRescoreArgs r;
    r.rows = ix->rows.as<const unsigned short>();
    r.q = a.q;
    r.thr = a.thr;
    r.scand = ix->scr_cand;
    r.scount = ix->scr_count;
    r.cand = a.cand;
    r.count = a.count;
    r.cap = a.cap;
    if constexpr (W == 1024) {
        if (ksplit) screen_rescore_kernel<W, true><<<dim3((unsigned)nq, kRescoreY), 256, 0, st>>>(r);
        else screen_rescore_kernel<W, false><<<dim3((unsigned)nq, kRescoreY), 256, 0, st>>>(r);
    } else {
        if (ksplit) return fail(TS_ERR_INTERNAL, "the k-split rescore is a form of the d = 1024 pass, not of d = %d", W);
        screen_rescore_kernel<W, false><<<dim3((unsigned)nq, kRescoreY), 256, 0, st>>>(r);
    }
    HIP_TRY(hipGetLastError());
    return TS_OK;
}
