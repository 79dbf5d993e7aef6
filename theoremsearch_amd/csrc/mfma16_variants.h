// The VARIANT values of mfma16_topk_kernel (kernels_mfma16.h) and of TS_MFMA_VARIANT, named once: the kernel, the planning and
// read-out of search_mfma.hip and the instantiation lists of launch_mfma16.hip / launch_screen8_impl.h all read these names and
// predicates.  Plain ints with fixed values: TS_MFMA_VARIANT is a user-visible option, the mangled kernel names contain the
// values, and the ISA tests find kernels by those names.
// (The 32x32 kernels number their variants differently - in kernels_mfma.h 3 is the cycle stamps and 4 .. 7 are the wait-less
// forms - and keep their digits: launch_mfma32.hip.)
#pragma once

namespace ts {

// 0 = the product kernel.
constexpr int kVariantProduct = 0;
// Timing-only diagnostics (wrong results; the diagnostic build, make diag, only): 1 = no epilogue,
constexpr int kVariantNoEpilogue = 1;
// 2 = DMA stream only,
constexpr int kVariantDmaOnly = 2;
// 3 = product + clock probe: s_memtime / s_memrealtime around the tile loop into a.dbg
// (4 words per workgroup: shader cycles, 100 MHz ticks, units, 0) - MI355X_MICROARCH.md "DVFS give-back" item 6.
constexpr int kVariantClockProbe = 3;
// 4 = threshold test without the append path,
constexpr int kVariantTestOnly = 4;
// 5 = product + per-unit cycle stamps around the vmcnt wait, the barrier and each DMA issue (sums per wave into a.dbg; the
// stamps drain the LDS queue: read the SHARES, not the length).
constexpr int kVariantStamps = 5;
// 6 = product + s_sleep of ~256 cycles per unit (how much of an added idle cycle shows up as time under the power cap).
constexpr int kVariantSleep = 6;
// 7 = no DMA (MFMA + LDS reads).
constexpr int kVariantNoDma = 7;
// 8 = the int8 screen (I8 in the kernel; kernels_screen8.h), the unmasked product: it holds no code that reads
// MfmaArgs::row_mask.
constexpr int kVariantScreen = 8;
// Its timing-only forms (the diagnostic build, I8 as well): 9 = no epilogue,
constexpr int kVariantScreenNoEpilogue = 9;
// 10 = cycle stamps around the vmcnt wait, the barrier and the tile tail (the drain to the end of the epilogue; a.dbg as 5, the
// tail in place of the DMA issue),
constexpr int kVariantScreenStamps = 10;
// 11 = clock probe (as 3),
constexpr int kVariantScreenClockProbe = 11;
// 12 = DMA stream only,
constexpr int kVariantScreenDmaOnly = 12;
// 13 = the block test without the append path and the flush (the screen's form of 4: product - 13 = what the admitted pairs
// cost inside the launch, 13 - 9 = the fall-through tail).
constexpr int kVariantScreenTestOnly = 13;
// 14 = the screen of a search with a row mask (a product kernel): 8 holds no code that reads MfmaArgs::row_mask; 14 and the
// product-with-instruments forms 10, 11 test the mask (when there is one) before a pair is staged.
constexpr int kVariantScreenMasked = 14;
// 15 = the late-test screen (a product kernel; TS_MFMA_SCREEN_LATE, launch_screen8_late.hip): the unmasked screen of d = 768 with
// four query blocks per wave, whose block tests of tile t - 1 stand in MFMA gaps of tile t (two accumulator sets by tile parity)
// and whose admitted pairs are staged one tile late.  The same pairs as 8.
constexpr int kVariantScreenLate = 15;

constexpr bool variant_is_screen(int v) { return v >= kVariantScreen && v <= kVariantScreenLate; }                    // I8
constexpr bool variant_screen_diag(int v) { return v >= kVariantScreenNoEpilogue && v <= kVariantScreenTestOnly; }    // the screen's timing-only forms
constexpr bool variant_masked(int v) { return variant_is_screen(v) && v != kVariantScreen && v != kVariantScreenLate; }    // the row mask is looked at (8, 15: the unmasked products)
constexpr bool variant_late(int v) { return v == kVariantScreenLate; }                           // block tests one tile late
constexpr bool variant_no_epilogue(int v) { return v == kVariantNoEpilogue || v == kVariantNoDma || v == kVariantScreenNoEpilogue; }
constexpr bool variant_no_mma(int v) { return v == kVariantDmaOnly || v == kVariantScreenDmaOnly; }
constexpr bool variant_no_dma(int v) { return v == kVariantNoDma; }
constexpr bool variant_stamped(int v) { return v == kVariantStamps || v == kVariantScreenStamps; }       // cycle stamps (general units only)
constexpr bool variant_probe(int v) { return v == kVariantClockProbe || v == kVariantScreenClockProbe; } // clock probe
constexpr bool variant_test_only(int v) { return v == kVariantTestOnly || v == kVariantScreenTestOnly; } // the block test without the append path
// the forms the k-split pass is instantiated for
constexpr bool variant_ksplit_form(int v) { return v == kVariantProduct || v == kVariantNoEpilogue || v == kVariantDmaOnly || v == kVariantNoDma; }
// MfmaArgs::dbg is handed to every diagnostic variant from 3 on, in either kernel's numbering (the lowest one that writes it is
// 3 in both: the clock probe here, the stamps of kernels_mfma.h)
constexpr bool variant_gets_dbg(int v) { return v >= kVariantClockProbe; }

}  // namespace ts
