// The corpus-moments pass's host decisions (kernels_moments.h, moments.hip) as pure functions of plain values: the widths it
// serves, the column panels and the list of panel pairs, the rows a workgroup accumulates in fp32 before it adds them in
// double (L), the split of the rows into ranges, the bytes of the partial tiles and of the LDS image, the grid, and the LDS
// image itself (where a 16-byte chunk of a staged row lies).  Nothing from HIP: the C ABI's codes (include/tsearch.h, plain
// C) only, so tests/moments_plan_check.cpp runs all of it on the CPU under the host sanitizers.
//
// Shape of the pass.  The Gram matrix X^T X is a SYRK whose summed index is the corpus row.  The d columns are cut into
// panels of kMomPanel; a workgroup owns one PAIR of panels (pi <= pj: the upper triangle) and one range of 64-row tiles,
// stages the two panels of every tile into LDS and multiplies them column-wise on the matrix pipe, accumulators in
// registers.  The column sums and the per-group sums are the same product with an indicator block [group][row] built in
// registers as the left operand: there a workgroup owns one panel, one chunk of kMomGroupChunk groups and one row range.
//
// L = kMomFlushRows.  A workgroup adds products in fp32 for at most L consecutive rows, then adds its accumulators IN DOUBLE
// into its own partial tile in global memory and starts again from zero, so an output element is a double sum of fp32
// chains of at most L terms: its error is bounded by (L + 2) 2^-23 sum |x_ri x_rj| whatever n is (first-order bound of an fp32
// chain of L terms in any order, doubled; bf16 products are exact in fp32, an fp32 product adds one rounding).  L = 8,192
// keeps that factor below 1e-3 of the absolute sum in the worst case (about sqrt(L) 2^-24 = 5e-6 typical), and makes the
// flush - a read-modify-write of 128 KiB of doubles per workgroup - 1/16 of the 2 MiB of bf16 rows the workgroup reads
// between two flushes (1/32 on fp32).  A smaller L buys accuracy nobody needs with traffic; a larger one saves little.
#pragma once
#include <stdint.h>

#include "../../include/tsearch.h"

namespace ts {

constexpr int kMomMinD = 128;
constexpr int kMomMaxD = 1024;
constexpr int kMomPanel = 128;             // columns of a panel: a 128 x 128 output tile per workgroup, 64 x 64 per wave
constexpr int kMomTileRows = 64;           // rows staged per tile (index allocations are padded to 256 rows: common.h kRowPad)
constexpr int kMomThreads = 256;           // four waves: the quadrants of the output tile
constexpr int kMomFlushRows = 8192;        // L
constexpr int kMomGroupChunk = 64;         // groups of one workgroup of the indicator pass (four blocks of 16)
constexpr int kMomMaxGroups = 256;
constexpr int kMomSubBytes = 128;          // the LDS image is made of sub-images [64 rows][128 bytes]: 64 bf16 / 32 fp32 columns
constexpr int kMomLdsLimit = 160 * 1024;
constexpr int64_t kMomPartialCap = (int64_t)256 << 20;
constexpr int kMomBlocksPerCU = 2;         // workgroups per CU the row-range split fills (what the fp32 launch's 64 KiB of LDS admit)
constexpr int kMomMaxRanges = 512;

static_assert(kMomFlushRows % kMomTileRows == 0, "a flush falls on a tile boundary");
static_assert(kMomPanel % 64 == 0 && kMomMinD % 64 == 0, "panels are made of whole 128-byte sub-images at every served width");

constexpr int mom_elem(int dtype) { return dtype == TS_BF16 ? 2 : 4; }
constexpr bool mom_served(int dtype, int d) {
    return (dtype == TS_BF16 || dtype == TS_F32) && d >= kMomMinD && d <= kMomMaxD && d % 64 == 0;
}
constexpr int mom_panels(int d) { return (d + kMomPanel - 1) / kMomPanel; }
constexpr int mom_panel_cols(int d, int p) { return d - p * kMomPanel < kMomPanel ? d - p * kMomPanel : kMomPanel; }   // the last one may be 64
constexpr int mom_pairs(int d) { return mom_panels(d) * (mom_panels(d) + 1) / 2; }
// pair `idx` of the upper triangle, row by row: (0,0) (0,1) .. (0,P-1) (1,1) ..
constexpr void mom_pair(int panels, int idx, int* pi, int* pj) {
    int i = 0;
    while (idx >= panels - i) { idx -= panels - i; ++i; }
    *pi = i;
    *pj = i + idx;
}
constexpr int mom_group_chunks(int ngroups) { return (ngroups + kMomGroupChunk - 1) / kMomGroupChunk; }

// LDS: sub-images of one panel, bytes of a launch (pair pass: two panels; indicator pass: one)
constexpr int mom_panel_subs(int dtype) { return kMomPanel * mom_elem(dtype) / kMomSubBytes; }
constexpr int mom_lds_bytes(int dtype, bool pair) { return (pair ? 2 : 1) * mom_panel_subs(dtype) * kMomTileRows * kMomSubBytes; }
// Where 16-byte chunk `ch` (0..7) of row `row` (0..63) of sub-image `sub` lies.  The chunk index is XOR-ed with a function of
// the row so that the fragment reads meet no bank conflict (cdna LDS: 64 banks of 4 bytes for the 64-bit transposed read, 32
// for the 32-bit read; conflicts count per half wave):
//   bf16: a half wave's transposed read takes 32 bytes (16 columns) of 8 consecutive rows r0 .. r0 + 7, r0 % 8 == 0; rows
//         128 bytes apart alternate between the two halves of the 256-byte bank row, and 2 ((row >> 1) & 3) moves each pair
//         of rows to another 32-byte slot pair: 8 rows, 8 distinct slot pairs;
//   fp32: a half wave's read takes 64 bytes (16 columns) of rows r, r + 1: 4 (row & 1) puts them in the two halves of the 128
//         bytes = 32 banks.
// Both staging (the chunk a DMA lane fetches) and the reads go through this one function.
constexpr int mom_swz(bool f32, int row) { return f32 ? 4 * (row & 1) : 2 * ((row >> 1) & 3); }
constexpr int mom_lds_off(bool f32, int sub, int row, int ch) {
    return (sub * kMomTileRows + row) * kMomSubBytes + 16 * (ch ^ mom_swz(f32, row));
}

// What a lane reads and fetches, so that tests/moments_plan_check.cpp can replay the kernel's addressing on the CPU.
// mom_frag_off: byte offset of the lane's fragment read of 16-column block `cb` of the panel whose first sub-image is
// `sub_base`, at the tile's first k-step.
//   bf16: the address lane 4 q + p of lane group g = lane >> 4 hands the transposed read - row 4 g + q of the step, columns
//         16 cb + 4 p .. + 3 (a multiple of 8 bytes); the lane RECEIVES column 16 cb + (lane & 15) of rows 4 g .. 4 g + 3.  The
//         operand's second read lies kMomTrSecond bytes on (rows 16 + 4 g ..), the next k-step mom_step_bytes on: neither
//         changes bits 1 and 2 of the row, so the XOR of mom_lds_off stays what it is.
//   fp32: the float of column 16 cb + (lane & 15), row lane >> 4 of the step; the next step (4 rows) mom_step_bytes on.
constexpr int mom_frag_off(bool f32, int lane, int sub_base, int cb) {
    const int bps = f32 ? 2 : 4, sub = sub_base + cb / bps, b = cb % bps, g = lane >> 4;
    if (f32) return mom_lds_off(true, sub, g, 4 * b + ((lane & 15) >> 2)) + 4 * (lane & 3);
    const int q = (lane >> 2) & 3, p = lane & 3;
    return mom_lds_off(false, sub, 4 * g + q, 2 * b + (p >> 1)) + 8 * (p & 1);
}
constexpr int mom_step_bytes(bool f32) { return (f32 ? 4 : 32) * kMomSubBytes; }
constexpr int kMomTrSecond = 16 * kMomSubBytes;
// bf16: the row of the 32-row k-step that element e (0..7) of a lane's fragment holds
constexpr int mom_frag_row(int lane, int e) { return e < 4 ? 4 * (lane >> 4) + e : 16 + 4 * (lane >> 4) + e - 4; }
// staging: one wave instruction moves rows r8 .. r8 + 7 of a sub-image, lane -> LDS slot 16 * lane behind (sub, r8, chunk 0):
// the lane's row is r8 + (lane >> 3), and it fetches the chunk that belongs in its slot
constexpr int mom_stage_chunk(bool f32, int lane, int r8) { return (lane & 7) ^ mom_swz(f32, r8 + (lane >> 3)); }

// tiles and row ranges: `units` = workgroups per range (panel pairs, or panels x group chunks), unit_bytes = one partial tile
constexpr int64_t mom_tiles(int64_t n) { return (n + kMomTileRows - 1) / kMomTileRows; }
constexpr int64_t mom_pair_tile_bytes() { return (int64_t)kMomPanel * kMomPanel * 8; }
constexpr int64_t mom_group_tile_bytes() { return (int64_t)kMomGroupChunk * kMomPanel * 8; }
constexpr int mom_ranges(int64_t n, int cu_count, int units, int64_t unit_bytes) {
    const int64_t tiles = mom_tiles(n);
    if (tiles <= 0 || units <= 0) return 0;
    // rounded DOWN: units x ranges workgroups never exceed the kMomBlocksPerCU x CUs that run at once, so the launch is one round
    // of equal shares (rounded up, 36 pairs x 15 ranges = 540 workgroups met 512 places: a second round for 28 of them)
    int64_t r = (int64_t)kMomBlocksPerCU * (cu_count > 0 ? cu_count : 1) / units;
    const int64_t cap = kMomPartialCap / (units * unit_bytes);
    if (r > cap) r = cap;
    if (r > kMomMaxRanges) r = kMomMaxRanges;
    if (r > tiles) r = tiles;
    return r < 1 ? 1 : (int)r;
}
constexpr int64_t mom_partial_bytes(int ranges, int units, int64_t unit_bytes) { return (int64_t)ranges * units * unit_bytes; }
// rows [*r0, *r1) of range i of `ranges`: whole tiles, the last one cut at n rounded up to 32 (a mask word)
constexpr void mom_range_rows(int64_t n, int ranges, int i, int64_t* r0, int64_t* r1) {
    const int64_t tiles = mom_tiles(n), end = (n + 31) / 32 * 32;
    const int64_t a = tiles * i / ranges * kMomTileRows, b = tiles * (i + 1) / ranges * kMomTileRows;
    *r0 = a < end ? a : end;
    *r1 = b < end ? b : end;
}

struct MomGrid { int x, y; };              // x = unit (neighbours in x read the same rows: they meet in the caches), y = range
constexpr MomGrid mom_grid(int units, int ranges) { return MomGrid{units, ranges}; }

// registers: fp32 accumulators of one wave (four per 16 x 16 block)
constexpr int kMomPairAccRegs = (kMomPanel / 2 / 16) * (kMomPanel / 2 / 16) * 4;                 // 64 x 64 per wave: 64
constexpr int kMomGroupAccRegs = (kMomGroupChunk / 16) * (kMomPanel / 4 / 16) * 4;               // 64 groups x 32 columns per wave: 32
static_assert(kMomPairAccRegs <= 128 && kMomGroupAccRegs <= 128, "accumulators leave half of a 256-register wave to the fragments");
static_assert(mom_lds_bytes(TS_F32, true) <= kMomLdsLimit / 2, "two workgroups of the widest launch share a CU's LDS");
static_assert(mom_pairs(kMomMaxD) * mom_pair_tile_bytes() * 2 <= kMomPartialCap, "the widest index still gets two row ranges under the cap");

}  // namespace ts
