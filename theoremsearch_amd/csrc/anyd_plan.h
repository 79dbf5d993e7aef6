// The general-width matrix kernel's host decisions (kernels_mfma_anyd.h, search_mfma.hip) as pure functions of plain values:
// which (storage type, width) it serves, the staging tile and the LDS bytes of its launch, the queries a launch holds, the
// batch from which AUTO prefers it to the scan.  Nothing from HIP: the C ABI's codes (include/tsearch.h, plain C) only, so
// tests/anywidth_plan_check.cpp runs all of it on the CPU under the host sanitizers.
#pragma once
#include "../../include/tsearch.h"

namespace ts {

constexpr int kAnydQueries = 256;        // queries of one launch: 8 waves x 2 blocks of 16
constexpr int kAnydMinD = 128;
constexpr int kAnydMaxRowBytes = 4096;   // a 32-row tile + padding still fits the LDS (32 x 4,112 = 131,584 bytes), and the
                                         // threshold sample (kernels_sample.h: 32 rows per workgroup) passes its own limit
constexpr int kAnydRowPad = 16;          // bytes between LDS rows: 16-row fragment reads spread over the banks
constexpr int kAnydLdsLimit = 160 * 1024;

// the four widths of the hand-laid kernels (kernels_mfma16.h, kernels_mfma.h): never served by the general one
constexpr bool anyd_hand_laid(int d) { return d == 384 || d == 512 || d == 768 || d == 1024; }
constexpr int anyd_row_bytes(int dtype, int d) { return d * (dtype == TS_BF16 ? 2 : 4); }

// two_level: the search is the usual two-level one (dense threshold sample + full pass): the kernel is a full pass only
constexpr bool anyd_served(int dtype, int d, bool two_level) {
    return (dtype == TS_BF16 || dtype == TS_F32) && two_level && d >= kAnydMinD && d % 64 == 0 && !anyd_hand_laid(d) &&
           anyd_row_bytes(dtype, d) <= kAnydMaxRowBytes;
}

// staging tile: 64 rows while a row is at most 2,048 bytes, else 32 (row blocks of 16: 4 or 2)
constexpr int anyd_row_blocks(int row_bytes) { return row_bytes <= 2048 ? 4 : 2; }
constexpr int anyd_tile_rows(int row_bytes) { return 16 * anyd_row_blocks(row_bytes); }
constexpr int anyd_lds_bytes(int row_bytes) { return anyd_tile_rows(row_bytes) * (row_bytes + kAnydRowPad); }
constexpr int kAnydLdsMax = 64 * (2048 + kAnydRowPad);   // the largest launch: 132,096 bytes (32 x 4,112 = 131,584 is the other peak)

// Largest batch AUTO still sends to the scan at these widths (AlgoInputs::scan_max_queries; scan_max_queries() drops it to 1
// for k > 64, where the scan serves one query per pass).  One pass of this kernel holds 256 queries whatever the batch, so a
// small batch pays a whole pass; the scan pays a pass per four queries.  Measured on 1M rows (profiles/anywidth_timing.json,
// bf16 d = 192 and 1536, fp32 d = 640): at 5 queries - the smallest batch above one scan pass - the
// kernel is already the faster path on both storage types, so the limit is the one scan pass, as on the hand-laid widths.
constexpr int kAnydScanMaxQueries = 4;
constexpr int anyd_scan_max_queries(int /*dtype*/) { return kAnydScanMaxQueries; }
// k > 64: the scan serves one query per pass and scan_max_queries() drops the limit to 1.  On bf16 the kernel wins from two
// queries on (1M x 1536: 0.84 against 1.01 ms; 1M x 192: 0.23 against 0.52).  fp32 runs the matrix pipe at 1/16 of the bf16
// rate: on 1M x 640 its pass is 1.10 ms whatever the batch, two single-query scan passes 0.86 ms, four 1.63 ms - two fp32
// queries stay on the scan.  The limit to pass as AlgoInputs::scan_max_queries for this (storage type, k); where it is above
// what scan_max_queries() lets through (k > 64), search_choose keeps AUTO on the scan up to it.
constexpr int anyd_scan_limit(int dtype, int k) { return k > 64 ? (dtype == TS_F32 ? 2 : 1) : kAnydScanMaxQueries; }

}  // namespace ts
