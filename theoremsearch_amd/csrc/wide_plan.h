// The k-chunked matrix kernel's host decisions (kernels_mfma_wide.h, search_mfma.hip) as pure functions of plain values: which
// (storage type, width) it serves, how a row is cut into k-chunks, the staging tile, the LDS bytes of its two launches (the
// full pass and the threshold sample), the batch from which AUTO prefers it to the scan.  Nothing from HIP: the C ABI's codes
// (include/tsearch.h, plain C) and anyd_plan.h only, so tests/wide_plan_check.cpp runs all of it on the CPU under the host
// sanitizers.
//
// The rule is a predicate of its own: anyd_served / bias_served (rows of at most 4,096 bytes, whole rows in LDS) stay what
// they are, and wide_served is disjoint from both and from the hand-laid widths.
#pragma once
#include "anyd_plan.h"

namespace ts {

constexpr int kWideQueries = kAnydQueries;    // queries of one launch: 8 waves x 2 blocks of 16
constexpr int kWideMaxRowBytes = 16384;       // bf16 d = 8,192, fp32 d = 4,096
constexpr int kWideChunkBytes = 1024;         // a k-chunk: what ONE LDS-DMA wave instruction writes (64 lanes x 16 bytes) = 16 k-steps
constexpr int kWideGroupBytes = 256;          // four k-steps of 64 bytes: the kernels read fragments in groups of four
constexpr int kWideRowPad = kAnydRowPad;      // bytes between LDS rows
constexpr int kWidePitch = kWideChunkBytes + kWideRowPad;
constexpr int kWideTileRows = 64;             // staging tile of the pass: four row blocks of 16
constexpr int kWideBuffers = 2;               // a chunk is staged into the buffer the previous chunk's MFMAs do not read
constexpr int kWideSampleRows = 32;           // rows of one workgroup of the threshold sample (kernels_sample.h's shape)
constexpr int kWideSampleLdsLimit = 144 * 1024;   // the sample's limit at the narrower widths (search_mfma.hip: kSampleLdsMax)

// two_level: the search is the usual two-level one (dense threshold sample + full pass): the kernel is a full pass only.
// d % 256 == 0: a bf16 row is then a multiple of 512 bytes, an fp32 row of 1,024 - whole groups of four k-steps in every
// chunk, the ragged last chunk included.
constexpr bool wide_served(int dtype, int d, bool two_level) {
    return (dtype == TS_BF16 || dtype == TS_F32) && two_level && d > 0 && d % 256 == 0 && anyd_row_bytes(dtype, d) > kAnydMaxRowBytes &&
           anyd_row_bytes(dtype, d) <= kWideMaxRowBytes;
}

// The chunks of a row: chunk c covers the bytes [1,024 c, 1,024 c + wide_chunk_bytes(row, c)) - all of 1,024 bytes except the
// last one of a bf16 row with d % 512 == 256, which is 512.
constexpr int wide_chunks(int row_bytes) { return (row_bytes + kWideChunkBytes - 1) / kWideChunkBytes; }
constexpr int wide_chunk_bytes(int row_bytes, int c) {
    return row_bytes - c * kWideChunkBytes < kWideChunkBytes ? row_bytes - c * kWideChunkBytes : kWideChunkBytes;
}

// LDS of the two launches: `buffers` chunks of `rows` rows each, whatever the row length
constexpr int wide_lds_bytes() { return kWideBuffers * kWideTileRows * kWidePitch; }            // 133,120
constexpr int wide_sample_lds_bytes() { return kWideBuffers * kWideSampleRows * kWidePitch; }   //  66,560: two workgroups a CU

// Largest batch AUTO still sends to the scan at these widths (AlgoInputs::scan_max_queries; scan_max_queries() drops it to 1
// for k > 64, where the scan serves one query per pass).  One pass of this kernel holds 256 queries whatever the batch, the
// scan pays a pass per four queries.  Measured on 1M rows, k = 10, scan against kernel in ms (profiles/wide_timing.json,
// DESIGN.md section 3.4): bf16 at 5 queries - two scan passes - 2.40 against 1.24 (d = 2560) and 3.04 against 1.89 (4096): the
// limit is the one scan pass.  fp32 d = 1536: 2.15 / 2.16 against 2.18 at 5 / 8 queries, 4.35 against 2.18 at 16 - two scan
// passes are still a shade ahead of the kernel's one (three would not be), so fp32 batches of up to 8 stay on the scan (as the biased search's do, bias_plan.h).
constexpr int kWideScanMaxQueries = 4;
constexpr int kWideScanMaxQueriesF32 = 8;
constexpr int wide_scan_max_queries(int dtype) { return dtype == TS_F32 ? kWideScanMaxQueriesF32 : kWideScanMaxQueries; }
// k > 64 (k = 100 measured): bf16 takes the kernel from two queries on (1.60 against 1.26 ms at d = 2560, 2.52 against 1.92 at
// 4096); two fp32 queries stay on the scan (1.89 against 2.20 ms), four take the kernel (3.68 against 2.21).  The limit for
// this (storage type, k); where it is above what scan_max_queries() lets through, search_choose keeps AUTO on the scan up to it.
constexpr int wide_scan_limit(int dtype, int k) { return k > 64 ? (dtype == TS_F32 ? 2 : 1) : wide_scan_max_queries(dtype); }

}  // namespace ts
