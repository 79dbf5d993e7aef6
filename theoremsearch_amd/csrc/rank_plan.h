// The many-targets rank pass's host decisions (kernels_rank_mfma.h, rank_many.hip) as pure functions of plain values: which
// (storage type, width) the matrix pass serves, the tile and the LDS bytes of its launch.  Nothing from HIP: the C ABI's codes
// (include/tsearch.h, plain C) only, so tests/rank_plan_check.cpp runs all of it on the CPU under the host sanitizers.
#pragma once
#include "../../include/tsearch.h"

namespace ts {

constexpr int kRankQueries = 256;        // queries of one launch: 8 waves x 2 blocks of 16
constexpr int kRankT = 16;               // targets per query per pass (the host splits longer lists into passes)
constexpr int kRankMinD = 128;
constexpr int kRankMaxRowBytes = 4096;   // a 32-row tile + padding still fits the LDS (32 x 4,112 = 131,584 bytes)
constexpr int kRankRowPad = 16;          // bytes between LDS rows: 16-row fragment reads spread over the banks
constexpr int kRankLdsLimit = 160 * 1024;

constexpr int rank_row_bytes(int dtype, int d) { return d * (dtype == TS_BF16 ? 2 : 4); }

// The widths of ts_rank_many's / ts_count_above_many's matrix pass: every multiple of 64 from 128 up to a 4,096-byte row (bf16
// up to d = 2048, fp32 up to d = 1024), the rule of the batched searches (anyd_plan.h) with the four hand-laid widths included.
// Rows of such a width are stored unpadded (ld == d).  Every other width takes one streaming pass per target column.
constexpr bool rank_many_served(int dtype, int d) {
    return (dtype == TS_BF16 || dtype == TS_F32) && d >= kRankMinD && d % 64 == 0 && rank_row_bytes(dtype, d) <= kRankMaxRowBytes;
}

// k-steps of 64 bytes per row quarter (bf16: 32 elements, fp32: 16), issued in groups of four.  A bf16 width with d % 128 == 64
// ends in a group of two: the kernel form with the tail group (TAIL).  fp32 has none: d / 16 is a multiple of 4.
constexpr int rank_steps(int dtype, int d) { return d / (dtype == TS_BF16 ? 32 : 16); }
constexpr bool rank_tail(int dtype, int d) { return rank_steps(dtype, d) % 4 != 0; }

// RB = row blocks of 16 per tile: 4 while a 64-row tile fits the LDS (row <= 2,048 bytes: bf16 at d <= 1024, fp32 at d <= 512),
// else 2
constexpr int rank_rb(int row_bytes) { return row_bytes <= 2048 ? 4 : 2; }
constexpr int rank_tile_rows(int row_bytes) { return 16 * rank_rb(row_bytes); }
constexpr int rank_lds_bytes(int rb, int row_bytes) { return 16 * rb * (row_bytes + kRankRowPad); }
// the largest launch of each RB: what the kernel's LDS limit is raised to, once
constexpr int rank_lds_max(int rb) { return rank_lds_bytes(rb, rb == 4 ? 2048 : kRankMaxRowBytes); }

static_assert(rank_lds_max(4) == 132096 && rank_lds_max(2) == 131584, "64 x 2,064 and 32 x 4,112 bytes");
static_assert(rank_lds_max(4) <= kRankLdsLimit && rank_lds_max(2) <= kRankLdsLimit, "every served row's tile fits the CU's LDS");
static_assert(rank_rb(2048) == 4 && rank_rb(2049) == 2 && rank_rb(kRankMaxRowBytes) == 2, "the tile halves past a 2,048-byte row");
static_assert(256 % rank_tile_rows(128) == 0 && 256 % rank_tile_rows(kRankMaxRowBytes) == 0, "whole tiles inside an allocation padded to 256 rows");

}  // namespace ts
