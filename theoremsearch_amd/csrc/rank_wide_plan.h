// The many-targets rank pass at the k-chunked row widths (kernels_rank_wide.h, rank_many.hip) as pure functions of plain
// values: which (storage type, width) it serves, the tile and the LDS bytes of its launches.  Nothing from HIP: rank_plan.h and
// wide_plan.h only, so tests/rank_wide_plan_check.cpp runs all of it on the CPU under the host sanitizers.
//
// The rule is a predicate of its own: rank_many_served (rows of at most 4,096 bytes, whole rows in LDS) stays what it is, and
// rank_wide_served is disjoint from it.  The staging - tile, chunk, pitch, buffers - is the k-chunked search's (wide_plan.h),
// taken from there and not restated.
#pragma once
#include "rank_plan.h"
#include "wide_plan.h"

namespace ts {

// The widths of the k-chunked rank pass: exactly those of the k-chunked search's full pass - bf16 or fp32, d % 256 == 0, a row of
// more than 4,096 and at most 16,384 bytes (bf16 d = 2,304 .. 8,192, fp32 d = 1,280 .. 4,096).  Rows of such a width are stored
// unpadded (ld == d).  Widths in that range that are no multiple of 256 keep one streaming pass per target column.
constexpr bool rank_wide_served(int dtype, int d) { return wide_served(dtype, d, /*two_level=*/true); }

constexpr int rank_wide_tile_rows() { return kWideTileRows; }
constexpr int rank_wide_lds_bytes() { return wide_lds_bytes(); }

static_assert(kRankQueries == kWideQueries, "one launch holds the same block of queries on both forms");
static_assert(kWideMaxRowBytes > kRankMaxRowBytes && kAnydMaxRowBytes == kRankMaxRowBytes, "the k-chunked widths begin where the whole-row widths end");
static_assert(rank_wide_lds_bytes() <= kRankLdsLimit, "the two chunk buffers of a tile fit the CU's LDS");
static_assert(256 % rank_wide_tile_rows() == 0, "whole tiles inside an allocation padded to 256 rows");

}  // namespace ts
