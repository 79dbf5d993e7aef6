// The grouped search's host decisions (grouped.hip) as pure functions of plain values: the depths of the ladder (over-fetch,
// deepen, exclude), the certificate of a collapsed list, the validation of the three entries' arguments, and the membership
// test on a sorted list that the exclusion kernel runs per row.  No handle, no HIP call: the C ABI's codes
// (include/tsearch.h, plain C) and the standard library only, so tests/group_plan_check.cpp runs all of it on the CPU under the
// host sanitizers.  group_certified and sorted_has are also compiled for the device (TS_HD): collapse_kernel writes the
// certificate, group_exclude_kernel searches the lists it holds in LDS.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/tsearch.h"

#ifndef TS_HD
#if defined(__HIPCC__)
#define TS_HD __host__ __device__
#else
#define TS_HD
#endif
#endif

namespace ts {

constexpr int kGroupMaxList = 256;        // codes, and rows, one exclusion can name: TS_MAX_K groups found at the most
constexpr int kGroupFirstSlack = 16;
static_assert(kGroupMaxList == TS_MAX_K, "an exclusion holds every group a grouped search can have found");

// ---------------------------------------------------------------------------------------------
// the ladder
// ---------------------------------------------------------------------------------------------
// Stage 1 fetches twice the groups asked for, at least 16 rows more, at most the library's depth: 64 rows or fewer up to
// k = 32, where the scan still serves four queries per pass.
inline int group_first_depth(int k) { return std::min<int>(TS_MAX_K, std::max(2 * k, k + kGroupFirstSlack)); }
inline int group_deep_depth() { return TS_MAX_K; }
// stage 2 is a search of its own only where it fetches more than stage 1 did
inline bool group_has_deep_stage(int k) { return group_first_depth(k) < group_deep_depth(); }

// A prefix of the canonical row order determines a prefix of the group order: a collapsed list is the exact answer when it
// holds k_out group-firsts, or when the list it came from was not full (the allowed rows are exhausted).
TS_HD inline bool group_certified(int found, int k_out, bool had_padding) { return found >= k_out || had_padding; }

// ---------------------------------------------------------------------------------------------
// membership in a sorted list (ascending, duplicates allowed): binary search
// ---------------------------------------------------------------------------------------------
template <class T>
TS_HD inline bool sorted_has(const T* list, int count, T v) {
    int lo = 0, hi = count;                 // the first element >= v lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < count && list[lo] == v;
}

// sorted and unique, in place; the new length
template <class T>
inline int sort_unique(T* list, int count) {
    std::sort(list, list + count);
    return (int)(std::unique(list, list + count) - list);
}

// ---------------------------------------------------------------------------------------------
// arguments: NULL = valid, else the text of TS_ERR_INVALID; the sizes are judged before the pointers
// ---------------------------------------------------------------------------------------------
inline const char* group_depth_invalid(int k) {
    if (k < 1 || k > TS_MAX_K) return "k outside [1, TS_MAX_K]";
    return nullptr;
}

// ts_search_grouped: what it checks before the first search (the searches check the rest as ts_search_rowset does)
inline const char* grouped_args_invalid(bool has_index, bool has_queries, bool has_meta, bool has_scores, bool has_idx, int q_dtype,
                                        int nq, int k, int algo) {
    if (q_dtype != TS_F32 && q_dtype != TS_BF16) return "q_dtype is neither TS_F32 nor TS_BF16";
    if (nq < 0) return "nq is negative";
    if (group_depth_invalid(k)) return group_depth_invalid(k);
    if (algo < TS_ALGO_AUTO || algo > TS_ALGO_MFMA) return "algo out of range";
    if (!has_index || !has_queries || !has_meta || !has_scores || !has_idx) return "NULL argument";
    return nullptr;
}

inline const char* collapse_args_invalid(bool has_scores, bool has_idx, bool has_column, bool has_out_scores, bool has_out_idx, int nq,
                                         int k_in, int k_out, int64_t n, int64_t row_offset) {
    if (nq < 0) return "nq is negative";
    if (k_in < 1 || k_in > TS_MAX_K) return "k_in outside [1, TS_MAX_K]";
    if (k_out < 1) return "k_out is less than 1";
    if (n < 0) return "n is negative";
    if (row_offset < 0) return "row_offset is negative";
    if (!has_scores || !has_idx || !has_column || !has_out_scores || !has_out_idx) return "NULL argument";
    return nullptr;
}

// the lists as the caller gave them (unsorted); n = the table's rows
inline const char* exclude_args_invalid(bool has_meta, bool has_out, const int32_t* codes, int ncodes, const int64_t* local_rows, int nrows,
                                        int64_t n) {
    if (ncodes < 0 || ncodes > kGroupMaxList) return "ncodes outside [0, 256]";
    if (nrows < 0 || nrows > kGroupMaxList) return "nrows outside [0, 256]";
    if (!has_meta || !has_out) return "NULL argument";
    if (ncodes > 0 && !codes) return "codes is NULL";
    if (nrows > 0 && !local_rows) return "local_rows is NULL";
    for (int i = 0; i < ncodes; ++i)
        if (codes[i] == TS_META_NULL) return "TS_META_NULL is not a code: NULL rows are groups of their own, excluded by row";
    for (int i = 0; i < nrows; ++i)
        if (local_rows[i] < 0 || local_rows[i] >= n) return "a row lies outside [0, n)";
    return nullptr;
}

}  // namespace ts
