// The grouped search's two kernels (include/tsearch.h: ts_search_grouped; group_plan.h holds the ladder they serve).
//   collapse_kernel       a query's sorted result list -> its group-firsts, in order, with the certificate of the list
//   group_exclude_kernel  a row mask without the rows of the groups found so far: the sibling of meta_eval_kernel
// Both are small and memory-bound by construction: 12 bytes per list entry plus one gathered code; 4 bytes per row plus the
// base mask's bit.
#pragma once
#include "common.h"
#include "group_plan.h"
#include "meta_plan.h"

namespace ts {

struct CollapseArgs {
    const float* scores;        // [nq][k_in], each list in canonical order (score descending, id ascending), padding anywhere
    const int64_t* idx;         // [nq][k_in] global ids; outside [row_offset, row_offset + n): padding
    int k_in, k_out;
    const int32_t* column;      // [n] the group code per local row
    int64_t n, row_offset;
    const int32_t* qmap;        // optional: list q belongs to query qmap[q] of the outputs (the gathered batch of stage 2)
    float* out_scores;          // [.][k_out]
    int64_t* out_idx;
    int32_t* out_groups;
    int32_t* out_found;         // optional [.]: group-firsts in the whole list
    int32_t* out_complete;      // optional [.]: 1 = the k_out slots are the exact answer
};

// One list per workgroup, one entry per thread (k_in <= T).  An entry is kept when its code is NULL or when no earlier entry
// of the list carries the code; the kept entries are compacted in list order (ballot per wave, prefix across the waves).  The
// lists are taken as sorted: nothing is compared but codes.  An entry with a NaN score is padding (no search returns one).
template <int T>
__global__ __launch_bounds__(T) void collapse_kernel(const CollapseArgs a) {
    constexpr int kWaves = T / kWave;
    __shared__ int32_t s_code[T];
    __shared__ unsigned char s_valid[T];
    __shared__ int s_kept[kWaves], s_pad[kWaves];
    const int j = threadIdx.x, lane = j & (kWave - 1), wave = j / kWave;
    const int64_t in = (int64_t)blockIdx.x * a.k_in + j;
    float s = -INFINITY;
    int64_t id = -1;
    int32_t code = TS_META_NULL;
    bool valid = false;
    if (j < a.k_in) {
        s = a.scores[in];
        id = a.idx[in];
        // unsigned: an id below row_offset wraps far past n
        valid = id >= 0 && s == s && (u64)id - (u64)a.row_offset < (u64)a.n;
        if (valid) code = a.column[id - a.row_offset];
    }
    s_code[j] = code;
    s_valid[j] = valid ? 1 : 0;
    __syncthreads();
    bool keep = valid;
    if (valid && code != TS_META_NULL) {
        for (int i = 0; i < j; ++i)
            if (s_valid[i] && s_code[i] == code) { keep = false; break; }
    }
    const u64 kept = __ballot(keep);                       // all lanes are here again
    const u64 pads = __ballot(j < a.k_in && !valid);
    if (lane == 0) {
        s_kept[wave] = __popcll(kept);
        s_pad[wave] = pads != 0;
    }
    __syncthreads();
    int before = 0, found = 0, padded = 0;
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) before += s_kept[w];
        found += s_kept[w];
        padded |= s_pad[w];
    }
    const int q = a.qmap ? a.qmap[blockIdx.x] : blockIdx.x;
    const int64_t out = (int64_t)q * a.k_out;
    const int pos = before + __popcll(kept & ((1ull << lane) - 1ull));
    if (keep && pos < a.k_out) {
        a.out_scores[out + pos] = s;
        a.out_idx[out + pos] = id;
        a.out_groups[out + pos] = code;
    }
    for (int p = found + j; p < a.k_out; p += T) {
        a.out_scores[out + p] = -INFINITY;
        a.out_idx[out + p] = -1;
        a.out_groups[out + p] = TS_META_NULL;
    }
    if (j == 0) {
        if (a.out_found) a.out_found[q] = found;
        if (a.out_complete) a.out_complete[q] = group_certified(found, a.k_out, padded != 0) ? 1 : 0;
    }
}

struct GroupExcludeArgs {
    int64_t n;
    int64_t nblocks;            // blocks of kMetaBlockRows rows = the mask's allocation
    const u32* base;            // optional: the mask to start from (a row set's: whole blocks, zero past n)
    const int32_t* column;      // [n]
    const int32_t* codes;       // [ncodes] ascending; never TS_META_NULL
    const int64_t* rows;        // [nrows] ascending local rows
    int ncodes, nrows;          // each <= kGroupMaxList
    u32* mask;                  // [nblocks * 8] words, every one written here
    u64* allowed;               // zeroed on the launch's stream before it
};

// base AND NOT (the row's code is in `codes`) AND NOT (the row is in `rows`).  One lane per row, as meta_eval_kernel: a
// workgroup walks the blocks blockIdx.x, blockIdx.x + gridDim.x, ...; lanes past n vote 0 but take part in the ballot, so
// every word of the allocation is written, zero past n.  The two lists wait in LDS.
__global__ __launch_bounds__(kMetaThreads) void group_exclude_kernel(const GroupExcludeArgs a) {
    static_assert(kMetaThreads >= kGroupMaxList, "one thread stages one entry of each list");
    __shared__ int32_t s_codes[kGroupMaxList];
    __shared__ int64_t s_rows[kGroupMaxList];
    __shared__ u64 wave_count[kMetaThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if ((int)threadIdx.x < a.ncodes) s_codes[threadIdx.x] = a.codes[threadIdx.x];
    if ((int)threadIdx.x < a.nrows) s_rows[threadIdx.x] = a.rows[threadIdx.x];
    __syncthreads();
    u64 count = 0;                                   // rows this wave allowed (the same in all its lanes)
    for (int64_t blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {
        const int64_t row = blk * kMetaBlockRows + threadIdx.x;
        bool pass = false;
        if (row < a.n) {
            pass = !a.base || ((a.base[row >> 5] >> (row & 31)) & 1u);
            if (pass && a.ncodes) pass = !sorted_has(s_codes, a.ncodes, a.column[row]);
            if (pass && a.nrows) pass = !sorted_has(s_rows, a.nrows, row);
        }
        const u64 votes = __ballot(pass);            // all 64 lanes are here again
        if (lane < 2) a.mask[(blk * kMetaBlockRows + wave * kWave) / 32 + lane] = (u32)(votes >> (32 * lane));
        count += (u64)__popcll(votes);
    }
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 total = 0;
        for (int w = 0; w < kMetaThreads / kWave; ++w) total += wave_count[w];
        if (total) atomicAdd(a.allowed, total);
    }
}

}  // namespace ts
