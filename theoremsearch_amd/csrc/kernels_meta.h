// The metadata filter: a program of atoms (include/tsearch.h: ts_atom; meta_plan.h lays it out) over the columns of a ts_meta,
// evaluated to the row bitmask of ts_search_filtered and its population count in one pass.  Memory-bound by construction: 4
// bytes per row and scalar column the program names, 16 bytes of offsets plus the codes per row of a list column.
#pragma once
#include "common.h"
#include "meta_plan.h"

namespace ts {

struct MetaKAtom {              // MetaAtom with its column and its set resolved to device addresses
    int32_t kind, lo, hi;
    int32_t negate, slot;
    u32 set_bits;
    const int32_t* values;      // scalar column [n]; a list column's codes
    const int64_t* offsets;     // list column: [n + 1]
    const u32* set;
};

// The whole program travels as the kernel's argument (32 x 48 bytes + the rest, within the 4 KiB of a launch): the atom index
// is uniform, so the atoms are read with scalar loads from the argument segment.
struct MetaArgs {
    int64_t n;
    int64_t nblocks;            // blocks of kMetaBlockRows rows = the mask's allocation
    int32_t natoms;
    u32 all_groups;             // verdict bits of a passing row
    u32* mask;                  // [nblocks * 8] words, every one written here
    u64* allowed;               // zeroed on the launch's stream before it
    MetaKAtom atom[TS_META_MAX_ATOMS];
};

__device__ __forceinline__ bool set_has(const u32* set, u32 set_bits, int32_t code) {
    return code >= 0 && (u32)code < set_bits && ((set[(u32)code >> 5] >> ((u32)code & 31u)) & 1u);
}

// One lane per row; a workgroup walks the blocks blockIdx.x, blockIdx.x + gridDim.x, ...  Lanes whose row is >= n evaluate
// nothing and vote 0, but take part in the ballot: the tail wave writes its full words, zero past n, and the waves behind
// it in the last block write zero words - the allocation is whole blocks (meta_plan.h: mask_alloc_words).
__global__ __launch_bounds__(kMetaThreads) void meta_eval_kernel(const MetaArgs a) {
    __shared__ u64 wave_count[kMetaThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    u64 count = 0;                                   // rows this wave allowed (the same in all its lanes)
    for (int64_t blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {
        const int64_t row = blk * kMetaBlockRows + threadIdx.x;
        bool pass = false;
        if (row < a.n) {
            u32 held = 0;
            for (int i = 0; i < a.natoms; ++i) {
                const MetaKAtom& t = a.atom[i];
                bool v;
                if (t.kind == TS_ATOM_ANY_IN) {
                    v = false;
                    const int64_t end = t.offsets[row + 1];
                    for (int64_t j = t.offsets[row]; j < end && !v; ++j) v = set_has(t.set, t.set_bits, t.values[j]);
                } else {
                    const int32_t x = t.values[row];
                    const bool null = x == TS_META_NULL;
                    if (t.kind == TS_ATOM_IS_NULL) v = null != (t.negate != 0);
                    else {
                        const bool in = t.kind == TS_ATOM_RANGE ? (t.lo <= x && x <= t.hi) : set_has(t.set, t.set_bits, x);
                        v = !null && (in != (t.negate != 0));
                    }
                }
                held |= (v ? 1u : 0u) << t.slot;
            }
            pass = held == a.all_groups;
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
