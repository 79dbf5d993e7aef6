// Cross-shard merge: per query, nparts * k_in (score, global id) pairs -> best k_out.  Global ids
// are 64-bit here, so the sort runs on (ordered score, id) pairs: score descending, then id ascending.  An entry with a
// negative id or a NaN score is padding; missing results are (-inf, -1).
#pragma once
#include "common.h"

namespace ts {

struct MergeArgs {
    const float* scores;   // part p: scores + p * part_stride (in floats), [nq][k_in]
    const int64_t* idx;    // part p: idx + p * part_stride_idx (in int64), [nq][k_in]
    int64_t part_stride, part_stride_idx;
    int nparts, nq, k_in, k_out;
    float* out_scores;     // [nq][k_out]
    int64_t* out_idx;
};

constexpr int kMergeMax = 4096;

// CAP = LDS entries per workgroup (>= the power of two that holds nparts * k_in).  The exchange of the sharded search
// merges 8 x 10 candidates per query: with CAP = 128 the workgroup is one wave and 1.5 KB of LDS, so the merge on the side
// stream does not take CU slots from the next batch's threshold sample (the 4,096-entry form holds 48 KB per workgroup).
template <int CAP>
__global__ void __launch_bounds__(256) merge_kernel(MergeArgs a) {
    __shared__ u32 so[CAP];
    __shared__ int64_t si[CAP];
    const int q = blockIdx.x;
    const int m = a.nparts * a.k_in;
    int P = 2;
    while (P < m) P <<= 1;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        u32 o = 0;
        int64_t id = INT64_MAX;
        if (i < m) {
            const int part = i / a.k_in, j = i - part * a.k_in;
            const int64_t off = (int64_t)q * a.k_in + j;
            const float s = a.scores[(int64_t)part * a.part_stride + off];
            const int64_t r = a.idx[(int64_t)part * a.part_stride_idx + off];
            if (r >= 0 && s == s) {
                o = ord_f32(s);
                id = r;
            }
        }
        so[i] = o;
        si[i] = id;
    }
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < (P >> 1); i += blockDim.x) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const u32 ao = so[lo], bo = so[hi];
                const int64_t ai = si[lo], bi = si[hi];
                const bool a_worse = (ao < bo) || (ao == bo && ai > bi);
                if (a_worse == desc && !(ao == bo && ai == bi)) {
                    so[lo] = bo; si[lo] = bi;
                    so[hi] = ao; si[hi] = ai;
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.k_out; i += blockDim.x) {
        const bool ok = i < P && si[i] != INT64_MAX;
        a.out_scores[(int64_t)q * a.k_out + i] = ok ? unord_f32(so[i]) : -INFINITY;
        a.out_idx[(int64_t)q * a.k_out + i] = ok ? si[i] : -1;
    }
}

// nparts * k_in <= kMergeMax (the caller refuses more)
inline void launch_merge(const MergeArgs& a, hipStream_t st) {
    const int m = a.nparts * a.k_in;
    if (m <= 128) merge_kernel<128><<<a.nq, 64, 0, st>>>(a);
    else if (m <= 1024) merge_kernel<1024><<<a.nq, 256, 0, st>>>(a);
    else merge_kernel<kMergeMax><<<a.nq, 256, 0, st>>>(a);
}

}  // namespace ts
