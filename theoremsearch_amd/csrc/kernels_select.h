// Selection of the best keys of a candidate list in LDS - what every search ends in - and the scan path's select rounds.
// Shared by the paths: the LDS layout (SelectLds), lds_select_top and its stages, the one-wave register sort, the result
// slot.  The matrix path's threshold and final select are in kernels_level.h, the cross-shard merge in kernels_merge.h.
//
// Replaces the reference's full sorts: np.argsort(-scores)[:k] (app_scratchpad.py:130,
// compare_embeddings.py:52), torch.topk(scores, k, sorted=True) (app_showcase_model.py:96) and
// Postgres' top-N heapsort behind ORDER BY ... LIMIT k (streamlit_app.py:282-283).  Order rule:
// score descending, then row ascending (unsigned order of the 64-bit keys, common.h).
#pragma once
#include <math.h>

#include "../../include/tsearch.h"
#include "common.h"

namespace ts {

constexpr int kMaxK = 256;             // keys a select returns at most: the per-wave lists and the key registers are sized by it
static_assert(kMaxK == TS_MAX_K, "the select kernels are sized for the k the C ABI admits");

constexpr int kLevelSortMax = 8192;
constexpr int kLevelThreads = 512;
constexpr int kLevelSmall = 2048;      // keys the direct sort takes (after the histogram cut)
constexpr int kLevelBins = 1024;

// The dynamic LDS of a kernel that runs lds_select_top, in this order:
//   gathered keys [nkeys] | short list (sorted in place) [kLevelSmall] | per-wave lists of the streaming path
//   [kLevelThreads / 64][kMaxK] | histogram [kLevelBins] | 16 counter words.
// The counter words have names (SelectCtr): the caller fills keys[0 .. cnt) and owns kSelFill (and, in level_select_kernel,
// kSelProduced and kSelSharedBase); the others are lds_select_top's.  Plain indices, not accessor functions: a member
// function that hands out a reference into ctr moves the instructions of every kernel that holds the struct.
enum SelectCtr {
    kSelFill = 0,         // keys made so far
    kSelProduced = 1,     // candidates seen, lost ones included
    kSelSharedBase = 2,   // where the shared list starts in keys
    kSelShort = 3,        // entries of the short list (may exceed kLevelSmall: the rest was not stored)
    kSelCutBin = 4,       // int: lowest bin the short list takes
    kSelStats = 8,        // two doubles: mean, sd of the gathered scores
    kSelCtrWords = 16
};
struct SelectLds {
    u64* keys;
    u64* small;
    u64* wlists;
    u32* hist;
    u32* ctr;

    static constexpr int bytes(int nkeys) {
        return nkeys * 8 + kLevelSmall * 8 + (kLevelThreads / 64) * kMaxK * 8 + kLevelBins * 4 + kSelCtrWords * 4;
    }
    static __device__ __forceinline__ SelectLds carve(unsigned char* smem, int nkeys) {
        SelectLds l;
        l.keys = (u64*)smem;
        l.small = l.keys + nkeys;
        l.wlists = l.small + kLevelSmall;
        l.hist = (u32*)(l.wlists + (kLevelThreads / 64) * kMaxK);
        l.ctr = l.hist + kLevelBins;
        return l;
    }
};

// Stage 1 of lds_select_top: mean and standard deviation (the population's, fp64) of the scores of keys[0 .. cnt), left in
// the two kSelStats doubles for every thread to read.  The per-wave sums pass through wlists, which is free until the
// streaming path.  (lane, wave and the wave count come from the caller: computed again in a stage, the kernels re-load
// blockDim behind every barrier.)
__device__ __forceinline__ void select_stats(SelectLds l, int cnt, int lane, int wave, int nw) {
    double* red = (double*)&l.ctr[kSelStats];
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        const double v = (double)key_score(l.keys[i]);
        s1 += v;
        s2 += v * v;
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    double* part = (double*)l.wlists;
    if (lane == 0) {
        part[2 * wave] = s1;
        part[2 * wave + 1] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < nw; ++w) {
            t1 += part[2 * w];
            t2 += part[2 * w + 1];
        }
        const double m = t1 / cnt;
        red[0] = m;
        red[1] = sqrt(fmax(t2 / cnt - m * m, 0.0));
    }
    __syncthreads();
}

// Stage 4 of lds_select_top, where the short list overflowed (many equal scores in the cut bin: duplicates, saturated
// scores, sd = 0), the streaming fallback over ALL gathered keys: every wave runs its slice through a running top-kl
// (WaveTopK; KR = key registers per lane, 1: kl <= 64, 4: kl <= 256), the lists are merged by one sort in wlists.
template <int KR>
__device__ __forceinline__ u64* select_stream(SelectLds l, int cnt, int kl, int lane, int wave, int nw) {
    WaveTopK<KR> tk;
    tk.init();
    for (int i0 = wave * 64; i0 < cnt; i0 += nw * 64) {
        const int i = i0 + lane;
        tk.offer((i < cnt) ? l.keys[i] : 0ull, kl, lane);
    }
    int P = 2;
    while (P < nw * kl) P <<= 1;
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += blockDim.x) l.wlists[i] = 0ull;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int s = r * 64 + lane;
        if (s < kl) l.wlists[wave * kl + s] = tk.key[r];
    }
    bitonic_sort_desc(l.wlists, P, threadIdx.x, blockDim.x);
    return l.wlists;
}

// The kl best of the `cnt` keys in l.keys, sorted descending; returns the sorted list (at least kl entries, 0 = empty).
// Shared by level_select_kernel, select_hist_kernel and sample_select_biased_kernel.  On entry the histogram is zeroed and
// kSelShort is 0: each caller does that together with its own counters, in front of the barrier behind which it makes the
// keys (one shared function for it moves level_select_kernel and sample_select_biased_kernel - profiles/HISTORY.md).  `want_stats_in`: the caller needs mean / sd of the scores even where the selection
// does not (at most kLevelSmall keys); otherwise they come back 0.
//
// The body is its stages: statistics (select_stats), the short list (all keys, or the histogram cut), the short sort, or
// the streaming fallback (select_stream) where the short list overflowed.  Two ways, chosen by the data:
//   * short path (the usual one): at most kLevelSmall keys -> one bitonic sort of them; more keys -> a 1024-bin histogram
//     of the scores over [mean - 4 sd, mean + 8 sd] (LDS atomics), a scan of the bins from the top down to the bin that
//     holds the kl-th best key, and the sort of just the keys in the bins above it (plus that bin);
//   * streaming path (more than kLevelSmall keys in the cut bin: piles of equal scores, sd = 0): every wave runs its
//     slice through a running top-kl and the eight lists are merged by one sort.
// The rule tests/test_final_select_gpu.py and tests/test_select_rounds_gpu.py hold this to: every path - direct sort,
// histogram cut, streaming (and, in kernels_level.h, the one-wave form in front of it) - returns the same keys in the
// same order, the kl largest in descending order; which one ran shows in timing only.
template <int KR>
__device__ __forceinline__ u64* lds_select_top(SelectLds l, int cnt, int kl, bool want_stats_in, double& mean, double& sd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;   // once, for every stage
    u32& nshort = l.ctr[kSelShort];
    int& cut_bin = *(int*)&l.ctr[kSelCutBin];
    const bool want_stats = cnt > kLevelSmall || want_stats_in;
    mean = 0.0;
    sd = 0.0;
    if (want_stats) {
        select_stats(l, cnt, lane, wave, nw);
        const double* stats = (const double*)&l.ctr[kSelStats];
        mean = stats[0];
        sd = stats[1];
    }

    // Stage 2, the short list: every key where there are at most kLevelSmall; otherwise the histogram cut - bins of
    // (12 / 1024) sd over [mean - 4 sd, mean + 8 sd], bin 1023 = everything above; the bin scan; the keys of the cut bin and
    // of the bins above it.  nshort counts them all, also those the list has no room for.  (Inline: as a function of its
    // own it moves the unrolled bin scan of every kernel that calls lds_select_top - profiles/HISTORY.md.)
    if (cnt <= kLevelSmall) {
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) l.small[i] = l.keys[i];
        if (threadIdx.x == 0) nshort = (u32)cnt;
    } else {
        const float lo = (float)(mean - 4.0 * sd);
        const float inv = (sd > 0.0) ? (float)((double)kLevelBins / (12.0 * sd)) : 0.0f;
        auto bin_of = [&](u64 key) -> int {
            const float t = (key_score(key) - lo) * inv;
            return (t >= (float)(kLevelBins - 1)) ? kLevelBins - 1 : (t > 0.0f ? (int)t : 0);
        };
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) atomicAdd(&l.hist[bin_of(l.keys[i])], 1u);
        __syncthreads();
        if (wave == 0) {
            // one wave scans the bins from the top: lane l owns bins [1023 - 16 l - 15, 1023 - 16 l]
            u32 mine = 0;
            for (int j = 0; j < 16; ++j) mine += l.hist[kLevelBins - 1 - 16 * lane - j];
            u32 incl = mine;
            for (int off = 1; off < 64; off <<= 1) {
                const u32 up = __shfl_up((int)incl, off, 64);
                if (lane >= off) incl += up;
            }
            const u64 reach = __ballot(incl >= (u32)kl);
            if (reach) {
                const int L = __ffsll((long long)reach) - 1;          // first lane group that reaches kl
                u32 run = (u32)__shfl((int)(incl - mine), L, 64);
                if (lane == L) {
                    int j = 0;
                    for (; j < 16; ++j) {
                        run += l.hist[kLevelBins - 1 - 16 * L - j];
                        if (run >= (u32)kl) break;
                    }
                    cut_bin = kLevelBins - 1 - 16 * L - min(j, 15);
                }
            } else if (lane == 0) {
                cut_bin = 0;
            }
        }
        __syncthreads();
        const int cb = cut_bin;
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
            const u64 key = l.keys[i];
            if (bin_of(key) >= cb) {
                const u32 at = atomicAdd(&nshort, 1u);
                if (at < (u32)kLevelSmall) l.small[at] = key;
            }
        }
    }
    __syncthreads();
    const u32 nsm = nshort;
    u64* best = l.small;
    if (nsm <= (u32)kLevelSmall) {
        // Stage 3, the short sort: the list padded with empty keys to a power of two that holds kl, one bitonic sort.
        // (Inline: as a function it turns a signed compare of every caller into an unsigned one - profiles/HISTORY.md.)
        int P = 2;
        while (P < (int)nsm) P <<= 1;
        if (P < kl) {
            P = 2;
            while (P < kl) P <<= 1;
        }
        for (int i = (int)nsm + threadIdx.x; i < P; i += blockDim.x) l.small[i] = 0ull;
        bitonic_sort_desc(l.small, P, threadIdx.x, blockDim.x);
    } else {
        best = select_stream<KR>(l, cnt, kl, lane, wave, nw);
    }
    return best;
}

// Descending bitonic sort of 64 R values held by ONE wave, element e = 64 r + lane in v[r]: exchanges between lanes are
// shuffles, exchanges at distances of 64 and more stay inside the lane - no LDS, no barrier.  What the two short selects
// of kernels_level.h run on: the kernels that bracket the full pass are latency, and a workgroup-wide sort of a hundred
// keys is 28 barriers of it.
template <typename T> __device__ __forceinline__ T wave_xor(T v, int mask);
template <> __device__ __forceinline__ u32 wave_xor<u32>(u32 v, int mask) { return (u32)__shfl_xor((int)v, mask, 64); }
template <> __device__ __forceinline__ u64 wave_xor<u64>(u64 v, int mask) {
    const u32 lo = (u32)__shfl_xor((int)(u32)v, mask, 64), hi = (u32)__shfl_xor((int)(u32)(v >> 32), mask, 64);
    return ((u64)hi << 32) | lo;
}
template <typename T, int R>
__device__ __forceinline__ void wave_sort_desc(T (&v)[R], int lane) {
#pragma unroll
    for (int size = 2; size <= 64 * R; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride >= 64) {
                const int rs = stride >> 6;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (r & rs) continue;
                    const bool desc = (((r << 6) & size) == 0);      // bit `size` of the element index lies in r here
                    const T a = v[r], b = v[r | rs];
                    const bool swap = (a < b) == desc;
                    v[r] = swap ? b : a;
                    v[r | rs] = swap ? a : b;
                }
            } else {
                const bool low = (lane & stride) == 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const bool desc = ((((r << 6) | lane) & size) == 0);
                    const T mine = v[r], other = wave_xor<T>(mine, stride);
                    const T hi = mine > other ? mine : other, lo = mine > other ? other : mine;
                    v[r] = (low == desc) ? hi : lo;
                }
            }
        }
    }
}

// Result slot i of query qid from a key: (score, global id), (-inf, -1) for the empty key.  The id is id_map[row] where the
// index has a map (subset indexes), row + row_offset otherwise.  Everything by value: taken by reference, or from the
// argument struct, it moves the instructions of every select kernel.
__device__ __forceinline__ void write_result_slot(float* out_scores, int64_t* out_idx, int k_user, const int64_t* id_map,
                                                  int64_t row_offset, int qid, int i, u64 key) {
    out_scores[(int64_t)qid * k_user + i] = key ? key_score(key) : -INFINITY;
    out_idx[(int64_t)qid * k_user + i] = !key ? -1 : id_map ? id_map[key_row(key)] : (int64_t)key_row(key) + row_offset;
}

struct SelectArgs {
    const u64* in;       // [slot][in_stride] keys (any order; 0 = empty)
    int64_t in_stride;
    int m;               // keys per slot
    int kout;            // keys written per segment
    u64* out;            // intermediate: [slot][out_stride], segment s writes at s * kout
    int64_t out_stride;
    float* out_scores;   // final round (one segment): [query][k_user]
    int64_t* out_idx;
    int k_user;
    int64_t row_offset;
    const int64_t* id_map;  // optional: local row -> global id (subset indexes); replaces row + row_offset
    const int* qlist;    // optional slot -> query id
    const int* qcount;   // optional device-side slot count
};

// One select round of the scan path: exact top-k of a key list, one workgroup per list segment (bitonic sort in LDS).
// grid = (segments, slots); 256 threads; SEG keys of LDS.
template <int SEG>
__global__ void __launch_bounds__(256) select_kernel(SelectArgs a) {
    __shared__ u64 keys[SEG];
    const int slot = blockIdx.y;
    if (a.qcount && slot >= *a.qcount) return;
    const int seg = blockIdx.x;
    const int begin = seg * SEG;
    const int cnt = min(SEG, a.m - begin);
    int P = 1;
    while (P < cnt) P <<= 1;
    if (P < 2) P = 2;
    const u64* src = a.in + (int64_t)slot * a.in_stride + begin;
    for (int i = threadIdx.x; i < P; i += blockDim.x) keys[i] = (i < cnt) ? src[i] : 0ull;
    bitonic_sort_desc(keys, P, threadIdx.x, blockDim.x);
    if (a.out_scores) {
        const int qid = a.qlist ? a.qlist[slot] : slot;
        for (int i = threadIdx.x; i < a.k_user; i += blockDim.x)
            write_result_slot(a.out_scores, a.out_idx, a.k_user, a.id_map, a.row_offset, qid, i, (i < P) ? keys[i] : 0ull);
    } else {
        u64* dst = a.out + (int64_t)slot * a.out_stride + (int64_t)seg * a.kout;
        for (int i = threadIdx.x; i < a.kout; i += blockDim.x) dst[i] = (i < P) ? keys[i] : 0ull;
    }
}

// One-launch reduction of the scan's partial lists (up to kHistSelectMax keys per query: 1024 workgroups x k <= 12) to the
// final k: the keys are loaded into LDS (empty slots squeezed out by ballot), then lds_select_top's histogram cut + short
// sort.  Replaces two select_kernel rounds (10 bitonic sorts of 1024 keys + a final one: 22 + 7 us and a kernel boundary)
// by ~10 us: what the single-query searches of the apps wait for (streamlit_app.py:282-283, app_showcase_model.py:93-96).
constexpr int kHistSelectMax = 12288;   // 96 KiB of keys: with the short list, the per-wave lists and the histogram 132 KiB of LDS
constexpr int kHistSelectLds = SelectLds::bytes(kHistSelectMax);
static_assert(kHistSelectLds <= 160 * 1024, "select kernels must fit the CU's LDS");

template <int KR>   // key registers per lane of the streaming path - 1: k <= 64, 4: k <= 256
__global__ void __launch_bounds__(kLevelThreads) select_hist_kernel(SelectArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SelectLds lds = SelectLds::carve(smem, kHistSelectMax);
    const int slot = blockIdx.x;
    if (a.qcount && slot >= *a.qcount) return;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) {
        lds.ctr[kSelFill] = 0;
        lds.ctr[kSelShort] = 0;
    }
    for (int i = threadIdx.x; i < kLevelBins; i += blockDim.x) lds.hist[i] = 0;
    __syncthreads();
    const u64* src = a.in + (int64_t)slot * a.in_stride;
    const int m = min(a.m, kHistSelectMax);
    for (int i0 = (threadIdx.x & ~63); i0 < m; i0 += blockDim.x) {
        const int i = i0 + lane;
        const u64 key = (i < m) ? src[i] : 0ull;
        const u64 live = __ballot(key != 0ull);
        u32 base = 0;
        if (lane == 0 && live) base = atomicAdd(&lds.ctr[kSelFill], (u32)__popcll(live));
        base = (u32)__shfl((int)base, 0, 64);
        if (key != 0ull) lds.keys[base + __popcll(live & ((1ull << lane) - 1ull))] = key;
    }
    __syncthreads();
    const int cnt = (int)lds.ctr[kSelFill];
    double mean, sd;
    u64* best = lds_select_top<KR>(lds, cnt, a.k_user, false, mean, sd);
    const int qid = a.qlist ? a.qlist[slot] : slot;
    for (int i = threadIdx.x; i < a.k_user; i += blockDim.x)
        write_result_slot(a.out_scores, a.out_idx, a.k_user, a.id_map, a.row_offset, qid, i, best[i]);
}

}  // namespace ts
