// The matrix path's threshold and final select: level_threshold (the pass threshold from a sample's best scores),
// level_select_kernel (the candidate lists of a level -> its threshold, or the k results) and sample_select_fast_kernel
// (the dense sample matrix -> the thresholds).
//
// Rules that tests/threshold_common.py (a numpy model of level_threshold and of the plan in search_mfma.hip) and
// tests/test_final_select_gpu.py hold this file to - on lattice corpora, where every score is exact, the candidate count
// of a search pins each of them:
//   * a threshold is max(k-th best of the live sample scores (-inf below k of them), float(mean + z_tail sd) from 256
//     live scores on, the tail fit from 1,024 on); mean and sd are the population's, in fp64, over LIVE scores only - a
//     masked row, a NaN row and a position past the sample carry none.  sd = 0 makes the estimate the score itself.
//   * the tail fit extrapolates only beyond the sample's 32nd best: ratio = (32 / cnt) / tail_p > 1, that is more than
//     64 allowed rows per live sample row - a sample stride above 64, from 262,145 rows on with the default 4,096-row
//     sample.  Armed below that (k n / sample > 4096) it never moves a threshold.
//   * the final level's count is every row at or above the threshold, kept or lost: above cap (8192) or below
//     min(k, allowed rows) the query re-runs exactly.  NaN rows are never candidates, so k above the number of rows WITH
//     a score re-runs by design: the select cannot tell "three rows have no score" from "the threshold lost three rows".
//   * the one-wave form of the final select (<= kFinalFast candidates, k <= kFinalFast, shared list only) returns the
//     same keys in the same order as every path of lds_select_top (kernels_select.h).
#pragma once
#include "kernels_select.h"

namespace ts {

// MFMA path, after each threshold level: one workgroup per query gathers that query's candidates
// (the writers' private lists plus the shared spill list), sorts them, and
//   sample level: sets thr[q] = score of the kk-th best candidate (-inf if fewer);
//   final level : writes the k results, or appends q to the fall-back list when candidates were
//                 lost (shared list overflow, or more candidates than the sort buffer holds).
struct LevelArgs {
    const u64* priv;     // [nq][nwriters][priv_cap]
    const u32* pcount;   // [nq][nwriters] entries produced per writer (> priv_cap: the rest spilled)
    int nwriters;
    int priv_cap;
    const u64* cand;     // [nq][cap] shared spill lists
    u32* count;          // [nq] appended to the shared list (may exceed cap); reset here
    int cap;
    int kk;              // threshold rank, >= k_user
    float* thr;          // [256]
    int final_level;
    float z_tail;        // sample level: > 0 = also apply the Gaussian-tail estimate mean + z * std of the sample
    float tail_p;        // sample level: > 0 = also apply the exponential-tail fit for this exceedance probability
    float tail_z;        // standard-normal quantile of the sample's 32nd best (z with P(X > z) = 32 / sample rows)
    int min_fill;        // final level: fewer candidates than this = the estimate was too high: exact re-run
    float* out_scores;
    int64_t* out_idx;
    int k_user;
    int64_t row_offset;
    const int64_t* id_map;
    int* fb_list;
    int* fb_count;
    u32* stat_q;         // [nq] candidates seen at the final level (the host adds them up when statistics are asked for:
                         // one atomic per query on ONE counter was 256 serialised L2 operations at the end of every search)
    int nq;
};

constexpr int kLevelLds = SelectLds::bytes(kLevelSortMax);
static_assert(kLevelLds <= 160 * 1024, "select kernels must fit the CU's LDS");

// Pass threshold of the next level from the kl best keys of a sample (`best`, sorted descending; cnt keys were sampled;
// mean / sd of all sampled scores).  Shared by level_select_kernel (candidate lists of a sample level) and
// sample_select_fast_kernel (the dense sample matrix).
__device__ __forceinline__ float level_threshold(const LevelArgs& a, const u64* best, int cnt, int kk, bool tail_fit, double mean,
                                                 double sd) {
    constexpr int kTailM = 32;
    // the kk-th best of a sample is a lower bound of the final kk-th best: a guaranteed threshold (any subset
    // of the candidates still gives a valid bound, so lost candidates are harmless here)
    const u64 kth = best[kk - 1];
    float thr = kth ? key_score(kth) : -INFINITY;
    // Heavier-than-Gaussian tails (clusters of near-duplicates: real corpora) make the Gaussian estimate far too
    // low and the full pass would drown in candidates.  Second estimate, from the sample's order statistics 8..32
    // (the top 7 are left out: outliers must not set the slope): an exponential tail fitted to their spacings
    // (E[x_j - x_32] = e * sum_{i=j}^{31} 1/i) and extrapolated to the exceedance probability tail_p, which the
    // host sets for ~2048 expected candidates - a quarter of the buffer, far above k - and only for corpora so large
    // that the guaranteed bound alone would swamp the buffer.  It is used only where the sample SHOWS a heavy tail:
    // its 32nd best lies more than half a standard deviation above where a Gaussian with the sample's mean and
    // variance puts it.  On Gaussian-like scores the fit is therefore never consulted - extrapolated over
    // ln(N / sample) it is noisier than the Gaussian estimate, and at 50M rows its overshoots sent one query per
    // batch to the exact re-run (an 11 ms scan pass per step, measured).  Like the Gaussian estimate it is only an
    // estimate that the final level verifies.
    float thr_tail = -INFINITY, x_m = -INFINITY;
    if (tail_fit && cnt >= 1024 && best[kTailM - 1] != 0ull) {
        x_m = key_score(best[kTailM - 1]);
        float spacing = 0.0f;
        for (int j = 8; j < kTailM; ++j) spacing += key_score(best[j - 1]) - x_m;
        const float e = spacing * (1.0f / 13.95928363f);
        const float ratio = ((float)kTailM / (float)cnt) / a.tail_p;  // how far beyond the sample's 32nd best
        if (ratio > 1.0f && e > 0.0f) thr_tail = x_m + e * __logf(ratio);
    }
    if (a.z_tail > 0.0f && cnt >= 256) {
        // ... and usually far too low for the next level when that level is much bigger.  The scores of one
        // query over the corpus are close to Gaussian (normalised, high-dimensional rows), so the sample's
        // mean + z * std estimates the score that only the wanted number of rows exceed.  NOT a bound: the
        // final level checks that at least min_fill candidates came back and re-runs the query exactly if not.
        thr = fmaxf(thr, (float)(mean + (double)a.z_tail * sd));
        const bool heavy_tail = (double)x_m > mean + ((double)a.tail_z + 0.5) * sd;
        if (heavy_tail) thr = fmaxf(thr, thr_tail);
    }
    return thr;
}

// Sum over the 64 lanes of a wave on the DPP path (row / quad permutes inside the vector pipe, a few cycles each) instead of
// six dependent ds_bpermute round trips through the LDS crossbar: quad xor 1, xor 2, half-row mirror, row mirror leave every
// lane with its row's sum; row_bcast15 / row_bcast31 fold the rows into lane 63; the result is read from there (uniform).
#define TS_DPP(v, ctrl, rmask) ((u32)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), (rmask), 0xf, false))
#define TS_DPP_QUAD_XOR1 0xB1      /* quad_perm [1,0,3,2] */
#define TS_DPP_QUAD_XOR2 0x4E      /* quad_perm [2,3,0,1] */
#define TS_DPP_HALF_MIRROR 0x141
#define TS_DPP_ROW_MIRROR 0x140
#define TS_DPP_BCAST15 0x142
#define TS_DPP_BCAST31 0x143
__device__ __forceinline__ double wave_total_f64(double v) {
#define TS_DPP_F64_STEP(ctrl, rmask)                                                                          \
    {                                                                                                          \
        const u64 b = (u64)__double_as_longlong(v);                                                            \
        const u32 lo = TS_DPP((u32)b, ctrl, rmask), hi = TS_DPP((u32)(b >> 32), ctrl, rmask);                  \
        v += __longlong_as_double((long long)(((u64)hi << 32) | lo));                                          \
    }
    TS_DPP_F64_STEP(TS_DPP_QUAD_XOR1, 0xf)
    TS_DPP_F64_STEP(TS_DPP_QUAD_XOR2, 0xf)
    TS_DPP_F64_STEP(TS_DPP_HALF_MIRROR, 0xf)
    TS_DPP_F64_STEP(TS_DPP_ROW_MIRROR, 0xf)
    TS_DPP_F64_STEP(TS_DPP_BCAST15, 0xa)      // rows 1 and 3 += the row before them (disabled rows add 0.0: old = 0)
    TS_DPP_F64_STEP(TS_DPP_BCAST31, 0xc)      // rows 2 and 3 += rows 0 + 1
#undef TS_DPP_F64_STEP
    const u64 b = (u64)__double_as_longlong(v);
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)b, 63), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(b >> 32), 63);
    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}

constexpr int kFinalFast = 128;     // candidates the one-wave form of the final select takes (2 keys per lane)

// The usual final level behind the 16x16 full pass: a few dozen candidates in the query's shared list and nothing else
// (the threshold estimate aims at 6 k, at least 64).  One wave takes them straight into registers, sorts them there and
// writes the answer (or sends the query to the exact re-run); the other waves leave.  Two dependent round trips (count,
// keys) and no barrier, instead of the gather / histogram / workgroup sort.  Returns whether it took the query (uniform
// over the workgroup: the kernel is done then).
__device__ __forceinline__ bool level_final_one_wave(const LevelArgs& a, int q) {
    if (!(a.final_level && a.nwriters == 0 && a.k_user <= kFinalFast)) return false;
    const u32 raw0 = a.count[q];                           // uniform over the workgroup
    if (!(raw0 <= (u32)kFinalFast && raw0 <= (u32)a.cap)) return false;
    if (threadIdx.x >= 64) return true;
    const int lane = threadIdx.x;
    u64 v[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) v[r] = ((u32)(64 * r + lane) < raw0) ? a.cand[(int64_t)q * a.cap + 64 * r + lane] : 0ull;
    if (lane == 0) {
        a.count[q] = 0;
        a.stat_q[q] = raw0;
    }
    if ((int)raw0 < a.min_fill) {
        if (lane == 0) a.fb_list[atomicAdd(a.fb_count, 1)] = q;
        return true;
    }
    wave_sort_desc<u64, 2>(v, lane);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = 64 * r + lane;
        if (i < a.k_user) {                                // (write_result_slot here moves this kernel's instructions)
            const u64 key = v[r];
            a.out_scores[(int64_t)q * a.k_user + i] = key ? key_score(key) : -INFINITY;
            a.out_idx[(int64_t)q * a.k_user + i] = !key ? -1 : a.id_map ? a.id_map[key_row(key)] : (int64_t)key_row(key) + a.row_offset;
        }
    }
    return true;
}

template <int KR>   // key registers per lane of lds_select_top's streaming path - 1: kk <= 64, 4: kk <= 256
__global__ void __launch_bounds__(kLevelThreads) level_select_kernel(LevelArgs a) {
#include "kernels_level_select.inc"
}

// Sample level of the batched search, dense form (kernels_sample.h): one workgroup per query reads that query's row of the
// sample score matrix (coalesced; -inf = no such row / filtered out, NaN never counted) and sets thr[q] with the estimates
// level_select_kernel applies to a sample level (level_threshold) - without the gather from a thousand lane-private lists.
// Shaped for latency: the threshold needs the SCORES of the kl best sample rows, their mean and their
// standard deviation - not which rows they were.  One workgroup of 256 threads per query holds the whole row of the sample
// matrix in registers (8 x 16-byte loads per thread, all in flight at once), reduces count / sum / sum of squares, cuts at
// mean + z sd (`z_sel`: the host's guess for ~2 kl survivors on Gaussian-like scores), and one wave sorts the survivors in
// registers (wave_sort_desc).  A cut that leaves fewer than kl or more than kSelCap survivors is moved (three tries), then
// found exactly by bisection on the ordered 32-bit scores - piles of equal scores included.
// test_dense_threshold_sample_and_the_list_form_give_the_same_answers holds the answers against the list form's.
constexpr int kSelCap = 1024;        // survivors the sort takes (kl <= 256)

// 256 threads per query (one wave per query measured 20 us against 15: the hundreds of compare / count instructions are
// issue time, and four SIMDs share it).
constexpr int kSelThreads = 256;
template <int THREADS>   // = kSelThreads (a template so that every translation unit may include this header)
__global__ void __launch_bounds__(THREADS) sample_select_fast_kernel(LevelArgs a, const float* scores, int row_stride, float z_sel) {
#include "kernels_sample_select.inc"
}

#undef TS_DPP
#undef TS_DPP_QUAD_XOR1
#undef TS_DPP_QUAD_XOR2
#undef TS_DPP_HALF_MIRROR
#undef TS_DPP_ROW_MIRROR
#undef TS_DPP_BCAST15
#undef TS_DPP_BCAST31

}  // namespace ts
