// The streaming scan path's host decisions (search.hip) as pure functions of plain values: which kernel form serves a row
// width, the shape of a scan pass, the select rounds that reduce its partial lists and the scratch they write, scan or
// matrix path, the allowed rows of a host mask, the host key of ts_count_above.  No handle, no HIP call, nothing from HIP:
// the C ABI's codes (include/tsearch.h, plain C) and the standard library only, so tests/scan_plan_check.cpp runs all of
// it on the CPU under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/tsearch.h"

namespace ts {

constexpr int kQBlock = 256;          // queries per pass of the search driver = slots of the scan's partial lists
constexpr int kScanGridPerCU = 4;
constexpr int kSelectHistKeys = 12288;   // keys per slot one histogram select takes (kernels_select.h: kHistSelectMax)

// ---------------------------------------------------------------------------------------------
// the width table: scan_kernel / rank_kernel <DT, CH, G> of a (storage type, row width); every other width runs the
// generic kernels (queries staged in LDS).  G lanes read one row, CH chunks of 16 bytes each: CH * G * 16 bytes = one row.
// ---------------------------------------------------------------------------------------------
struct ScanWidth { int dtype; int ld; int ch; int g; };
constexpr int kScanWidths = 8;
constexpr ScanWidth kScanWidth[kScanWidths] = {
    {TS_F32, 768, 3, 64}, {TS_F32, 1024, 4, 64}, {TS_BF16, 768, 3, 32}, {TS_BF16, 1024, 2, 64},
    // the other common embedding widths (MiniLM-class 384, 512): same kernel, narrower lane groups
    {TS_F32, 384, 3, 32}, {TS_BF16, 384, 3, 16}, {TS_F32, 512, 2, 64}, {TS_BF16, 512, 2, 32}};

// index into kScanWidth, or -1 = generic
inline int scan_width(int dtype, int64_t ld) {
    for (int i = 0; i < kScanWidths; ++i)
        if (kScanWidth[i].dtype == dtype && kScanWidth[i].ld == ld) return i;
    return -1;
}

// the generic kernels: 4 queries per pass while they fit the LDS (ld <= 8192) and one list of keys per lane does
// (k <= 64, or no list at all: EMIT); 8 KiB of LDS for the lists + one fp32 copy of each query
inline int scan_generic_qb(int qb_pref, int64_t ld, int kr, bool emit) {
    return (qb_pref == 4 && ld <= 8192 && (emit || kr == 1)) ? 4 : 1;
}
inline int scan_generic_lds(int64_t ld, int qb) { return 8192 + (int)ld * 4 * qb; }
inline int rank_generic_lds(int64_t ld) { return (int)ld * 4; }

// ---------------------------------------------------------------------------------------------
// the pass shape of scan_search
// ---------------------------------------------------------------------------------------------
struct ScanPass {
    int grid;   // workgroups: each hands k keys per query to the select
    int kr;     // keys per lane and query: 1 (k <= 64) or 4
    int qb;     // queries per pass: 4 or 1
};

inline int scan_kr(int k) { return k <= 64 ? 1 : 4; }

// Large k over a small corpus (app_showcase_model.py:96: topk(200) over a few thousand theorems): every workgroup hands k
// keys to the select, and 1,024 x 200 of them cost three rounds of sorts (150 us) for a scan of 10 us.  Few enough
// workgroups that ONE histogram select takes all their keys.
inline int scan_grid(int cu_count, int64_t n, int k) {
    const int grid = cu_count * kScanGridPerCU;
    if (k > 64 && n <= 16384) return std::min(grid, std::max(8, kSelectHistKeys / k));
    return grid;
}

// one_launch: the matrix path's exact re-run (device-side query count), whose last workgroup reduces the lists itself
inline ScanPass scan_pass(int cu_count, int64_t n, int dtype, int64_t ld, int nq, int k, bool one_launch) {
    ScanPass p;
    p.grid = scan_grid(cu_count, n, k);
    // an almost always empty launch: one workgroup per CU dispatches (and drains) faster than four; when it does run, a
    // pass at a lower share of the HBM rate is the price of the rare query the estimate failed for
    if (one_launch) p.grid = std::min(p.grid, cu_count);
    p.kr = scan_kr(k);
    // k > 64 keeps 4 keys per lane and query: on bf16 x 768 four queries at once need all 256 VGPRs, one wave per SIMD
    // (measured 0.18 of the HBM rate against 0.8 for one query per pass); the other shapes keep two waves
    const bool wide_k_one_wave = k > 64 && dtype == TS_BF16 && (ld == 768 || ld == 384);
    p.qb = ((nq >= 2 || one_launch) && !wide_k_one_wave) ? 4 : 1;
    return p;
}

// ---------------------------------------------------------------------------------------------
// the select plan: [slots][m] partial keys -> the k best per slot
// ---------------------------------------------------------------------------------------------
enum SelectFinal { kSelectHist, kSelectSort1024, kSelectSort4096 };
struct SelectRound { int seg, nseg, out; };   // nseg sorts of seg keys, k kept of each: out = nseg * k keys per slot
// a round keeps at most a quarter of its keys + 256 (a sixteenth while m > 65,536): 5 rounds reduce any int m at k <= TS_MAX_K
constexpr int kSelectMaxRounds = 8;
struct SelectPlan {
    int nrounds;                // intermediate rounds; -1 = no plan (k > TS_MAX_K)
    SelectRound round[kSelectMaxRounds];
    int final_m;                // keys per slot the final launch reads
    SelectFinal final_form;
    int hist_kr;                // kSelectHist: keys per lane of the per-wave lists, 1 (k <= 64) or 4
};

inline SelectPlan select_plan(int m, int k) {
    SelectPlan p;
    memset(&p, 0, sizeof(p));
    for (;;) {
        p.final_m = m;
        if (m > 1024 && m <= kSelectHistKeys) {
            // the usual case (k <= 12 over 1024 workgroups, or k up to 256 over the fewer workgroups scan_grid gives a
            // small corpus): one launch, histogram cut instead of rounds of bitonic sorts
            p.final_form = kSelectHist;
            p.hist_kr = scan_kr(k);
            return p;
        }
        if (m <= 1024 || (k > 64 && m <= 4096)) {
            p.final_form = m <= 1024 ? kSelectSort1024 : kSelectSort4096;
            return p;
        }
        if (p.nrounds == kSelectMaxRounds || k > TS_MAX_K) {
            p.nrounds = -1;
            return p;
        }
        // intermediate round: many small sorts in parallel beat a few big ones (a 4096-key bitonic sort by one
        // workgroup costs ~80 us, a 1024-key one ~15 us)
        SelectRound& r = p.round[p.nrounds++];
        r.seg = (m > 65536) ? 4096 : 1024;
        r.nseg = (m + r.seg - 1) / r.seg;
        r.out = r.nseg * k;
        m = r.out;
    }
}

// The rounds ping-pong: the scan writes `partial`, round 0 `partial2`, round 1 `partial` again, ...  Keys per slot of the
// largest output that lands in each.
struct SelectScratch { int64_t partial, partial2; };
inline SelectScratch select_scratch(const SelectPlan& p) {
    SelectScratch s = {0, 0};
    for (int r = 0; r < p.nrounds; ++r) {
        int64_t& into = (r & 1) ? s.partial : s.partial2;
        into = std::max<int64_t>(into, p.round[r].out);
    }
    return s;
}

// Keys of the two buffers for kQBlock slots of a scan at this k, at the full grid and at the small-corpus one.  `partial2`
// keeps the size it always had (an eighth of `partial` + 4,096 keys) wherever that holds its rounds' outputs - every k
// at 128 CUs and more; a partition of fewer CUs takes 1,024-key segments at large k, whose outputs it did not hold.
struct ScanScratch { size_t partial, partial2; };
inline ScanScratch scan_scratch(int cu_count, int k) {
    const size_t full = (size_t)cu_count * kScanGridPerCU * (size_t)k;
    ScanScratch s = {(size_t)kQBlock * full, (size_t)kQBlock / 8 * full + 4096};
    for (const int64_t n : {(int64_t)16384, (int64_t)16385}) {      // the small-corpus grid, the full grid
        const SelectScratch need = select_scratch(select_plan(scan_grid(cu_count, n, k) * k, k));
        s.partial = std::max(s.partial, (size_t)kQBlock * (size_t)need.partial);
        s.partial2 = std::max(s.partial2, (size_t)kQBlock * (size_t)need.partial2);
    }
    return s;
}

// ---------------------------------------------------------------------------------------------
// scan or matrix path
// ---------------------------------------------------------------------------------------------
// Largest batch the streaming scan still serves faster than the MFMA path: one scan pass serves 4 queries at the HBM
// rate, and one launch of the matrix kernels (64 queries or more) costs less than two scan passes on both storage types
// (1M x 768 fp32, 5-8 queries: 0.99 ms through the scan, 0.74 ms through the 16x16x4 kernel; 10M x 768 bf16: 4.44 against
// 2.21 ms).  Large k (4 keys per lane in the scan) moves it down to 1.
inline int scan_max_queries(int k, int knob) { return k > 64 ? 1 : knob; }

struct AlgoInputs {
    int algo;                   // requested: TS_ALGO_AUTO / SCAN / MFMA
    bool mfma_ok;               // the matrix kernels serve this index
    int64_t n;
    int nq, k;
    int mfma_min_rows;          // TS_MFMA_MIN_ROWS
    int scan_max_queries;       // TS_SCAN_MAX_QUERIES
    bool bias, subset;          // a biased search; a subset index
    bool mask, mask_on_device;
    int64_t allowed;            // rows the mask allows: a host mask's (count_allowed_rows), read only where mask_wants_count(),
                                //   or a device mask's where allowed_known
    bool allowed_known;         // a device mask that comes with its count (a row set, meta_plan.h); false: every decision as before
};
struct AlgoChoice {
    int algo;                   // TS_ALGO_SCAN or TS_ALGO_MFMA
    const char* unsupported;    // not NULL: TS_ERR_UNSUPPORTED with this text
};

inline bool mfma_batch(const AlgoInputs& in) {
    return in.mfma_ok && in.n >= in.mfma_min_rows && in.nq > scan_max_queries(in.k, in.scan_max_queries);
}
// a host mask in front of a batch the matrix path would take: its density decides, so its bits are counted
inline bool mask_wants_count(const AlgoInputs& in) {
    return in.mask && !in.mask_on_device && !in.bias && in.algo != TS_ALGO_SCAN && mfma_batch(in);
}
// ... or a device mask whose count came with it (a row set): the same batches, nothing to count
inline bool mask_count_decides(const AlgoInputs& in) {
    return mask_wants_count(in) ||
           (in.mask && in.mask_on_device && in.allowed_known && !in.bias && in.algo != TS_ALGO_SCAN && mfma_batch(in));
}

inline AlgoChoice choose_algo(const AlgoInputs& in) {
    int algo = in.algo;
    if (in.bias) {
        // ts_search_biased: the additive term is applied where the row is known and the key is made, in the scan kernel
        // (four queries per pass at the HBM rate).  A threshold that prunes exists - not the Gaussian estimate of the
        // weighted scores (a per-row term of the size of w * ln(citations), several standard deviations of the scores, is
        // not Gaussian), but one that models the similarities and the known term apart: ts_search_biased_ex runs the
        // general-width matrix pass behind it and decides with choose_bias_algo (bias_plan.h), not here.
        if (in.subset) return {0, "biased search on a subset index"};
        if (algo == TS_ALGO_MFMA) return {0, "the biased search runs on the scan kernel"};
        algo = TS_ALGO_SCAN;
    }
    if (in.mask) {
        // Batches behind a host mask that keeps at least a tenth of the rows run the MFMA path: the bit is tested in its
        // append path and the threshold estimates are made for the allowed rows (the sample sees only those).  Sparser
        // masks leave the sample too few allowed rows to estimate from; device masks would need a count + sync first:
        // both go through the scan kernel, 4 queries per pass (or through a subset index).  A device mask that comes with
        // its count (allowed_known: a row set) is decided as a counted host mask is.
        const bool dense_host_mask = mask_count_decides(in) && in.allowed * 10 >= in.n;
        if (algo == TS_ALGO_MFMA && !dense_host_mask)
            return {0, "the MFMA path serves host masks that keep at least a tenth of the rows, for more than 4 queries"};
        algo = dense_host_mask ? TS_ALGO_MFMA : TS_ALGO_SCAN;
    }
    // The scan serves 4 queries per pass at the HBM rate; the MFMA path serves up to 256 per pass but its pass is
    // ~1.7x longer (matrix + HBM load drops the clock): a handful of queries is faster through the scan.
    if (algo == TS_ALGO_AUTO) algo = mfma_batch(in) ? TS_ALGO_MFMA : TS_ALGO_SCAN;
    return {algo, nullptr};
}

// rows a bitmask of (n + 31) / 32 words allows: its set bits, without the bits past the last row
inline int64_t count_allowed_rows(const uint32_t* mask, int64_t n) {
    const int64_t words = (n + 31) / 32;
    int64_t allowed = 0;
    for (int64_t w = 0; w < words; ++w) allowed += __builtin_popcount(mask[w]);
    const int tail_bits = (int)(words * 32 - n);
    if (tail_bits > 0) allowed -= __builtin_popcount(mask[words - 1] >> (32 - tail_bits));
    return allowed;
}

// ---------------------------------------------------------------------------------------------
// host keys
// ---------------------------------------------------------------------------------------------
// host twin of ord_f32 (common.h): the score half of a key
inline uint32_t host_ord_f32(float s) {
    s = s + 0.0f;
    uint32_t u;
    memcpy(&u, &s, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ts_count_above: key of (score, document) in the key space of a shard of n rows, `row` = the document's global id minus
// the shard's row offset.  A document before the shard loses every tie (low word all ones), one behind it wins every tie
// (low word zero).  NaN: all ones, nothing counts.
inline uint64_t count_above_key(float score, int64_t row, int64_t n) {
    if (!(score == score)) return ~0ull;
    const uint64_t low = row < 0 ? 0xFFFFFFFFull : (row >= n ? 0ull : (uint64_t)(0xFFFFFFFFu - (uint32_t)row));
    return ((uint64_t)host_ord_f32(score) << 32) | low;
}

}  // namespace ts
