// Host side shared by the translation units of libtsearch.so (index.hip, search.hip, search_mfma.hip, the launch_*.hip
// files, encoder_ops.hip, shards.hip): error reporting, the launch helpers, the per-handle knobs, the handles themselves,
// stream ordering.
// Internal: nothing here is part of the C ABI (include/tsearch.h); the library is built with hidden visibility.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cctype>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <memory>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/tsearch.h"
#include "common.h"
#include "scan_plan.h"
#include "anyd_plan.h"
#include "bias_plan.h"
#include "rowsets_plan.h"
#include "biased_rowsets_plan.h"
#include "wide_plan.h"
#include "encoder_plan.h"
#include "meta_plan.h"
#include "dev_array.h"

using namespace ts;

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
inline thread_local char g_err[512] = "";

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(e_ == hipErrorOutOfMemory ? TS_ERR_NOMEM : TS_ERR_HIP, "%s failed: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                              \
    } while (0)

// a DevArray call (below): its code is the hipError_t of the allocator
#define DEV_TRY(expr) HIP_TRY((hipError_t)(expr))

#define TS_TRY(expr)            \
    do {                        \
        int rc_ = (expr);       \
        if (rc_ != TS_OK) return rc_; \
    } while (0)

// ---------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------
// One launch of a kernel with `lds` bytes of dynamic LDS: the limit is raised per function AND per device, so the first
// launch of `Kernel` on device `dev` (the CURRENT device: every entry point sets it) raises it, every launch is checked.
// Limit: what the limit is raised to, once - the largest `lds` this kernel is ever launched with; 0 = to `lds` itself, and
// again whenever a launch asks for more than any before it on that device (kernels whose `lds` follows the row width).
template <auto Kernel, int Limit = 0, class... A>
inline int launch_lds(int dev, dim3 grid, dim3 block, int lds, hipStream_t st, const A&... args) {
    static std::atomic<int> raised[64];     // per device: the limit set so far
    static std::mutex raise_mu;
    const int want = Limit ? Limit : lds;
    std::atomic<int>& have = raised[dev & 63];
    if (have.load(std::memory_order_acquire) < want) {
        std::lock_guard<std::mutex> lock(raise_mu);     // two first launches at once: the limit never goes down
        if (have.load(std::memory_order_relaxed) < want) {
            HIP_TRY(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, want));
            have.store(want, std::memory_order_release);
        }
    }
    Kernel<<<grid, block, lds, st>>>(args...);
    HIP_TRY(hipGetLastError());
    return TS_OK;
}

// The kernel form a TS_MFMA_VARIANT names: go(std::integral_constant<int, V>) for the V of Vs... equal to `variant`, its
// result in *rc; false when the list does not name it (the caller then launches the product kernel).
template <int V> using variant_c = std::integral_constant<int, V>;
template <int... Vs, class Go>
inline bool launch_variant(int variant, int* rc, Go&& go) {
    return ((variant == Vs && ((*rc = go(variant_c<Vs>{})), true)) || ...);
}

// A run-time value an entry point has validated, as the template argument it selects: go(variant_c<V>{}) for the V of Vs...
// equal to `v`, its result returned.  Nested for several values (storage type x accesses per lane, tiles x causal x R).
template <int... Vs, class Go>
inline int dispatch_value(int v, Go&& go) {
    int rc = TS_ERR_INVALID;
    if (!launch_variant<Vs...>(v, &rc, go)) return fail(rc, "internal: no kernel for the value %d", v);
    return rc;
}

// Tuning / diagnostic knobs.  Read from the environment ONCE per handle (ts_index_create / ts_index_view /
// ts_index_subset), changed afterwards only through ts_index_set_option: no getenv on the search path.
enum Knob {
    K_MFMA_MIN_RANK, K_MFMA_VARIANT, K_MFMA_GROUPS, K_MFMA_GRID, K_MFMA_STAT, K_MFMA_STAT_CANDS, K_MFMA_TAIL_FIT,
    K_MFMA_NO_IDLE, K_MFMA_AHEAD, K_MFMA_TARGET_CANDS, K_MFMA_FIRST_ROWS, K_MFMA_TARGET_SPARSE, K_MFMA_RUN,
    K_MFMA_MIN_ROWS, K_MFMA_SHAPE, K_MFMA_F32, K_SCAN_GENERIC, K_SCAN_MAX_QUERIES, K_MFMA_BALANCE, K_PROBE_SPREAD, K_MFMA_SAMPLE,
    K_MFMA_PAIR, K_MFMA_PAIR_LAG, K_MFMA_SCREEN, K_MFMA_SCREEN_WIDE, K_MFMA_SCREEN_F32, K_MFMA_SCREEN_LATE, K_MFMA_WIDE_SERIAL, K_COUNT
};
inline const char* const kKnobNames[K_COUNT] = {
    "TS_MFMA_MIN_RANK", "TS_MFMA_VARIANT", "TS_MFMA_GROUPS", "TS_MFMA_GRID", "TS_MFMA_STAT", "TS_MFMA_STAT_CANDS",
    "TS_MFMA_TAIL_FIT", "TS_MFMA_NO_IDLE", "TS_MFMA_AHEAD", "TS_MFMA_TARGET_CANDS", "TS_MFMA_FIRST_ROWS",
    "TS_MFMA_TARGET_SPARSE", "TS_MFMA_RUN", "TS_MFMA_MIN_ROWS", "TS_MFMA_SHAPE", "TS_MFMA_F32", "TS_SCAN_GENERIC",
    "TS_SCAN_MAX_QUERIES", "TS_MFMA_BALANCE", "TS_PROBE_SPREAD", "TS_MFMA_SAMPLE", "TS_MFMA_PAIR", "TS_MFMA_PAIR_LAG",
    "TS_MFMA_SCREEN", "TS_MFMA_SCREEN_WIDE", "TS_MFMA_SCREEN_F32", "TS_MFMA_SCREEN_LATE", "TS_MFMA_WIDE_SERIAL"};
struct Knobs {
    int v[K_COUNT];
    bool set[K_COUNT];
    Knobs() {
        for (int i = 0; i < K_COUNT; ++i) {
            const char* e = getenv(kKnobNames[i]);
            set[i] = e && *e;
            v[i] = set[i] ? atoi(e) : 0;
        }
#ifndef TS_DIAG
        // the timing-only kernel variants and the knobs only the A/B tools ever turned exist in the diagnostic build only
        // (make diag): the product library runs their defaults
        for (int i = 0; i < K_COUNT; ++i)
            if (diag_only((Knob)i)) { set[i] = false; v[i] = 0; }
#endif
    }
    static bool diag_only(Knob k) {
        return k == K_MFMA_VARIANT || k == K_MFMA_MIN_RANK || k == K_MFMA_GROUPS || k == K_MFMA_STAT_CANDS || k == K_MFMA_NO_IDLE ||
               k == K_MFMA_TARGET_CANDS || k == K_MFMA_TARGET_SPARSE || k == K_MFMA_MIN_ROWS || k == K_SCAN_GENERIC ||
               k == K_SCAN_MAX_QUERIES || k == K_PROBE_SPREAD;
    }
    int get(Knob k, int dflt) const { return set[k] ? v[k] : dflt; }
};

// ---------------------------------------------------------------------------------------------
// handles
// ---------------------------------------------------------------------------------------------
constexpr int kCandCap = 8192;        // candidate slots per query (MFMA path); kQBlock, kScanGridPerCU: scan_plan.h
constexpr size_t kStageBytes = (size_t)256 << 20;

// Device memory has one kind of owner, DevArray (dev_array.h) over hipMalloc: a handle's buffers are members of this type and
// a temporary is a local of it, so each is freed once, by its destructor, on every path.  No other code of the library
// allocates, frees or (synchronously) zeroes device scratch.
struct HipMem {
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes ? bytes : 1); }
    static void free(void* p) { (void)hipFree(p); }
    static int zero(void* p, size_t bytes) { return (int)hipMemset(p, 0, bytes); }
};
template <class T> using DevArray = DevArrayOf<T, HipMem>;
using DevBuf = DevArray<void>;        // a temporary, freed on every return path

// The stream and the events of an index handle.  A base of ts_index, so destroyed after every member of it: the buffers
// are freed first, then the events and the stream go.
struct IndexQueue {
    hipStream_t stream = nullptr;
    hipEvent_t order_ev = nullptr;                           // recorded at the end of every call on that call's stream: orders the
    bool ordered = false;                                    //   next call behind it (`ordered`: recorded at least once)
    std::vector<hipEvent_t> ev_pool;                         // ts_index_profile_*: pairs, [2i] start, [2i+1] stop
    IndexQueue() = default;
    IndexQueue(const IndexQueue&) = delete;
    IndexQueue& operator=(const IndexQueue&) = delete;
    ~IndexQueue() {
        for (hipEvent_t e : ev_pool) hipEventDestroy(e);
        if (order_ev) hipEventDestroy(order_ev);
        if (stream) hipStreamDestroy(stream);
    }
};

// ts_search_rowsets: the block of pass queries in progress (under the handle's `mu`).  mfma_search reads the sets, makes the
// block's table from them and adds what the block's final select and re-run counted.
struct RowsetsCall {
    const ts_rowset* const* sets = nullptr;
    const int32_t* which = nullptr;      // [nq of the block]: the set of each query of the block, -1 = every row
    int fallback_queries = 0;            // summed over the blocks so far
    int64_t candidates = 0;
    // ts_search_biased_rowsets (with ix->active_bias, active_bias_matrix): a weight per query; NULL for ts_search_rowsets
    const float* weights = nullptr;      // [nq of the block]
    const int32_t* hist_of = nullptr;    // [nq of the block]: which of the call's histograms of the raw bias is the query's set's
    int nhists = 0;                      // histograms in ix->bias_sets_hist
};

struct ts_index : IndexQueue {
    int device = 0;
    int64_t n = 0, n_pad = 0, ld = 0, row_offset = 0;
    int d = 0, dtype = 0, metric = 0;
    int cu_count = 256;
    DevArray<void> rows;                                     // owned, or borrowed: a view's (`borrowed`), the caller's (`attached`)
    std::mutex mu;
    // scratch (lazily sized)
    DevArray<void> stage;                                    // host->device staging
    DevArray<void> qstore;      DevArray<float> qf32;        // prepared queries [256 x ld]
    DevArray<u64> cand;         DevArray<u32> count;         DevArray<float> thr;
    DevArray<u64> priv;         DevArray<u32> pcount;        int priv_writers = 0;  // MFMA path: lane-private candidate lists
    DevArray<float> sample;                                  // MFMA path: dense [256 x 8192] score matrix of the threshold sample
    bool rebalance_pending = false, rebalance_in_rerun = false; int rebalance_grid = 0;  // the exact re-run's launch also moves the full pass's tile boundaries
    DevArray<int> fb_list;      DevArray<int> fb_count;      DevArray<u32> stat;    // [kQBlock] candidates per query of the last final select
    DevArray<u64> partial;                                   // scan partials [256 slots][grid][k] keys, and the buffer the
    DevArray<u64> partial2;                                  //   select rounds ping-pong with (scan_plan.h: scan_scratch)
    DevArray<float> res_scores; DevArray<int64_t> res_idx;   size_t res_cap = 0;  // device result buffers (entries)
    DevArray<u32> mask_dev;                                  // filtered search: device copy of a host bitmask
    DevArray<float> bias_dev;                                // biased search: device copy of a host bias array
    DevArray<u32> bias_hist;                                 // biased matrix search: histogram of w * bias over the call's rows + its range (kernels_sample_biased.h)
    DevArray<u32> bias_sets_hist;                            // biased search with a weight and a set per query: [sets][kBiasBins] counts of the raw bias, then the range (kernels_biased_rowsets.h)
    const float* active_bias = nullptr; float active_bias_w = 0.f;   // per-row additive term of the search in progress (under `mu`)
    bool active_bias_matrix = false;                         // ... which runs on the matrix path (ts_search_biased_ex): the biased general-width pass
    DevArray<int64_t> id_map;                                // subset index: local row -> global id (a view of one borrows it)
    bool borrowed = false;                                   // a view: rows / id_map belong to another handle
    bool attached = false;                                   // rows adopted from the caller (ts_index_attach_device): never freed here
    ts_index* parent = nullptr;                              // a view: the handle that owns the rows
    std::atomic<int> nviews{0};                              // live views of this handle (it cannot grow meanwhile)
    DevArray<void> rank_buf;                                 // ts_rank_of: targets | counts | target scores, one query block
    DevArray<void> rank_many_buf;                            // ts_rank_many: slots | keys | counts of one pass of one query block
    const u32* active_mask = nullptr;                        // bitmask of the search in progress (under `mu`)
    RowsetsCall* active_rowsets = nullptr;                   // ts_search_rowsets' shared pass in progress: a mask per query (active_mask is NULL then)
    DevArray<void> rowsets_dev;                              // ... the block's RowsetsTable (BiasedRowsetsTable under a weight per query), then its re-run lists [256] and their counts [256]
    std::vector<unsigned char> rowsets_host;                 // ... and the host copy both are uploaded from
    int64_t active_allowed = 0;                              // rows that bitmask allows (host masks: counted; a row set's: known; else n)
    Knobs knobs;                                             // env at creation, then ts_index_set_option
    hipStream_t last_stream = nullptr;                       // stream the previous call ran on: compared, never used (it may be gone)
    DevArray<int64_t> part;     DevArray<unsigned> wg_ticks;     // full pass of the 16x16 kernel: tile boundaries per workgroup, their times
    int part_g = 0;             int64_t part_ntiles = -1;        // ... the grid and tile count the table was made for
    // int8 screen of the d = 768 (or, opt-in, 1024) bf16 full pass and, opt-in, of the d = 768 / 1024 fp32 one (kernels_screen8.h): the image [scr_pad x d] int8 + [scr_pad / 32] tile scalars,
    // brought up to date before a screened pass for the rows written since (scr_lo .. scr_hi, marked by every upload / append)
    DevArray<void> scr_rows;    DevArray<float> scr_tile;    int64_t scr_pad = 0;
    int64_t scr_lo = 0, scr_hi = 0;
    DevArray<void> scr_q;       DevArray<float> scr_qmeta;       // the launch's queries in int8 [256 x d] + their scalars
    DevArray<u64> scr_cand;     DevArray<u32> scr_count;         // the screen's lists [256][kScreenCap] + counts
    DevArray<unsigned> pair_pos;                             // paired full pass: the tile each workgroup has reached (one word per workgroup of the largest grid)
    DevArray<unsigned long long> dbg;                        // TS_MFMA_VARIANT=3: per-wave cycle sums / clock probe
    double probe_ghz = 0.0, probe_cycles_per_unit = 0.0, probe_units = 0.0;   // last clock probe (16x16 shape, VARIANT 3)
    // optional event brackets around the dominant kernel (ts_index_profile_*)
    bool profiling = false;            // (the events: IndexQueue::ev_pool)
    size_t ev_used = 0;                // events handed out since the last read
    int64_t prof_rows = 0;
    size_t elem() const { return dtype == TS_BF16 ? 2 : 4; }
};

// rows [lo, hi) were written: the int8 screen image must be brought up to date for them before its next use
inline void screen_touch(ts_index* ix, int64_t lo, int64_t hi) {
    if (hi <= lo) return;
    if (ix->scr_hi <= ix->scr_lo) { ix->scr_lo = lo; ix->scr_hi = hi; }
    else { ix->scr_lo = std::min(ix->scr_lo, lo); ix->scr_hi = std::max(ix->scr_hi, hi); }
}

// The rows' metadata as columns (meta.hip).  A scalar column: `values` [n]; a list column: `offsets` [n + 1] and `values`
// [offsets[n]], its codes.  `sets` and `allowed` are the scratch of one ts_meta_eval (under `mu`; the call waits for its
// count, so nothing of it is in flight when the next one starts).
struct ts_meta {
    int device = 0;
    int64_t n = 0;
    int ncols = 0;
    int cu_count = 256;
    std::mutex mu;
    int kind[TS_META_MAX_COLS] = {};                         // MetaColKind
    DevArray<int32_t> values[TS_META_MAX_COLS];
    DevArray<int64_t> offsets[TS_META_MAX_COLS];
    DevArray<u32> sets;
    DevArray<u64> allowed;
};

// A device row bitmask in the layout of ts_search_filtered, allocated in whole 256-row blocks (bits past n are zero), and
// the number of rows it allows
struct ts_rowset {
    int device = 0;
    int64_t n = 0, allowed = 0;
    DevArray<u32> mask;
};

struct ts_timer {
    int device = 0;
    hipEvent_t a = nullptr, b = nullptr;
    ~ts_timer() {
        if (a) hipEventDestroy(a);
        if (b) hipEventDestroy(b);
    }
};

// The staging buffer between host and device holds what ONE call moves, up to kStageBytes (larger transfers pass through it in
// pieces), in steps of 1 MiB; it only grows.  (A fixed 256 MiB per index cost the throw-away index of util.cos_sim -
// compare_embeddings.py:61, a thousand rows - 5.6 ms of hipMalloc in its upload and 0.9 ms of hipFree in its close around a
// 0.4 ms score kernel: profiles/r05m_cos_sim_phases.json.)  `floor_bytes`: the largest single piece the caller will put there.
inline int ensure_stage(ts_index* ix, size_t need, size_t floor_bytes) {
    const size_t gran = (size_t)1 << 20;
    const size_t want = std::max(std::min(kStageBytes, need), std::max(floor_bytes, (size_t)1));
    DEV_TRY(ix->stage.need((want + gran - 1) / gran * gran));
    return TS_OK;
}

// Event bracket around one launch: prof_begin records the start event and returns the stop event
// (NULL when profiling is off); the caller records it with prof_end after the launch.
inline hipEvent_t prof_begin(ts_index* ix, hipStream_t st, int64_t rows) {
    if (!ix->profiling) return nullptr;
    if (ix->ev_used + 2 > ix->ev_pool.size()) {
        if (ix->ev_pool.size() >= 16384) return nullptr;
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) != hipSuccess) return nullptr;
        if (hipEventCreate(&b) != hipSuccess) { hipEventDestroy(a); return nullptr; }
        ix->ev_pool.push_back(a);
        ix->ev_pool.push_back(b);
    }
    hipEvent_t start = ix->ev_pool[ix->ev_used], stop = ix->ev_pool[ix->ev_used + 1];
    ix->ev_used += 2;
    ix->prof_rows = rows;
    hipEventRecord(start, st);
    return stop;
}
inline void prof_end(hipEvent_t stop, hipStream_t st) {
    if (stop) hipEventRecord(stop, st);
}

// Stream of this call (NULL = the index's own).  The per-handle scratch buffers are shared by all calls: a call that
// arrives on ANOTHER stream than the previous one is ordered behind it, so that it never overwrites scratch the first
// one still reads.  The order event is recorded at the END of every entry point, on the stream of that call, while that
// stream is known to be alive (StreamScope's destructor, on every return path); the next call only waits on the event,
// and ts_index_synchronize / ts_index_destroy only synchronise on it: a caller's stream handle is never touched after
// the call that was given it has returned, so the caller may destroy the stream whenever its own work on it is done.
// Called under ix->mu.
// The index's own stream is a BLOCKING stream: it orders with the legacy null stream, which is what a torch
// default stream's handle (0 = NULL here) means - encoder kernels before an upload / search, torch ops after it.
struct StreamScope {
    ts_index* ix = nullptr;
    hipStream_t st = nullptr;
    ~StreamScope() {
        if (!ix || !ix->order_ev) return;
        // a call that is being captured into a HIP graph records nothing: an event recorded during capture belongs to the
        // graph and cannot order a later call on another stream (include/tsearch.h: captured calls are ordered by the caller)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess) (void)hipGetLastError();
        if (cap != hipStreamCaptureStatusNone) return;
        if (hipEventRecord(ix->order_ev, st) == hipSuccess) {
            ix->last_stream = st;
            ix->ordered = true;
        } else {
            (void)hipGetLastError();
        }
    }
};
inline int enter_stream(ts_index* ix, void* stream, hipStream_t* out, StreamScope* scope) {
    hipStream_t st = stream ? (hipStream_t)stream : ix->stream;
    if (!ix->order_ev) HIP_TRY(hipEventCreateWithFlags(&ix->order_ev, hipEventDisableTiming));
    if (ix->ordered && ix->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, ix->order_ev, 0));
    scope->ix = ix;
    scope->st = st;
    *out = st;
    return TS_OK;
}

inline int check_device(int device) {
    int c = 0;
    ts_device_count(&c);
    if (c <= 0) return fail(TS_ERR_NODEVICE, "no HIP device visible (libtsearch has no CPU path)");
    if (device < 0 || device >= c) return fail(TS_ERR_INVALID, "device %d out of range [0, %d)", device, c);
    return TS_OK;
}

// ---------------------------------------------------------------------------------------------
// search
// ---------------------------------------------------------------------------------------------
static inline bool mfma_dim(int d) { return d == 384 || d == 512 || d == 768 || d == 1024; }
// indexes the batched MFMA path serves: bf16 at the four widths, fp32 at d = 768 (kernels_mfma_f32.h) and d = 1024
// (kernels_mfma16.h, F32) on the exact-fp32 matrix instructions
// d = 384 / 512 on the 16x16 kernel exist as the full pass only: they need the usual two-level search (dense threshold
// sample + full pass), not the guaranteed chain (TS_MFMA_STAT=0) or the list-form sample (TS_MFMA_SAMPLE=0)
static inline bool two_level_search(const ts_index* ix) {
    return ix->knobs.get(K_MFMA_STAT, 1) != 0 && ix->knobs.get(K_MFMA_SAMPLE, 1) != 0;
}
// every other multiple of 64 from 128 up to a 4,096-byte row: the general-width kernel (kernels_mfma_anyd.h; anyd_plan.h holds the
// rule), a full pass only, so the usual two-level search as for d = 384 / 512; rows must be unpadded (ld == d: d % 64 == 0)
static inline bool anyd_index(const ts_index* ix) {
    if (ix->dtype == TS_F32 && ix->knobs.get(K_MFMA_F32, 16) == 0) return false;
    return ix->ld == ix->d && anyd_served(ix->dtype, ix->d, two_level_search(ix));
}
// the biased matrix search (bias_plan.h: bias_served): the general-width rule with the hand-laid widths included
static inline bool bias_index(const ts_index* ix) {
    if (ix->dtype == TS_F32 && ix->knobs.get(K_MFMA_F32, 16) == 0) return false;
    return ix->ld == ix->d && ix->n >= 1 && bias_served(ix->dtype, ix->d, two_level_search(ix));
}
// wider rows, d % 256 == 0 up to a 16,384-byte row: the k-chunked kernel (kernels_mfma_wide.h; wide_plan.h holds the rule), under
// the same conditions.  Disjoint from anyd_index, bias_index and the hand-laid widths; it serves the biased search too
static inline bool wide_index(const ts_index* ix) {
    if (ix->dtype == TS_F32 && ix->knobs.get(K_MFMA_F32, 16) == 0) return false;
    return ix->ld == ix->d && wide_served(ix->dtype, ix->d, two_level_search(ix));
}
// Workgroups of one matrix pass: one per CU, or TS_MFMA_GRID clamped to 1 .. kMfmaMaxGrid (search_mfma.hip: the pairs' position
// words are sized by it).  The k-chunked rank pass (rank_many.hip) takes the same grid.
constexpr int kMfmaMaxGrid = 2048;
static inline int mfma_grid(const ts_index* ix) { return std::max(1, std::min(ix->knobs.get(K_MFMA_GRID, ix->cu_count), kMfmaMaxGrid)); }
static inline bool mfma_index(const ts_index* ix) {
    if (anyd_index(ix) || wide_index(ix)) return true;
    if (ix->dtype == TS_BF16) return mfma_dim(ix->d);
    if (ix->knobs.get(K_MFMA_F32, 16) == 0) return false;
    return ix->d == 768 || ix->d == 1024 || ((ix->d == 384 || ix->d == 512) && two_level_search(ix));
}

// Which MFMA shape serves this index: d = 768 runs the 16x16x32 kernel (kernels_mfma16.h) unless TS_MFMA_SHAPE=32 asks for
// the 32x32x16 one (kernels_mfma.h), which also serves the other widths.
static inline bool use_shape16(const ts_index* ix) {
    // d = 384 / 512 (round 3): the 16x16 kernel has the full pass only for these widths, so it serves them when the search
    // is the usual two-level one (dense threshold sample + full pass); the guaranteed chain (TS_MFMA_STAT=0) and the
    // list-form sample (TS_MFMA_SAMPLE=0) run the 32x32 kernel (bf16) - fp32 at these widths has no other matrix kernel
    if (!mfma_dim(ix->d)) return false;                     // the general-width kernel is neither shape
    const bool narrow = ix->d == 384 || ix->d == 512;
    const bool two_level = two_level_search(ix);
    // fp32: the 16x16x4 form of the same kernel (10M x 768, 256 queries: 14.1 ms a pass against 14.8 ms of the 32x32x2
    // kernel, which TS_MFMA_F32=32 still selects for d = 768)
    if (ix->dtype == TS_F32) return ix->d != 768 || ix->knobs.get(K_MFMA_F32, 16) != 32;
    if (narrow && !two_level) return false;
    return ix->dtype == TS_BF16 && mfma_dim(ix->d) && ix->knobs.get(K_MFMA_SHAPE, 16) != 32;
}

// ---------------------------------------------------------------------------------------------
// functions one translation unit defines for the others
// ---------------------------------------------------------------------------------------------
namespace ts { struct MfmaArgs; struct SampleArgs; struct LevelArgs; }
// index.hip: normalise / convert / pad rows (uploads, query preparation)
int prep_dispatch(int src_dtype, int dst_dtype, bool normalize, const void* src, int64_t src_ld, void* dst, float* f32copy,
                  int64_t ld, int d, int64_t nrows, int64_t rows_total, hipStream_t st);
// search.hip: the streaming scan + its select (also the exact re-run of the matrix path: qlist / qcount on the device)
int scan_search(ts_index* ix, int nq, int k, float* out_scores, int64_t* out_idx, const int* qlist, const int* qcount,
                hipStream_t st, const float* qbuf = nullptr, const unsigned short* qb16 = nullptr);
// search.hip: a whole search as ts_search_ex / ts_search_rowset run it (validation, lock, stream order, path choice, read-back),
// for a unit that builds on searches (grouped.hip).  row_mask: NULL, or a DEVICE mask that allows known_allowed rows
int search_core(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k, float* out_scores,
                int64_t* out_idx, int out_on_device, void* stream, int algo, ts_search_stats* stats, const uint32_t* row_mask,
                int64_t known_allowed);
// search.hip: the queries of a call, one block of at most kQBlock at a time.  query_feed_open makes sure of ix->qstore (f32copy:
// and ix->qf32) and, for host queries, sizes the staging buffer once; query_feed_block copies a block of host queries there and
// prepares it (prep_dispatch: normalise (COS), round to the storage type, zero-pad to 256 rows x ld; f32copy: the fp32 copy the
// scan kernels read).
struct QueryFeed {
    ts_index* ix = nullptr;
    const char* queries = nullptr;
    size_t row_bytes = 0;
    int q_dtype = 0;
    bool on_device = false, f32copy = false;
    hipStream_t st = nullptr;
    const void* at(int q0) const { return queries + (size_t)q0 * row_bytes; }    // where block q0's queries lie, as given
};
int query_feed_open(QueryFeed* f, ts_index* ix, const void* queries, int q_dtype, int q_on_device, int nq, bool f32copy, hipStream_t st);
int query_feed_block(const QueryFeed& f, int q0, int nb);
// search_mfma.hip: the matrix path (threshold sample, full pass, final select, re-run)
int mfma_block_queries(const ts_index* ix, int nq);
// ... the histogram of the call's additive term over all (allowed) rows, once per biased matrix search (ix->active_bias, active_mask)
int bias_histogram(ts_index* ix, hipStream_t st);
int mfma_search(ts_index* ix, int nq, int k, float* out_scores, int64_t* out_idx, hipStream_t st, ts_search_stats* stats,
                const void* qmat, bool in_place);
// launch_mfma16.hip / launch_mfma16_f32.hip / launch_mfma32.hip: one launch of a matrix kernel (a full pass or a sparse level)
// on device `dev`, the handle's
int launch_pass_mfma16(int dev, int d, int nb, bool full_pass, int variant, int grid, hipStream_t st, const ts::MfmaArgs& a);
int launch_pass_mfma16_f32(int dev, int d, int nb, bool full_pass, int grid, hipStream_t st, const ts::MfmaArgs& a);
// the int8 screen + exact rescore in place of the full pass (launch_screen8.hip): screen_usable = this index, this launch;
// ksplit = the rescore takes the k-split form of the d = 1024 bf16 pass (the form the call's unscreened pass would have taken)
bool screen_usable(const ts_index* ix);
int screen_prepare(ts_index* ix, const void* qmat, int nq_launch, bool quantize_queries, hipStream_t st);
int screen_full_pass(ts_index* ix, int nb, int nq, int grid, int variant, bool ksplit, hipStream_t st, const ts::MfmaArgs& a);
// ... the screen's launch alone, the tile kernel over the image (either width)
int screen_tile_pass(ts_index* ix, int nb, int grid, int variant, hipStream_t st, const ts::MfmaArgs& a);
// ... their d = 1024 halves (launch_screen8_wide.hip)
int screen_prepare_wide(ts_index* ix, const void* qmat, int nq_launch, bool quantize_queries, hipStream_t st);
int screen_full_pass_wide(ts_index* ix, int nb, int nq, int grid, int variant, bool ksplit, hipStream_t st, const ts::MfmaArgs& a);
int screen_tile_pass_wide(ts_index* ix, int nb, int grid, int variant, hipStream_t st, const ts::MfmaArgs& a);
// ... the late-test form of the d = 768 tile kernel at four query blocks per wave, unmasked (launch_screen8_late.hip;
// TS_MFMA_SCREEN_LATE): `a` is the screen's argument block
int launch_screen8_late(int dev, int grid, hipStream_t st, const ts::MfmaArgs& a);
// ... and those of fp32 indexes (launch_screen8_f32.hip): fp32 quantisers, screen_tile_pass, the fp32 rescore
int screen_prepare_f32(ts_index* ix, const void* qmat, int nq_launch, hipStream_t st);
int screen_full_pass_f32(ts_index* ix, int nb, int nq, int grid, int variant, hipStream_t st, const ts::MfmaArgs& a);
// launch_mfma_anyd.hip: the full pass of an index the general-width kernel serves (anyd_index)
int launch_pass_mfma_anyd(const ts_index* ix, int grid, hipStream_t st, const ts::MfmaArgs& a);
// launch_mfma_anyd_biased.hip: the same pass with the call's bias term in the epilogue (ix->active_bias, active_bias_w), at any
// width of bias_index
int launch_pass_mfma_anyd_biased(const ts_index* ix, int grid, hipStream_t st, const ts::MfmaArgs& a);
// launch_mfma_anyd_rowsets.hip: the pass, the threshold sample, its select and the final select of ts_search_rowsets (a row set per
// query: ix->rowsets_dev holds the block's table), at any width of bias_index
int launch_pass_mfma_anyd_rowsets(const ts_index* ix, int grid, hipStream_t st, const ts::MfmaArgs& a);
int launch_sample_rowsets(const ts_index* ix, dim3 grid, int lds, hipStream_t st, const ts::SampleArgs& sa);
int launch_sample_select_rowsets(const ts_index* ix, int nq, hipStream_t st, const ts::LevelArgs& l, const float* scores, int row_stride);
int launch_level_select_rowsets(const ts_index* ix, int nq, hipStream_t st, const ts::LevelArgs& l);
// ts_search_biased_rowsets (a weight and a row set per query: ix->rowsets_dev holds the block's BiasedRowsetsTable, ix->active_bias
// the call's bias).  launch_mfma_anyd_biased_rowsets.hip: the pass.  search_mfma.hip: the histograms of the raw bias per set
// (masks[h]: NULL = every row), the sample select that reads them, and out_sims under a weight per query
int launch_pass_mfma_anyd_biased_rowsets(const ts_index* ix, int grid, hipStream_t st, const ts::MfmaArgs& a);
int biased_rowsets_histograms(ts_index* ix, const uint32_t* const* masks, int nhists, hipStream_t st);
int launch_sample_select_biased_rowsets(const ts_index* ix, int nq, int kk, int nhists, double target, const float* scores, int row_stride,
                                        int64_t ntiles, int64_t tile_stride, int run, hipStream_t st);
int launch_unbias_rows(const ts_index* ix, const float* scores, const int64_t* idx, const float* bias, const float* weights, int k, float* sims,
                       int64_t count, hipStream_t st);
// launch_mfma_wide.hip: the same two passes and the threshold sample of an index the k-chunked kernels serve (wide_index)
int launch_pass_mfma_wide(const ts_index* ix, int grid, hipStream_t st, const ts::MfmaArgs& a);
int launch_pass_mfma_wide_biased(const ts_index* ix, int grid, hipStream_t st, const ts::MfmaArgs& a);
int launch_sample_wide(const ts_index* ix, dim3 grid, hipStream_t st, const ts::SampleArgs& sa);
int launch_pass_mfma32(int dev, int d, int groups, bool full_pass, int variant, int grid, hipStream_t st, const ts::MfmaArgs& a);
int launch_pass_mfma32_f32(int dev, bool full_pass, int variant, int grid, hipStream_t st, const ts::MfmaArgs& a);
