// libtsearch.so - C ABI (include/tsearch.h), part 2: the search entry points (ts_search*, ts_rank_of, ts_count_above,
// ts_scores), the streaming scan path and its selects.  The matrix path lives in search_mfma.hip.
#include "host.h"
#include "kernels_scan.h"
#include "kernels_select.h"

static_assert(kSelectHistKeys == kHistSelectMax, "scan_plan.h plans the select rounds for the histogram select's capacity");

// scratch that starts zeroed: a failed allocation leaves the others as they are and is retried by the next call
template <class T>
static int need_zeroed(DevArray<T>& a, size_t bytes) {
    bool zeroing = false;
    const hipError_t e = (hipError_t)a.need_zeroed(bytes, &zeroing);
    if (zeroing) return fail(TS_ERR_HIP, "hipMemset of search scratch failed: %s", hipGetErrorString(e));
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? TS_ERR_NOMEM : TS_ERR_HIP, "hipMalloc of %zu bytes of search scratch failed: %s", bytes, hipGetErrorString(e));
    return TS_OK;
}

static int ensure_search_scratch(ts_index* ix, int k) {
    TS_TRY(need_zeroed(ix->count, (size_t)kQBlock * 4));
    DEV_TRY(ix->thr.need((size_t)kQBlock * 4));
    DEV_TRY(ix->fb_list.need((size_t)kQBlock * 4));
    TS_TRY(need_zeroed(ix->fb_count, 16));
    TS_TRY(need_zeroed(ix->stat, (size_t)kQBlock * 4));
    if (mfma_index(ix)) DEV_TRY(ix->cand.need((size_t)kQBlock * kCandCap * 8));
    // scan partials: [256 slots][grid][k] keys, and what the select rounds write (ping-pong)
    const ScanScratch keys = scan_scratch(ix->cu_count, k);
    DEV_TRY(ix->partial.need(keys.partial * 8));
    DEV_TRY(ix->partial2.need(keys.partial2 * 8));
    return TS_OK;
}

int query_feed_open(QueryFeed* f, ts_index* ix, const void* queries, int q_dtype, int q_on_device, int nq, bool f32copy, hipStream_t st) {
    f->ix = ix;
    f->queries = (const char*)queries;
    f->row_bytes = (size_t)ix->d * (q_dtype == TS_BF16 ? 2 : 4);
    f->q_dtype = q_dtype;
    f->on_device = q_on_device != 0;
    f->f32copy = f32copy;
    f->st = st;
    DEV_TRY(ix->qstore.need((size_t)kQBlock * ix->ld * ix->elem()));
    if (f32copy) DEV_TRY(ix->qf32.need((size_t)kQBlock * ix->ld * 4));
    if (!f->on_device) TS_TRY(ensure_stage(ix, (size_t)std::min(nq, kQBlock) * f->row_bytes, 0));   // one block of queries at a time
    return TS_OK;
}

int query_feed_block(const QueryFeed& f, int q0, int nb) {
    ts_index* ix = f.ix;
    const void* qsrc = f.at(q0);
    if (!f.on_device) {
        const hipError_t e = hipMemcpyAsync(ix->stage, qsrc, (size_t)nb * f.row_bytes, hipMemcpyHostToDevice, f.st);
        if (e != hipSuccess) return fail(TS_ERR_HIP, "copy of the queries failed: %s", hipGetErrorString(e));
        qsrc = ix->stage;
    }
    return prep_dispatch(f.q_dtype, ix->dtype, ix->metric == TS_METRIC_COS, qsrc, ix->d, ix->qstore, f.f32copy ? ix->qf32 : nullptr,
                         ix->ld, ix->d, nb, kQBlock, f.st);
}

// The scan and rank launchers return the status of their own launch (as launch_lds does): no caller checks it again.
template <int DT, int CH, int G, bool EMIT>
static int launch_scan_spec(int qb, int kr, int grid, hipStream_t st, const ScanArgs& a) {
    if (EMIT) {
        if (qb == 4) scan_kernel<DT, CH, G, 4, 1, true><<<grid, 256, 0, st>>>(a);
        else scan_kernel<DT, CH, G, 1, 1, true><<<grid, 256, 0, st>>>(a);
    } else if (qb == 4) {
        if (kr == 1) scan_kernel<DT, CH, G, 4, 1, false><<<grid, 256, 0, st>>>(a);
        else scan_kernel<DT, CH, G, 4, 4, false><<<grid, 256, 0, st>>>(a);
    } else {
        if (kr == 1) scan_kernel<DT, CH, G, 1, 1, false><<<grid, 256, 0, st>>>(a);
        else scan_kernel<DT, CH, G, 1, 4, false><<<grid, 256, 0, st>>>(a);
    }
    HIP_TRY(hipGetLastError());
    return TS_OK;
}

// any other width: queries staged in LDS
template <int DT, bool EMIT>
static int launch_scan_generic(int dev, int qb_pref, int kr, int grid, hipStream_t st, const ScanArgs& a) {
    const int qb = scan_generic_qb(qb_pref, a.ld, kr, EMIT);
    const int lds = scan_generic_lds(a.ld, qb);
    if (qb == 4) return launch_lds<scan_generic_kernel<DT, 1, EMIT, 4>>(dev, grid, 256, lds, st, a);
    if (EMIT || kr == 1) return launch_lds<scan_generic_kernel<DT, 1, EMIT, 1>>(dev, grid, 256, lds, st, a);
    return launch_lds<scan_generic_kernel<DT, 4, EMIT, 1>>(dev, grid, 256, lds, st, a);   // k > 64: four lists of 4 keys per lane do not fit; one query per pass
}

// The kernel form of this index's rows (scan_plan.h: kScanWidth): go(DT, CH, G) as std::integral_constants, CH = 0 for the
// generic kernels (every other width, or TS_SCAN_GENERIC).
template <int V> using int_c = std::integral_constant<int, V>;
template <class Go, size_t... I>
static int with_scan_width(const ts_index* ix, Go&& go, std::index_sequence<I...>) {
    const int w = ix->knobs.get(K_SCAN_GENERIC, 0) != 0 ? -1 : scan_width(ix->dtype, ix->ld);
    int rc = TS_OK;
    if (((w == (int)I && ((rc = go(int_c<kScanWidth[I].dtype>{}, int_c<kScanWidth[I].ch>{}, int_c<kScanWidth[I].g>{})), true)) || ...))
        return rc;
    return ix->dtype == TS_F32 ? go(int_c<TS_F32>{}, int_c<0>{}, int_c<0>{}) : go(int_c<TS_BF16>{}, int_c<0>{}, int_c<0>{});
}

// One scan pass configuration for (dtype, ld).
template <bool EMIT>
static int launch_scan(const ts_index* ix, const ScanArgs& a, int qb_pref, hipStream_t st, int grid) {
    const int kr = scan_kr(a.k);
    return with_scan_width(ix, [&](auto dt, auto ch, auto g) {
        if constexpr (ch.value == 0) return launch_scan_generic<dt.value, EMIT>(ix->device, qb_pref, kr, grid, st, a);
        else return launch_scan_spec<dt.value, ch.value, g.value, EMIT>(qb_pref, kr, grid, st, a);
    }, std::make_index_sequence<kScanWidths>{});
}

// Reduce [slots][m] partial keys to the final k per query: the rounds of select_plan(m, k).
static int run_select_rounds(ts_index* ix, int slots, int m, int k, float* out_scores, int64_t* out_idx, const int* qlist,
                             const int* qcount, hipStream_t st) {
    const SelectPlan p = select_plan(m, k);
    if (p.nrounds < 0) return fail(TS_ERR_INTERNAL, "no select plan for %d keys per query at k = %d", m, k);
    SelectArgs a;
    memset(&a, 0, sizeof(a));
    a.in = ix->partial;
    a.in_stride = m;
    a.m = m;
    a.kout = k;
    a.k_user = k;
    a.row_offset = ix->row_offset;
    a.id_map = ix->id_map;
    a.qlist = qlist;
    a.qcount = qcount;
    for (int r = 0; r < p.nrounds; ++r) {
        const SelectRound& rd = p.round[r];
        a.out = (r & 1) ? ix->partial : ix->partial2;
        a.out_stride = rd.out;
        if ((size_t)slots * rd.out * 8 > ((r & 1) ? ix->partial : ix->partial2).bytes())
            return fail(TS_ERR_INTERNAL, "select round %d of %d x %d keys does not fit its scratch", r, slots, rd.out);
        if (rd.seg == 4096) select_kernel<4096><<<dim3(rd.nseg, slots), 256, 0, st>>>(a);
        else select_kernel<1024><<<dim3(rd.nseg, slots), 256, 0, st>>>(a);
        HIP_TRY(hipGetLastError());
        a.in = a.out;
        a.in_stride = a.out_stride;
        a.m = rd.out;
    }
    a.out = nullptr;
    a.out_stride = 0;
    a.out_scores = out_scores;
    a.out_idx = out_idx;
    if (p.final_form == kSelectHist) {
        if (p.hist_kr == 1) return launch_lds<select_hist_kernel<1>>(ix->device, slots, kLevelThreads, kHistSelectLds, st, a);
        return launch_lds<select_hist_kernel<4>>(ix->device, slots, kLevelThreads, kHistSelectLds, st, a);
    }
    if (p.final_form == kSelectSort1024) select_kernel<1024><<<dim3(1, slots), 256, 0, st>>>(a);
    else select_kernel<4096><<<dim3(1, slots), 256, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    return TS_OK;
}

// `qbuf`: fp32 queries to read instead of the prepared copy; `qb16`: bf16 queries to read in place (the caller's matrix).
int scan_search(ts_index* ix, int nq, int k, float* out_scores, int64_t* out_idx, const int* qlist, const int* qcount,
                hipStream_t st, const float* qbuf, const unsigned short* qb16) {
    // The exact re-run of the MFMA path (device-side query count, almost always zero) is ONE launch: the workgroup that
    // finishes last reduces the partial lists itself (scan_finish), so the common case pays one empty launch, not one per
    // select round as well.
    // (Tried for the app's own shape too - one to four queries, small k - in place of the separate histogram select:
    // 0.471 -> 0.505 ms per search on 1M x 768 fp32, 53 instead of 33 us on 1,000 rows: every workgroup's release fence and
    // the last workgroup's serial sweep of 10,240 keys cost more than the second launch.  The re-run path only.)
    const bool one_launch = qcount != nullptr;
    const ScanPass pass = scan_pass(ix->cu_count, ix->n, ix->dtype, ix->ld, nq, k, one_launch);
    ScanArgs a;
    memset(&a, 0, sizeof(a));
    a.corpus = ix->rows;
    a.ld = ix->ld;
    a.n = ix->n;
    a.qbuf = qb16 ? nullptr : (qbuf ? qbuf : ix->qf32);
    a.qb16 = qb16;
    a.qlist = qlist;
    a.qcount = qcount;
    a.nq = nq;
    a.k = k;
    a.partial = ix->partial;
    a.row_mask = ix->active_mask;
    a.bias = ix->active_bias;
    a.bias_w = ix->active_bias_w;
    if (one_launch) {
        a.done_ctr = ix->fb_count.as<unsigned>() + 2;    // zeroed with the block, left zeroed by the kernel
        a.out_scores = out_scores;
        a.out_idx = out_idx;
        a.row_offset = ix->row_offset;
        a.id_map = ix->id_map;
        if (ix->rebalance_pending && ix->rebalance_in_rerun && ix->rebalance_grid <= 256) {
            a.part = ix->part;
            a.wg_ticks = ix->wg_ticks;
            a.part_g = ix->rebalance_grid;
            const int b = ix->knobs.get(K_MFMA_BALANCE, 1);      // TS_MFMA_BALANCE = n > 1: gain n / 10 (default 0.7)
            a.part_gain = (b >= 2 && b <= 10) ? 0.1f * (float)b : 0.7f;
            ix->rebalance_pending = false;
        }
    }
    hipEvent_t stop = qcount ? nullptr : prof_begin(ix, st, ix->n);  // the MFMA path's fall-back pass is not bracketed
    const int rc = launch_scan<false>(ix, a, pass.qb, st, pass.grid);
    prof_end(stop, st);
    TS_TRY(rc);
    if (one_launch) return TS_OK;
    return run_select_rounds(ix, nq, pass.grid * k, k, out_scores, out_idx, qlist, qcount, st);
}

struct BiasSpec {       // ts_search_biased: rank by score + weight * bias[row]
    const float* bias = nullptr;
    int on_device = 0;
    float weight = 0.f;
    float* out_sims = nullptr;   // optional: raw similarities of the results, where the scores go
    bool ex = false;             // ts_search_biased_ex: the call may run on the matrix path (bias_plan.h decides)
};

// ---- search_impl's stages -------------------------------------------------------------------------------------------------
static int search_validate(const ts_index* ix, const void* queries, int q_dtype, int32_t nq, int32_t k, const float* out_scores,
                           const int64_t* out_idx, int algo) {
    if (!ix || !queries || !out_scores || !out_idx) return fail(TS_ERR_INVALID, "NULL argument");
    if (q_dtype != TS_F32 && q_dtype != TS_BF16) return fail(TS_ERR_INVALID, "q_dtype %d", q_dtype);
    if (nq < 0) return fail(TS_ERR_INVALID, "nq = %d", nq);
    if (k < 1 || k > TS_MAX_K) return fail(TS_ERR_INVALID, "k = %d outside [1, %d]", k, TS_MAX_K);
    if (algo < TS_ALGO_AUTO || algo > TS_ALGO_MFMA) return fail(TS_ERR_INVALID, "algo %d", algo);
    if (algo == TS_ALGO_MFMA && !(mfma_index(ix) && ix->n >= 1))
        return fail(TS_ERR_UNSUPPORTED, "the MFMA path needs a bf16 or fp32 index with d = 384, 512, 768 or 1024, or with any other multiple of 64 "
                                        "from 128 up to a 4,096-byte row (bf16 d <= 2048, fp32 d <= 960) or any multiple of 256 from there up to a "
                                        "16,384-byte row (bf16 d = 2304 .. 8192, fp32 d = 1280 .. 4096) under the default two-level search");
    return TS_OK;
}

// the bias and the bitmask of this call, on the device (search_impl's MaskScope takes them off again)
static int install_bias(ts_index* ix, const BiasSpec& bias, hipStream_t st) {
    ix->active_bias = bias.bias;
    if (!bias.on_device) {
        DEV_TRY(ix->bias_dev.need(std::max<size_t>((size_t)ix->n * 4, 4)));
        HIP_TRY(hipMemcpyAsync(ix->bias_dev, bias.bias, (size_t)ix->n * 4, hipMemcpyHostToDevice, st));
        ix->active_bias = ix->bias_dev;
    }
    ix->active_bias_w = bias.weight;
    return TS_OK;
}

static int install_mask(ts_index* ix, const uint32_t* row_mask, int mask_on_device, hipStream_t st) {
    ix->active_mask = row_mask;
    if (!mask_on_device) {
        const size_t words = (size_t)((ix->n + 31) / 32);
        DEV_TRY(ix->mask_dev.need(std::max<size_t>(words * 4, 4)));
        HIP_TRY(hipMemcpyAsync(ix->mask_dev, row_mask, words * 4, hipMemcpyHostToDevice, st));
        ix->active_mask = ix->mask_dev;
    }
    return TS_OK;
}

// scan or matrix path (scan_plan.h: choose_algo); a host mask whose density decides is counted here.  known_allowed >= 0: the
// rows a device mask allows (a row set's count)
static int search_choose(ts_index* ix, int algo, int nq, int k, const BiasSpec* bias, const uint32_t* row_mask, int mask_on_device,
                         int64_t known_allowed, int* use) {
    AlgoInputs in;
    in.algo = algo;
    in.mfma_ok = mfma_index(ix) && ix->n >= 1;
    in.n = ix->n;
    in.nq = nq;
    in.k = k;
    in.mfma_min_rows = ix->knobs.get(K_MFMA_MIN_ROWS, 16384);
    // the general-width kernel's limit comes from its own measurement (anyd_plan.h)
    const bool anyd = anyd_index(ix);
    const bool wide = wide_index(ix);                      // ... and the k-chunked kernel's from wide_plan.h
    in.scan_max_queries = ix->knobs.get(K_SCAN_MAX_QUERIES, anyd ? anyd_scan_max_queries(ix->dtype) : wide ? wide_scan_max_queries(ix->dtype) : 4);
    // k > 64 on the fp32 general-width kernel: choose_algo() lets every batch of two through, the measured limit is two
    // (anyd_scan_limit); the kernel is then not offered to AUTO.  TS_SCAN_MAX_QUERIES, when set, is the only limit.
    if (anyd && algo == TS_ALGO_AUTO && !ix->knobs.set[K_SCAN_MAX_QUERIES] && nq <= anyd_scan_limit(ix->dtype, k)) in.mfma_ok = false;
    if (wide && algo == TS_ALGO_AUTO && !ix->knobs.set[K_SCAN_MAX_QUERIES] && nq <= wide_scan_limit(ix->dtype, k)) in.mfma_ok = false;
    in.bias = bias != nullptr;
    in.subset = ix->id_map != nullptr;
    in.mask = row_mask != nullptr;
    in.mask_on_device = mask_on_device != 0;
    in.allowed = 0;
    in.allowed_known = row_mask && mask_on_device && known_allowed >= 0;
    if (in.allowed_known) ix->active_allowed = in.allowed = known_allowed;
    if (bias && bias->ex) {
        // ts_search_biased_ex decides with its own rule (bias_plan.h): the biased general-width pass serves the hand-laid
        // widths too, and its AUTO limit is its own
        // (bias_served is the narrower widths' rule; at the k-chunked widths the biased pass is mfma_wide_kernel's)
        const bool served = bias_index(ix) || (wide && ix->n >= 1);
        in.scan_max_queries = ix->knobs.get(K_SCAN_MAX_QUERIES, bias_scan_max_queries(ix->dtype));
        if (mask_wants_count(bias_algo_inputs(in, served))) ix->active_allowed = in.allowed = count_allowed_rows(row_mask, ix->n);
        const AlgoChoice c = choose_bias_algo(in, served);
        if (c.unsupported && algo == TS_ALGO_MFMA && !served && !in.subset)
            return fail(TS_ERR_UNSUPPORTED, "%s, or one whose width is a multiple of 256 up to a 16,384-byte row", c.unsupported);
        if (c.unsupported) return fail(TS_ERR_UNSUPPORTED, "%s", c.unsupported);
        *use = c.algo;
        ix->active_bias_matrix = c.algo == TS_ALGO_MFMA;
        return TS_OK;
    }
    if (mask_wants_count(in)) ix->active_allowed = in.allowed = count_allowed_rows(row_mask, ix->n);
    const AlgoChoice c = choose_algo(in);
    if (c.unsupported) return fail(TS_ERR_UNSUPPORTED, "%s", c.unsupported);
    *use = c.algo;
    return TS_OK;
}

// where the kernels write the results: the caller's device buffers, or the handle's (read back at the end)
static int result_buffers(ts_index* ix, size_t want, int out_on_device, float** dscores, int64_t** didx) {
    if (out_on_device) return TS_OK;
    if (ix->res_cap < want) {
        ix->res_cap = 0;
        DEV_TRY(remake(ix->res_scores, want * 4, ix->res_idx, want * 8));
        ix->res_cap = want;
    }
    *dscores = ix->res_scores;
    *didx = ix->res_idx;
    return TS_OK;
}

// queries are served in blocks: 256 per pass, or what one launch of the MFMA kernel holds
static int search_blocks(ts_index* ix, const QueryFeed& feed, int use, int block, int nq, int k, float* dscores, int64_t* didx,
                         ts_search_stats* stats) {
    hipStream_t st = feed.st;
    for (int q0 = 0; q0 < nq; q0 += block) {
        const int nb = std::min(block, nq - q0);
        const void* qsrc = feed.at(q0);
        float* os = dscores + (size_t)q0 * k;
        int64_t* oi = didx + (size_t)q0 * k;
        // One fp32 query against an fp32 inner-product index whose rows are not padded (the single query of the apps,
        // streamlit_app.py:173, app_showcase_model.py:92; configs[1]): nothing to normalise, round or pad - the scan
        // reads the query where it is (device) or where the copy puts it (host).  No preparation launch.
        if (use == TS_ALGO_SCAN && nb == 1 && nq == 1 && feed.q_dtype == TS_F32 && ix->dtype == TS_F32 &&
            ix->metric == TS_METRIC_IP && ix->ld == ix->d && ((uintptr_t)qsrc & 3) == 0) {
            const float* qb = (const float*)qsrc;
            if (!feed.on_device) {
                HIP_TRY(hipMemcpyAsync(ix->qf32, qsrc, (size_t)ix->d * 4, hipMemcpyHostToDevice, st));
                qb = ix->qf32;
            }
            TS_TRY(scan_search(ix, 1, k, os, oi, nullptr, nullptr, st, qb));
            continue;
        }
        // Device queries that already are what the matrix kernels multiply - the index's storage type, an inner-product
        // index (nothing to normalise), rows not padded, a whole launch's worth of them, 16-byte aligned - are read where
        // they lie: no preparation launch (the encoder's fused pooling writes this form, ts_pool_normalize with
        // out_dtype = the index's; bench.py's resident query batch).  They must stay unchanged until the search has run.
        if (use == TS_ALGO_MFMA && feed.on_device && feed.q_dtype == ix->dtype && ix->metric == TS_METRIC_IP && ix->ld == ix->d &&
            nb == block && ((uintptr_t)qsrc & 15) == 0) {
            TS_TRY(mfma_search(ix, nb, k, os, oi, st, stats, qsrc, true));
            continue;
        }
        TS_TRY(query_feed_block(feed, q0, nb));
        if (use == TS_ALGO_MFMA) TS_TRY(mfma_search(ix, nb, k, os, oi, st, stats, ix->qstore, false));
        else TS_TRY(scan_search(ix, nb, k, os, oi, nullptr, nullptr, st));
    }
    return TS_OK;
}

// ts_search_biased's out_sims: the raw similarities of the results (`tmp` holds them until a host caller's copy has run)
static int search_unbias(ts_index* ix, const BiasSpec& bias, int64_t cnt, const float* dscores, const int64_t* didx,
                         int out_on_device, DevBuf* tmp, hipStream_t st) {
    float* dsims = bias.out_sims;
    if (!out_on_device) {
        DEV_TRY(tmp->need((size_t)cnt * 4));
        dsims = tmp->as<float>();
    }
    unbias_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, st>>>(dscores, didx, ix->active_bias, ix->active_bias_w, ix->row_offset, dsims, cnt);
    HIP_TRY(hipGetLastError());
    if (!out_on_device) HIP_TRY(hipMemcpyAsync(bias.out_sims, dsims, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
    return TS_OK;
}

// results to a host caller, the matrix path's counters to `stats`; synchronises for either
static int search_read_back(ts_index* ix, int use, int block, int nq, int k, const float* dscores, const int64_t* didx,
                            float* out_scores, int64_t* out_idx, int out_on_device, ts_search_stats* stats, hipStream_t st) {
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(out_scores, dscores, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_idx, didx, (size_t)nq * k * 8, hipMemcpyDeviceToHost, st));
    }
    if (out_on_device && !stats) return TS_OK;
    int fb = 0;
    std::vector<u32> cands_q;
    const int last_nb = nq - (nq - 1) / block * block;     // queries of the last block: what the counters describe
    if (stats && use == TS_ALGO_MFMA) {
        cands_q.resize((size_t)last_nb);
        HIP_TRY(hipMemcpyAsync(&fb, ix->fb_count, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(cands_q.data(), ix->stat, (size_t)last_nb * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (stats && use == TS_ALGO_MFMA) {
        stats->fallback_queries = fb;
        int64_t cands = 0;
        for (u32 c_ : cands_q) cands += c_;
        stats->candidates = cands;
    }
    return TS_OK;
}

static int search_impl(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                       float* out_scores, int64_t* out_idx, int out_on_device, void* stream, int algo,
                       ts_search_stats* stats, const uint32_t* row_mask = nullptr, int mask_on_device = 0,
                       const BiasSpec* bias = nullptr, int64_t known_allowed = -1) {
    if (stats) memset(stats, 0, sizeof(*stats));
    TS_TRY(search_validate(ix, queries, q_dtype, nq, k, out_scores, out_idx, algo));
    if (nq == 0) return TS_OK;
    std::lock_guard<std::mutex> lock(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st;
    StreamScope scope;
    TS_TRY(enter_stream(ix, stream, &st, &scope));
    TS_TRY(ensure_search_scratch(ix, k));
    struct MaskScope {  // the bitmask and the bias are properties of this call only
        ts_index* ix;
        ~MaskScope() { ix->active_mask = nullptr; ix->active_bias = nullptr; ix->active_bias_matrix = false; }
    } mask_scope{ix};
    if (bias) TS_TRY(install_bias(ix, *bias, st));
    if (row_mask) TS_TRY(install_mask(ix, row_mask, mask_on_device, st));
    int use = TS_ALGO_SCAN;
    TS_TRY(search_choose(ix, algo, nq, k, bias, row_mask, mask_on_device, known_allowed, &use));
    if (stats) stats->algo = use;

    float* dscores = out_scores;
    int64_t* didx = out_idx;
    TS_TRY(result_buffers(ix, (size_t)nq * k, out_on_device, &dscores, &didx));
    QueryFeed feed;
    TS_TRY(query_feed_open(&feed, ix, queries, q_dtype, q_on_device, nq, true, st));
    if (ix->active_bias_matrix) TS_TRY(bias_histogram(ix, st));
    const int block = (use == TS_ALGO_MFMA) ? mfma_block_queries(ix, nq) : kQBlock;
    TS_TRY(search_blocks(ix, feed, use, block, nq, k, dscores, didx, stats));
    DevBuf sims_tmp;
    if (bias && bias->out_sims) TS_TRY(search_unbias(ix, *bias, (int64_t)nq * k, dscores, didx, out_on_device, &sims_tmp, st));
    return search_read_back(ix, use, block, nq, k, dscores, didx, out_scores, out_idx, out_on_device, stats, st);
}

// search_impl for the other translation units (grouped.hip): row_mask, when given, is a device mask that allows known_allowed rows
int search_core(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k, float* out_scores,
                int64_t* out_idx, int out_on_device, void* stream, int algo, ts_search_stats* stats, const uint32_t* row_mask,
                int64_t known_allowed) {
    return search_impl(ix, queries, q_dtype, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream, algo, stats, row_mask,
                       row_mask ? 1 : 0, nullptr, known_allowed);
}

extern "C" int ts_search_ex(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                            float* out_scores, int64_t* out_idx, int out_on_device, void* stream, int algo,
                            ts_search_stats* stats) {
    return search_impl(ix, queries, q_dtype, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream, algo, stats);
}

extern "C" int ts_search(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                         float* out_scores, int64_t* out_idx, int out_on_device, void* stream) {
    return search_impl(ix, queries, q_dtype, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream, TS_ALGO_AUTO,
                       nullptr);
}

extern "C" int ts_search_filtered(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                                  const uint32_t* row_mask, int mask_on_device, float* out_scores, int64_t* out_idx,
                                  int out_on_device, void* stream) {
    if (!row_mask) return fail(TS_ERR_INVALID, "row_mask is NULL");
    return search_impl(ix, queries, q_dtype, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream, TS_ALGO_AUTO,
                       nullptr, row_mask, mask_on_device);
}

extern "C" int ts_search_filtered_ex(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                                     const uint32_t* row_mask, int mask_on_device, float* out_scores, int64_t* out_idx,
                                     int out_on_device, void* stream, int algo, ts_search_stats* stats) {
    if (!row_mask) return fail(TS_ERR_INVALID, "row_mask is NULL");
    return search_impl(ix, queries, q_dtype, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream, algo, stats,
                       row_mask, mask_on_device);
}

extern "C" int ts_search_biased(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                                const float* bias, int bias_on_device, float weight, const uint32_t* row_mask, int mask_on_device,
                                float* out_scores, float* out_sims, int64_t* out_idx, int out_on_device, void* stream) {
    if (!bias) return fail(TS_ERR_INVALID, "bias is NULL");
    if (!(weight == weight) || std::isinf(weight)) return fail(TS_ERR_INVALID, "weight must be finite");
    BiasSpec b;
    b.bias = bias;
    b.on_device = bias_on_device;
    b.weight = weight;
    b.out_sims = out_sims;
    return search_impl(ix, queries, q_dtype, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream, TS_ALGO_AUTO, nullptr,
                       row_mask, mask_on_device, &b);
}

extern "C" int ts_search_biased_ex(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                                   const float* bias, int bias_on_device, float weight, const uint32_t* row_mask, int mask_on_device,
                                   float* out_scores, float* out_sims, int64_t* out_idx, int out_on_device, void* stream, int algo,
                                   ts_search_stats* stats) {
    if (!bias) return fail(TS_ERR_INVALID, "bias is NULL");
    if (!(weight == weight) || std::isinf(weight)) return fail(TS_ERR_INVALID, "weight must be finite");
    BiasSpec b;
    b.bias = bias;
    b.on_device = bias_on_device;
    b.weight = weight;
    b.out_sims = out_sims;
    b.ex = true;
    return search_impl(ix, queries, q_dtype, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream, algo, stats, row_mask,
                       mask_on_device, &b);
}

// the mask and its count from a row set (meta.hip): one of this index's shape, on its device
static int rowset_check(const ts_index* ix, const ts_rowset* rows) {
    if (!ix || !rows) return fail(TS_ERR_INVALID, "NULL argument");
    if (rows->n != ix->n) return fail(TS_ERR_INVALID, "the row set has %lld rows, the index %lld", (long long)rows->n, (long long)ix->n);
    if (rows->device != ix->device) return fail(TS_ERR_INVALID, "the row set lives on device %d, the index on device %d", rows->device, ix->device);
    return TS_OK;
}

extern "C" int ts_search_rowset(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                                const ts_rowset* rows, float* out_scores, int64_t* out_idx, int out_on_device, void* stream, int algo,
                                ts_search_stats* stats) {
    TS_TRY(rowset_check(ix, rows));
    return search_impl(ix, queries, q_dtype, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream, algo, stats, rows->mask, 1,
                       nullptr, rows->allowed);
}

extern "C" int ts_search_biased_rowset(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                                       const float* bias, int bias_on_device, float weight, const ts_rowset* rows, float* out_scores,
                                       float* out_sims, int64_t* out_idx, int out_on_device, void* stream, int algo,
                                       ts_search_stats* stats) {
    if (!bias) return fail(TS_ERR_INVALID, "bias is NULL");
    if (!(weight == weight) || std::isinf(weight)) return fail(TS_ERR_INVALID, "weight must be finite");
    TS_TRY(rowset_check(ix, rows));
    BiasSpec b;
    b.bias = bias;
    b.on_device = bias_on_device;
    b.weight = weight;
    b.out_sims = out_sims;
    b.ex = true;
    return search_impl(ix, queries, q_dtype, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream, algo, stats, rows->mask, 1,
                       &b, rows->allowed);
}

// ---- ts_search_rowsets: a row set per query (rowsets_plan.h holds the rules) ---------------------------------------------------
// The shared pass for `nq` queries that all ride it (validated, routed): search_impl's stages with a mask per query.  which[q]:
// the set of query q.  Blocks of kRowsetsBlock queries; each block waits for its re-run list (search_mfma.hip: rowsets_rerun).
// ts_search_biased_rowsets: the same with `bias` (device) and weights[q], the weight of query q - the biased pass with a weight per
// query, behind one histogram of the raw bias per distinct set of these queries (made here, once, before the first block).
static int rowsets_pass(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k, const ts_rowset* const* sets,
                        const int32_t* which, float* out_scores, int64_t* out_idx, int out_on_device, void* stream, ts_rowsets_stats* stats,
                        const float* bias = nullptr, const float* weights = nullptr) {
    std::lock_guard<std::mutex> lock(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st;
    StreamScope scope;
    TS_TRY(enter_stream(ix, stream, &st, &scope));
    TS_TRY(ensure_search_scratch(ix, k));
    RowsetsCall call;
    call.sets = sets;
    struct Scope {      // the sets are properties of this call only
        ts_index* ix;
        ~Scope() { ix->active_rowsets = nullptr; ix->active_mask = nullptr; ix->active_bias = nullptr; ix->active_bias_matrix = false; }
    } call_scope{ix};
    ix->active_rowsets = &call;
    float* dscores = out_scores;
    int64_t* didx = out_idx;
    TS_TRY(result_buffers(ix, (size_t)nq * k, out_on_device, &dscores, &didx));
    QueryFeed feed;
    TS_TRY(query_feed_open(&feed, ix, queries, q_dtype, q_on_device, nq, true, st));
    const int block = mfma_block_queries(ix, nq);
    if (block != kRowsetsBlock) return fail(TS_ERR_INTERNAL, "a block of the row-set pass holds %d queries, not %d", kRowsetsBlock, block);
    std::vector<int32_t> hist_of, hist_sets;
    if (bias) {
        ix->active_bias = bias;
        ix->active_bias_w = 0.0f;           // (the pass reads the table's weights; the re-run sets its class's)
        ix->active_bias_matrix = true;
        call.nhists = biased_rowsets_hists(which, nq, &hist_of, &hist_sets);
        std::vector<const uint32_t*> masks(hist_sets.size());
        for (size_t h = 0; h < hist_sets.size(); ++h) masks[h] = hist_sets[h] < 0 ? nullptr : (const uint32_t*)sets[hist_sets[h]]->mask;
        TS_TRY(biased_rowsets_histograms(ix, masks.data(), call.nhists, st));
    }
    for (int q0 = 0; q0 < nq; q0 += block) {
        const int nb = std::min(block, nq - q0);
        const void* qsrc = feed.at(q0);
        call.which = which + q0;
        if (bias) {
            call.weights = weights + q0;
            call.hist_of = hist_of.data() + q0;
        }
        // device queries that already are what the kernels multiply are read where they lie (search_blocks' rule)
        if (feed.on_device && feed.q_dtype == ix->dtype && ix->metric == TS_METRIC_IP && ix->ld == ix->d && nb == block && ((uintptr_t)qsrc & 15) == 0) {
            TS_TRY(mfma_search(ix, nb, k, dscores + (size_t)q0 * k, didx + (size_t)q0 * k, st, nullptr, qsrc, true));
            continue;
        }
        TS_TRY(query_feed_block(feed, q0, nb));
        TS_TRY(mfma_search(ix, nb, k, dscores + (size_t)q0 * k, didx + (size_t)q0 * k, st, nullptr, ix->qstore, false));
    }
    if (stats) {
        stats->fallback_queries += call.fallback_queries;
        stats->candidates += call.candidates;
    }
    if (out_on_device) return TS_OK;
    HIP_TRY(hipMemcpyAsync(out_scores, dscores, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_idx, didx, (size_t)nq * k * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return TS_OK;
}

// Some of a call's queries (`sel`, ascending) as a call of their own: gathered into contiguous rows where the caller's lie (host or
// device), run(queries, out_scores, out_idx), and the result rows put back at their places.  Device temporaries are the call's own
// (the per-handle scratch belongs to the searches `run` makes); the stream is drained before they go.
template <class Run>
static int rowsets_subset(ts_index* ix, const std::vector<int32_t>& sel, const void* queries, size_t q_row_bytes, int q_on_device, int32_t nq,
                          int32_t k, float* out_scores, int64_t* out_idx, int out_on_device, void* stream, Run&& run) {
    const size_t m = sel.size();
    if (m == 0) return TS_OK;
    if (m == (size_t)nq) return run(queries, out_scores, out_idx);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = stream ? (hipStream_t)stream : ix->stream;
    std::vector<unsigned char> hq;
    std::vector<float> hs;
    std::vector<int64_t> hi;
    DevBuf dq, dout;
    const void* q_sub = nullptr;
    float* s_sub = nullptr;
    int64_t* i_sub = nullptr;
    int rc = TS_OK;
    auto enqueue = [&]() -> int {
        if (q_on_device) {
            DEV_TRY(dq.need(m * q_row_bytes));
            for (size_t j = 0; j < m; ++j)
                HIP_TRY(hipMemcpyAsync(dq.as<unsigned char>() + j * q_row_bytes, (const unsigned char*)queries + (size_t)sel[j] * q_row_bytes, q_row_bytes,
                                       hipMemcpyDeviceToDevice, st));
            q_sub = dq;
        } else {
            hq.resize(m * q_row_bytes);
            for (size_t j = 0; j < m; ++j) memcpy(hq.data() + j * q_row_bytes, (const unsigned char*)queries + (size_t)sel[j] * q_row_bytes, q_row_bytes);
            q_sub = hq.data();
        }
        if (out_on_device) {
            DEV_TRY(dout.need(m * k * 12));
            i_sub = dout.as<int64_t>();
            s_sub = (float*)(i_sub + m * k);
        } else {
            hs.resize(m * k);
            hi.resize(m * k);
            s_sub = hs.data();
            i_sub = hi.data();
        }
        TS_TRY(run(q_sub, s_sub, i_sub));
        for (size_t j = 0; j < m; ++j) {
            if (out_on_device) {
                HIP_TRY(hipMemcpyAsync(out_scores + (size_t)sel[j] * k, s_sub + j * k, (size_t)k * 4, hipMemcpyDeviceToDevice, st));
                HIP_TRY(hipMemcpyAsync(out_idx + (size_t)sel[j] * k, i_sub + j * k, (size_t)k * 8, hipMemcpyDeviceToDevice, st));
            } else {
                memcpy(out_scores + (size_t)sel[j] * k, s_sub + j * k, (size_t)k * 4);
                memcpy(out_idx + (size_t)sel[j] * k, i_sub + j * k, (size_t)k * 8);
            }
        }
        return TS_OK;
    };
    rc = enqueue();
    // every path drains the stream before the device temporaries are freed
    if (q_on_device || out_on_device) {
        const hipError_t e = hipStreamSynchronize(st);
        if (rc == TS_OK && e != hipSuccess) rc = fail(TS_ERR_HIP, "stream synchronize failed: %s", hipGetErrorString(e));
    }
    return rc;
}

// the padding of a query whose set allows nothing: -inf / -1, without a launch of the search
static int rowsets_padding(ts_index* ix, const std::vector<int32_t>& sel, int32_t k, float* out_scores, int64_t* out_idx, int out_on_device,
                           void* stream) {
    std::vector<float> s((size_t)k, -INFINITY);
    std::vector<int64_t> i((size_t)k, -1);
    if (!out_on_device) {
        for (int32_t q : sel) {
            memcpy(out_scores + (size_t)q * k, s.data(), (size_t)k * 4);
            memcpy(out_idx + (size_t)q * k, i.data(), (size_t)k * 8);
        }
        return TS_OK;
    }
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = stream ? (hipStream_t)stream : ix->stream;
    for (int32_t q : sel) {
        HIP_TRY(hipMemcpyAsync(out_scores + (size_t)q * k, s.data(), (size_t)k * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(out_idx + (size_t)q * k, i.data(), (size_t)k * 8, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));      // the two host rows are locals
    return TS_OK;
}

extern "C" int ts_search_rowsets(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                                 const ts_rowset* const* sets, int32_t nsets, const int32_t* which, float* out_scores, int64_t* out_idx,
                                 int out_on_device, void* stream, int algo, ts_rowsets_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (const char* bad = rowsets_args_invalid(queries, out_scores, out_idx, sets, which, q_dtype, nq, k, nsets, algo))
        return fail(TS_ERR_INVALID, "ts_search_rowsets (nq = %d, k = %d, nsets = %d): %s", nq, k, nsets, bad);
    std::vector<RowsetsSet> info((size_t)std::max(nsets, 1));
    for (int s = 0; s < nsets; ++s) {
        const ts_rowset* r = sets[s];
        info[(size_t)s] = r ? RowsetsSet{true, r->n, r->allowed, r->device} : RowsetsSet{false, 0, 0, 0};
    }
    if (const char* bad = rowsets_sets_invalid(info.data(), nsets, which, nq, ix != nullptr, ix ? ix->n : 0, ix ? ix->device : 0))
        return fail(TS_ERR_INVALID, "ts_search_rowsets (nq = %d, nsets = %d, index of %lld rows): %s", nq, nsets, (long long)(ix ? ix->n : 0), bad);
    if (ix->id_map) return fail(TS_ERR_UNSUPPORTED, "a row set per query on a subset index");
    if (nq == 0) return TS_OK;
    RowsetsIndex ri;
    ri.dtype = ix->dtype;
    ri.d = ix->d;
    ri.n = ix->n;
    ri.unpadded = ix->ld == ix->d;
    ri.two_level = two_level_search(ix);
    ri.f32_matrix = ix->knobs.get(K_MFMA_F32, 16) != 0;
    ri.mfma_min_rows = ix->knobs.get(K_MFMA_MIN_ROWS, 16384);
    ri.scan_max_knob = ix->knobs.get(K_SCAN_MAX_QUERIES, bias_scan_max_queries(ix->dtype));
    const RowsetsRoute route = rowsets_route(ri, info.data(), nsets, which, nq, k, algo);
    if (route.kind == kRowsetsUnsupported) return fail(TS_ERR_UNSUPPORTED, "%s", route.unsupported);
    if (stats) stats->sets_used = route.sets_used;
    if (route.kind == kRowsetsSearchEx || route.kind == kRowsetsSearchRowset) {
        const ts_rowset* one = route.kind == kRowsetsSearchRowset ? sets[route.one_set] : nullptr;
        ts_search_stats ss;
        TS_TRY(search_core(ix, queries, q_dtype, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream, algo, &ss,
                           one ? (const uint32_t*)one->mask : nullptr, one ? one->allowed : -1));
        if (stats) {
            stats->algo = ss.algo;
            stats->scan_queries = nq;
            stats->scan_calls = 1;
            stats->fallback_queries = ss.fallback_queries;
            stats->candidates = ss.candidates;
        }
        return TS_OK;
    }
    const size_t q_row_bytes = (size_t)ix->d * (q_dtype == TS_BF16 ? 2 : 4);
    if (stats) {
        stats->algo = route.pass.empty() ? TS_ALGO_SCAN : TS_ALGO_MFMA;
        stats->pass_queries = (int32_t)route.pass.size();
        stats->scan_queries = route.scan_queries();
        stats->scan_calls = route.scan_calls();
    }
    std::vector<int32_t> which_pass(route.pass.size());
    for (size_t j = 0; j < route.pass.size(); ++j) which_pass[j] = which[route.pass[j]];
    TS_TRY(rowsets_subset(ix, route.pass, queries, q_row_bytes, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream,
                          [&](const void* q, float* os, int64_t* oi) {
                              return rowsets_pass(ix, q, q_dtype, q_on_device, (int32_t)route.pass.size(), k, sets, which_pass.data(), os, oi,
                                                  out_on_device, stream, stats);
                          }));
    for (const RowsetsGroup& g : route.groups) {
        if (g.empty) {
            TS_TRY(rowsets_padding(ix, g.queries, k, out_scores, out_idx, out_on_device, stream));
            continue;
        }
        const ts_rowset* one = g.set >= 0 ? sets[g.set] : nullptr;
        TS_TRY(rowsets_subset(ix, g.queries, queries, q_row_bytes, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream,
                              [&](const void* q, float* os, int64_t* oi) {
                                  return search_core(ix, q, q_dtype, q_on_device, (int32_t)g.queries.size(), k, os, oi, out_on_device, stream,
                                                     route.group_algo, nullptr, one ? (const uint32_t*)one->mask : nullptr, one ? one->allowed : -1);
                              }));
    }
    return TS_OK;
}

// ---- ts_search_biased_rowsets: a weight and a row set per query (biased_rowsets_plan.h holds the rules) -----------------------
// one class of the call as the existing biased search runs it (ts_search_biased_rowset, or ts_search_biased_ex for set -1)
static int biased_class_search(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k, const float* bias,
                               int bias_on_device, float weight, const ts_rowset* rows, float* out_scores, float* out_sims, int64_t* out_idx,
                               int out_on_device, void* stream, int algo, ts_search_stats* stats) {
    BiasSpec b;
    b.bias = bias;
    b.on_device = bias_on_device;
    b.weight = weight;
    b.out_sims = out_sims;
    b.ex = true;
    return search_impl(ix, queries, q_dtype, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream, algo, stats,
                       rows ? (const uint32_t*)rows->mask : nullptr, rows ? 1 : 0, &b, rows ? rows->allowed : -1);
}

// out_sims of a split call, from its finished outputs: fmaf(-weights[q], bias[row], score) per entry (unbias_kernel's rule).  Host
// outputs go through device temporaries; the stream is drained before they are freed.
static int biased_rowsets_unbias(ts_index* ix, const float* dbias, const float* weights, int32_t nq, int32_t k, const float* out_scores,
                                 float* out_sims, const int64_t* out_idx, int out_on_device, hipStream_t st) {
    const size_t cnt = (size_t)nq * k;
    DevBuf tmp;             // weights [nq] | sims [cnt] | scores [cnt] | ids [cnt] (8-byte aligned: nq + 2 cnt floats padded to even)
    const size_t head = ((size_t)nq + 1) / 2 * 2;
    DEV_TRY(tmp.need((head + (out_on_device ? 0 : 2 * cnt + 2 * cnt)) * 4));
    float* dw = tmp.as<float>();
    int rc = TS_OK;
    auto enqueue = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(dw, weights, (size_t)nq * 4, hipMemcpyHostToDevice, st));
        if (out_on_device) return launch_unbias_rows(ix, out_scores, out_idx, dbias, dw, k, out_sims, (int64_t)cnt, st);
        float* dsims = dw + head;
        float* dscores = dsims + cnt;
        int64_t* didx = (int64_t*)(dscores + cnt);
        HIP_TRY(hipMemcpyAsync(dscores, out_scores, cnt * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(didx, out_idx, cnt * 8, hipMemcpyHostToDevice, st));
        TS_TRY(launch_unbias_rows(ix, dscores, didx, dbias, dw, k, dsims, (int64_t)cnt, st));
        HIP_TRY(hipMemcpyAsync(out_sims, dsims, cnt * 4, hipMemcpyDeviceToHost, st));
        return TS_OK;
    };
    rc = enqueue();
    const hipError_t e = hipStreamSynchronize(st);
    if (rc == TS_OK && e != hipSuccess) rc = fail(TS_ERR_HIP, "stream synchronize failed: %s", hipGetErrorString(e));
    return rc;
}

extern "C" int ts_search_biased_rowsets(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, int32_t k,
                                        const float* bias, int bias_on_device, const float* weights, const ts_rowset* const* sets,
                                        int32_t nsets, const int32_t* which, float* out_scores, float* out_sims, int64_t* out_idx,
                                        int out_on_device, void* stream, int algo, ts_rowsets_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (const char* bad = biased_rowsets_args_invalid(queries, out_scores, out_idx, sets, which, bias, weights, q_dtype, nq, k, nsets, algo))
        return fail(TS_ERR_INVALID, "ts_search_biased_rowsets (nq = %d, k = %d, nsets = %d): %s", nq, k, nsets, bad);
    std::vector<RowsetsSet> info((size_t)std::max(nsets, 1));
    for (int s = 0; s < nsets; ++s) {
        const ts_rowset* r = sets[s];
        info[(size_t)s] = r ? RowsetsSet{true, r->n, r->allowed, r->device} : RowsetsSet{false, 0, 0, 0};
    }
    if (const char* bad = rowsets_sets_invalid(info.data(), nsets, which, nq, ix != nullptr, ix ? ix->n : 0, ix ? ix->device : 0))
        return fail(TS_ERR_INVALID, "ts_search_biased_rowsets (nq = %d, nsets = %d, index of %lld rows): %s", nq, nsets, (long long)(ix ? ix->n : 0), bad);
    if (ix->id_map) return fail(TS_ERR_UNSUPPORTED, "ts_search_biased_rowsets: a weight and a row set per query on a subset index");
    if (nq == 0) return TS_OK;
    RowsetsIndex ri;
    ri.dtype = ix->dtype;
    ri.d = ix->d;
    ri.n = ix->n;
    ri.unpadded = ix->ld == ix->d;
    ri.two_level = two_level_search(ix);
    ri.f32_matrix = ix->knobs.get(K_MFMA_F32, 16) != 0;
    ri.mfma_min_rows = ix->knobs.get(K_MFMA_MIN_ROWS, 16384);
    ri.scan_max_knob = ix->knobs.get(K_SCAN_MAX_QUERIES, bias_scan_max_queries(ix->dtype));
    const BiasedRowsetsRoute route = biased_rowsets_route(ri, info.data(), nsets, which, weights, nq, k, algo);
    if (route.kind == kBiasedRowsetsUnsupported) return fail(TS_ERR_UNSUPPORTED, "%s", route.unsupported);
    if (stats) stats->sets_used = route.sets_used;
    if (route.kind == kBiasedRowsetsOneClass) {
        ts_search_stats ss;
        TS_TRY(biased_class_search(ix, queries, q_dtype, q_on_device, nq, k, bias, bias_on_device, route.one_weight,
                                   route.one_set >= 0 ? sets[route.one_set] : nullptr, out_scores, out_sims, out_idx, out_on_device, stream, algo, &ss));
        if (stats) {
            stats->algo = ss.algo;
            stats->scan_queries = nq;
            stats->scan_calls = 1;
            stats->fallback_queries = ss.fallback_queries;
            stats->candidates = ss.candidates;
        }
        return TS_OK;
    }
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = stream ? (hipStream_t)stream : ix->stream;
    // a host bias goes to the device once, for the pass and every per-class call (the call's own copy: the handle's belongs to the
    // searches below)
    DevBuf bias_copy;
    const float* dbias = bias;
    if (!bias_on_device) {
        DEV_TRY(bias_copy.need(std::max<size_t>((size_t)ix->n * 4, 4)));
        HIP_TRY(hipMemcpyAsync(bias_copy, bias, (size_t)ix->n * 4, hipMemcpyHostToDevice, st));
        dbias = bias_copy.as<const float>();
    }
    const size_t q_row_bytes = (size_t)ix->d * (q_dtype == TS_BF16 ? 2 : 4);
    if (stats) {
        stats->algo = route.pass.empty() ? TS_ALGO_SCAN : TS_ALGO_MFMA;
        stats->pass_queries = (int32_t)route.pass.size();
        stats->scan_queries = route.scan_queries();
        stats->scan_calls = route.scan_calls();
    }
    // from here on every path drains the stream before `bias_copy` is freed: failures are kept in rc
    auto run = [&]() -> int {
        std::vector<int32_t> which_pass(route.pass.size());
        std::vector<float> weights_pass(route.pass.size());
        for (size_t j = 0; j < route.pass.size(); ++j) {
            which_pass[j] = which[route.pass[j]];
            weights_pass[j] = weights[route.pass[j]];
        }
        TS_TRY(rowsets_subset(ix, route.pass, queries, q_row_bytes, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream,
                              [&](const void* q, float* os, int64_t* oi) {
                                  return rowsets_pass(ix, q, q_dtype, q_on_device, (int32_t)route.pass.size(), k, sets, which_pass.data(), os, oi,
                                                      out_on_device, stream, stats, dbias, weights_pass.data());
                              }));
        for (const BiasedRowsetsGroup& g : route.groups) {
            if (g.empty) {
                TS_TRY(rowsets_padding(ix, g.queries, k, out_scores, out_idx, out_on_device, stream));
                continue;
            }
            const ts_rowset* one = g.set >= 0 ? sets[g.set] : nullptr;
            TS_TRY(rowsets_subset(ix, g.queries, queries, q_row_bytes, q_on_device, nq, k, out_scores, out_idx, out_on_device, stream,
                                  [&](const void* q, float* os, int64_t* oi) {
                                      return biased_class_search(ix, q, q_dtype, q_on_device, (int32_t)g.queries.size(), k, dbias, 1, g.weight, one,
                                                                 os, nullptr, oi, out_on_device, stream, route.group_algo, nullptr);
                                  }));
        }
        if (out_sims) TS_TRY(biased_rowsets_unbias(ix, dbias, weights, nq, k, out_scores, out_sims, out_idx, out_on_device, st));
        return TS_OK;
    };
    int rc = run();
    if (!bias_on_device) {
        const hipError_t e = hipStreamSynchronize(st);
        if (rc == TS_OK && e != hipSuccess) rc = fail(TS_ERR_HIP, "stream synchronize failed: %s", hipGetErrorString(e));
    }
    return rc;
}

template <int DT, int CH, int G>
static int launch_rank_spec(int qb, int grid, hipStream_t st, const RankArgs& a) {
    if (qb == 4) rank_kernel<DT, CH, G, 4><<<grid, 256, 0, st>>>(a);
    else rank_kernel<DT, CH, G, 1><<<grid, 256, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    return TS_OK;
}

static int launch_rank(const ts_index* ix, const RankArgs& a, hipStream_t st, int grid) {
    return with_scan_width(ix, [&](auto dt, auto ch, auto g) {
        if constexpr (ch.value == 0) return launch_lds<rank_generic_kernel<dt.value>>(ix->device, grid, 256, rank_generic_lds(a.ld), st, a);
        else return launch_rank_spec<dt.value, ch.value, g.value>(a.nq >= 2 ? 4 : 1, grid, st, a);
    }, std::make_index_sequence<kScanWidths>{});
}

// target_rows != NULL: rank of that row (its score is computed by the kernel);  otherwise target_scores / target_ids:
// number of rows of THIS index that rank before a document with that score and global id (it may live on another shard).
static int rank_impl(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, const int64_t* target_rows,
                     const float* target_scores, const int64_t* target_ids, int64_t* out_rank, float* out_score, void* stream) {
    if (!ix || !queries || !out_rank) return fail(TS_ERR_INVALID, "NULL argument");
    if (q_dtype != TS_F32 && q_dtype != TS_BF16) return fail(TS_ERR_INVALID, "q_dtype %d", q_dtype);
    if (nq < 0) return fail(TS_ERR_INVALID, "nq = %d", nq);
    if (nq == 0) return TS_OK;
    if (ix->id_map) return fail(TS_ERR_UNSUPPORTED, "rank / count on a subset index");
    std::lock_guard<std::mutex> lock(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st;
    StreamScope scope;
    TS_TRY(enter_stream(ix, stream, &st, &scope));
    TS_TRY(ensure_search_scratch(ix, 1));
    constexpr size_t kPer = 8 + 8 + 4;
    DEV_TRY(ix->rank_buf.need((size_t)kQBlock * kPer));
    int64_t* d_target = ix->rank_buf.as<int64_t>();  // rows, or ready-made keys
    unsigned long long* d_counts = (unsigned long long*)(d_target + kQBlock);
    float* d_tscore = (float*)(d_counts + kQBlock);
    QueryFeed feed;
    TS_TRY(query_feed_open(&feed, ix, queries, q_dtype, q_on_device, nq, true, st));
    std::vector<int64_t> local(kQBlock);
    std::vector<unsigned long long> counts(kQBlock);
    std::vector<float> tscore(kQBlock);
    for (int q0 = 0; q0 < nq; q0 += kQBlock) {
        const int nb = std::min(kQBlock, nq - q0);
        TS_TRY(query_feed_block(feed, q0, nb));
        for (int i = 0; i < nb; ++i) {
            if (target_rows) {
                const int64_t r = target_rows[q0 + i] - ix->row_offset;
                local[i] = (r >= 0 && r < ix->n) ? r : -1;
            } else {
                local[i] = (int64_t)count_above_key(target_scores[q0 + i], target_ids[q0 + i] - ix->row_offset, ix->n);
            }
        }
        HIP_TRY(hipMemcpyAsync(d_target, local.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)nb * 8, st));
        RankArgs a;
        memset(&a, 0, sizeof(a));
        a.corpus = ix->rows;
        a.ld = ix->ld;
        a.n = ix->n;
        a.qbuf = ix->qf32;
        a.nq = nb;
        a.target = d_target;
        a.tkey = target_rows ? nullptr : (const u64*)d_target;
        a.counts = d_counts;
        a.tscore = d_tscore;
        hipEvent_t stop = prof_begin(ix, st, ix->n);
        const int rc = launch_rank(ix, a, st, ix->cu_count * kScanGridPerCU);
        prof_end(stop, st);
        TS_TRY(rc);
        HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
        if (target_rows) HIP_TRY(hipMemcpyAsync(tscore.data(), d_tscore, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));  // `local` is reused by the next block
        for (int i = 0; i < nb; ++i) {
            if (target_rows) {
                const bool ok = local[i] >= 0 && tscore[i] == tscore[i];
                out_rank[q0 + i] = ok ? (int64_t)counts[i] : -1;
                if (out_score) out_score[q0 + i] = tscore[i];
            } else {
                out_rank[q0 + i] = (target_scores[q0 + i] == target_scores[q0 + i]) ? (int64_t)counts[i] : -1;
            }
        }
    }
    return TS_OK;
}

extern "C" int ts_rank_of(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, const int64_t* target_rows,
                          int64_t* out_rank, float* out_score, void* stream) {
    if (!target_rows) return fail(TS_ERR_INVALID, "target_rows is NULL");
    return rank_impl(ix, queries, q_dtype, q_on_device, nq, target_rows, nullptr, nullptr, out_rank, out_score, stream);
}

extern "C" int ts_count_above(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, const float* target_scores,
                              const int64_t* target_ids, int64_t* out_counts, void* stream) {
    if (!target_scores || !target_ids) return fail(TS_ERR_INVALID, "NULL argument");
    return rank_impl(ix, queries, q_dtype, q_on_device, nq, nullptr, target_scores, target_ids, out_counts, nullptr, stream);
}

extern "C" int ts_scores(ts_index* ix, const void* queries, int q_dtype, int q_on_device, int32_t nq, float* out,
                         int out_on_device, void* stream) {
    if (!ix || !queries || !out) return fail(TS_ERR_INVALID, "NULL argument");
    if (q_dtype != TS_F32 && q_dtype != TS_BF16) return fail(TS_ERR_INVALID, "q_dtype %d", q_dtype);
    if (nq < 0) return fail(TS_ERR_INVALID, "nq = %d", nq);
    if (nq == 0 || ix->n == 0) return TS_OK;
    std::lock_guard<std::mutex> lock(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st;
    StreamScope scope;
    TS_TRY(enter_stream(ix, stream, &st, &scope));
    TS_TRY(ensure_search_scratch(ix, 1));
    float* dout = out;
    DevBuf tmp;
    if (!out_on_device) {
        // the score matrix is for the evaluation script's small shapes: refuse what cannot fit beside the index
        const size_t want = (size_t)nq * (size_t)ix->n * 4;
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        if (want > free_b / 2)
            return fail(TS_ERR_NOMEM, "score matrix of %d x %lld floats (%zu bytes) does not fit: use ts_search / ts_rank_of",
                        nq, (long long)ix->n, want);
        DEV_TRY(tmp.need(want));
        dout = tmp.as<float>();
    }
    QueryFeed feed;
    TS_TRY(query_feed_open(&feed, ix, queries, q_dtype, q_on_device, nq, true, st));
    // from here on every path drains the stream before `tmp` is freed: failures are kept in rc, not returned
    int rc = TS_OK;
    for (int q0 = 0; q0 < nq && rc == TS_OK; q0 += kQBlock) {
        const int nb = std::min(kQBlock, nq - q0);
        rc = query_feed_block(feed, q0, nb);
        if (rc != TS_OK) break;
        ScanArgs a;
        memset(&a, 0, sizeof(a));
        a.corpus = ix->rows;
        a.ld = ix->ld;
        a.n = ix->n;
        a.qbuf = ix->qf32;
        a.nq = nb;
        a.k = 1;
        a.scores = dout + (size_t)q0 * ix->n;
        rc = launch_scan<true>(ix, a, nb >= 2 ? 4 : 1, st, ix->cu_count * kScanGridPerCU);
    }
    if (!out_on_device) {
        if (rc == TS_OK && hipMemcpyAsync(out, dout, (size_t)nq * ix->n * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = fail(TS_ERR_HIP, "copy of the score matrix failed");
        if (hipStreamSynchronize(st) != hipSuccess && rc == TS_OK) rc = fail(TS_ERR_HIP, "stream synchronize failed");
    }
    return rc;
}

