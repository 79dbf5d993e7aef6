// The matrix path's level select (kernels_level.h), the text of its body: included inside level_select_kernel and
// level_select_rowsets_kernel (kernels_rowsets.h), which define   KR (template parameter) and a (LevelArgs).  Text and not a
// function template for the reason kernels_mfma_anyd_pass.inc gives.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SelectLds lds = SelectLds::carve(smem, kLevelSortMax);
    const int q = blockIdx.x;
    if (level_final_one_wave(a, q)) return;
    u32& fill = lds.ctr[kSelFill];
    u32& produced = lds.ctr[kSelProduced];
    u32& base_shared = lds.ctr[kSelSharedBase];
    if (threadIdx.x == 0) {
        fill = 0;
        produced = 0;
        lds.ctr[kSelShort] = 0;
    }
    for (int i = threadIdx.x; i < kLevelBins; i += blockDim.x) lds.hist[i] = 0;
    __syncthreads();
    // The gather (inline: as a function it moves this kernel's instructions - profiles/HISTORY.md): the private lists
    // (a writer's entries are loaded together: one round trip, not one per entry) ...
    for (int w = threadIdx.x; w < a.nwriters; w += blockDim.x) {
        const u32 made = a.pcount[(int64_t)q * a.nwriters + w];
        if (made == 0) continue;
        const u32 n = min(made, (u32)a.priv_cap);
        const u64* src = a.priv + ((int64_t)q * a.nwriters + w) * a.priv_cap;
        const u32 at = atomicAdd(&fill, n);
        atomicAdd(&produced, n);
        u64 v[32];
#pragma unroll
        for (int e = 0; e < 32; ++e) v[e] = ((u32)e < n) ? src[e] : 0ull;
#pragma unroll
        for (int e = 0; e < 32; ++e)
            if ((u32)e < n && at + e < (u32)kLevelSortMax) lds.keys[at + e] = v[e];
    }
    // ... and the shared spill list
    const u32 raw = a.count[q];
    const u32 ns = min(raw, (u32)a.cap);
    __syncthreads();
    if (threadIdx.x == 0) {
        base_shared = fill;
        fill += ns;
        produced += raw;
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < ns; i += blockDim.x)
        if (base_shared + i < (u32)kLevelSortMax) lds.keys[base_shared + i] = a.cand[(int64_t)q * a.cap + i];
    __syncthreads();
    const u32 total = fill;
    const bool lost = raw > (u32)a.cap || total > (u32)kLevelSortMax;
    const int cnt = (int)min(total, (u32)kLevelSortMax);
    const int kk = a.kk;
    // the sample level of the estimated threshold also needs the sample's 32 best for the tail fit
    constexpr int kTailM = 32;
    const bool tail_fit = !a.final_level && a.tail_p > 0.0f;
    const int kl = tail_fit ? max(kk, kTailM) : kk;  // entries wanted, sorted

    // mean / sd of the gathered scores (the histogram's range, and the Gaussian-tail estimate of the sample level) and the
    // kl best keys, sorted
    double mean = 0.0, sd = 0.0;
    u64* best = lds_select_top<KR>(lds, cnt, kl, !a.final_level && a.z_tail > 0.0f && cnt >= 256, mean, sd);

    if (threadIdx.x == 0) a.count[q] = 0;
    if (!a.final_level) {
        const float thr = level_threshold(a, best, cnt, kk, tail_fit, mean, sd);
        if (threadIdx.x == 0) a.thr[q] = thr;
        return;
    }
    if (threadIdx.x == 0) a.stat_q[q] = produced;
    if (lost || (int)total < a.min_fill) {
        if (threadIdx.x == 0) a.fb_list[atomicAdd(a.fb_count, 1)] = q;
        return;
    }
    for (int i = threadIdx.x; i < a.k_user; i += blockDim.x) {     // (write_result_slot here moves this kernel's instructions)
        const u64 key = best[i];
        a.out_scores[(int64_t)q * a.k_user + i] = key ? key_score(key) : -INFINITY;
        a.out_idx[(int64_t)q * a.k_user + i] = !key ? -1 : a.id_map ? a.id_map[key_row(key)] : (int64_t)key_row(key) + a.row_offset;
    }
