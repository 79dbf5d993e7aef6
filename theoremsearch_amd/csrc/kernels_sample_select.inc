// The dense sample's threshold select (kernels_level.h), the text of its body: included inside sample_select_fast_kernel and
// sample_select_rowsets_kernel (kernels_rowsets.h), which define   THREADS (template parameter), a (LevelArgs), scores, row_stride
// and z_sel.  Text and not a function template for the reason kernels_mfma_anyd_pass.inc gives.
    constexpr int NW = THREADS / 64;
    constexpr int J4 = kLevelSortMax / (4 * THREADS);         // 8 float4 per thread cover 8192 positions
    __shared__ double red[2 * NW];
    __shared__ u32 wcount[2][NW];
    __shared__ __attribute__((aligned(16))) u32 surv[kSelCap];
    __shared__ __attribute__((aligned(16))) u64 best[kSelCap];
    __shared__ u32 nsurv;
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        a.count[q] = 0;                                       // the shared list of the full pass starts empty
        nsurv = 0;
    }
    const float4* src = (const float4*)(scores + (int64_t)q * row_stride);
    const int n4 = row_stride >> 2;                           // row_stride is a multiple of 64; positions past the sample hold -inf
    float v[4 * J4];
#pragma unroll
    for (int j = 0; j < J4; ++j) {
        const int i = j * THREADS + threadIdx.x;
        const float4 t = (i < n4) ? src[i] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
    }
    // live scores: not NaN, not -inf (no such row / filtered out).  From here on a score is its ordered 32-bit image
    // (0 = dead; every live score's image is above 0).
    double s1 = 0.0, s2 = 0.0;
    u32 nl = 0;
    u32 o[4 * J4];
#pragma unroll
    for (int e = 0; e < 4 * J4; ++e) {
        const bool live = v[e] == v[e] && v[e] > -INFINITY;
        const double d = live ? (double)v[e] : 0.0;
        s1 += d;
        s2 += d * d;
        nl += (u32)__popcll(__ballot(live));                  // wave-uniform: this wave's live count so far
        o[e] = live ? ord_f32(v[e]) : 0u;
    }
    s1 = wave_total_f64(s1);
    s2 = wave_total_f64(s2);
    if (lane == 0) { red[2 * wave] = s1; red[2 * wave + 1] = s2; wcount[0][wave] = nl; }
    __syncthreads();
    double t1 = 0.0, t2 = 0.0;
    int cnt = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { t1 += red[2 * w]; t2 += red[2 * w + 1]; cnt += (int)wcount[0][w]; }
    const double mean = cnt > 0 ? t1 / cnt : 0.0;
    const double sd = cnt > 0 ? sqrt(fmax(t2 / cnt - mean * mean, 0.0)) : 0.0;
    const int kk = a.kk;
    constexpr int kTailM = 32;
    const bool tail_fit = a.tail_p > 0.0f;
    const int kl = min(tail_fit ? max(kk, kTailM) : kk, kMaxK);

    // survivors of a cut (>= cut, cut >= 1), counted over the workgroup (uniform result); the two count buffers alternate,
    // so one barrier per call is enough
    int flip = 1;
    auto count_ge = [&](u32 cut) __attribute__((always_inline)) -> u32 {
        u32 c = 0;
#pragma unroll
        for (int e = 0; e < 4 * J4; ++e) c += (u32)__popcll(__ballot(o[e] >= cut));
        if (lane == 0) wcount[flip][wave] = c;
        __syncthreads();
        u32 tot = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) tot += wcount[flip][w];
        flip ^= 1;
        return tot;
    };
    const u32 want = (u32)min(kl, cnt);                       // fewer live rows than kl: all of them
    u32 cut = 1u, c = 0;
    bool found = want == 0;
    if (!found && sd > 0.0) {
        float z = z_sel;
        for (int t = 0; t < 3 && !found; ++t) {
            cut = max(ord_f32((float)(mean + (double)z * sd)), 1u);
            c = count_ge(cut);
            if (c < want) z -= 0.75f;
            else if (c > (u32)kSelCap) z += 0.75f;
            else found = true;
        }
    }
    if (!found) {
        // exact: the largest cut that still leaves `want` survivors = the want-th best score itself; everything above it
        // (fewer than want <= 256 values) plus copies of it are the want best scores
        u32 lo = 1u, hi = 0xFFFFFFFFu;                        // count_ge(lo) >= want always; hi may fail
        if (count_ge(hi) >= want) lo = hi;
        while (lo < hi) {                                     // invariant: count_ge(lo) >= want, count_ge(hi + 1) < want
            const u32 mid = lo + (hi - lo) / 2u + ((hi - lo) & 1u);
            if (count_ge(mid) >= want) lo = mid;
            else hi = mid - 1u;
        }
        cut = lo;
        c = count_ge(cut);
    }
    // gather the survivors (order does not matter; equal scores beyond the capacity are the cut itself and are padded back)
    const bool over = c > (u32)kSelCap;                       // only after the exact search: a pile of scores equal to the cut
    const u32 take_cut = (over && cut != 0xFFFFFFFFu) ? cut + 1u : cut;   // then take what lies strictly above and pad with the cut
    const bool take_any = want > 0 && !(over && cut == 0xFFFFFFFFu);
#pragma unroll
    for (int e = 0; e < 4 * J4; ++e) {
        const bool in = take_any && o[e] >= take_cut;
        const u64 m = __ballot(in);
        if (m) {
            u32 base = 0;
            if (lane == 0) base = atomicAdd(&nsurv, (u32)__popcll(m));
            base = (u32)__builtin_amdgcn_readfirstlane((int)base);
            const u32 at = base + (u32)__popcll(m & ((1ull << lane) - 1ull));
            if (in && at < (u32)kSelCap) surv[at] = o[e];
        }
    }
    __syncthreads();
    const int ns = (int)min(nsurv, (u32)kSelCap);
    const int m = over ? max(ns, (int)want) : ns;             // `over`: surv[ns .. want) are copies of the cut (not stored)
    // sorted scores as keys (score << 32), entries past the survivors 0 = empty, as level_threshold expects (it reads up
    // to best[kl - 1])
    if (m <= THREADS) {
        // rank sort: thread t owns survivor t and counts the survivors that come before it - m broadcast reads of LDS and
        // two instructions each, no exchange network
        const u32 mine = (int)threadIdx.x < ns ? surv[threadIdx.x] : cut;
        int rank = 0;
        const uint4* s4 = (const uint4*)surv;                 // four survivors per read (entries past ns are not counted)
#pragma unroll 2
        for (int i = 0; i < ns; i += 4) {
            const uint4 x = s4[i >> 2];
            rank += (x.x > mine || (x.x == mine && i < (int)threadIdx.x)) ? 1 : 0;
            rank += (i + 1 < ns && (x.y > mine || (x.y == mine && i + 1 < (int)threadIdx.x))) ? 1 : 0;
            rank += (i + 2 < ns && (x.z > mine || (x.z == mine && i + 2 < (int)threadIdx.x))) ? 1 : 0;
            rank += (i + 3 < ns && (x.w > mine || (x.w == mine && i + 3 < (int)threadIdx.x))) ? 1 : 0;
        }
        if ((int)threadIdx.x >= ns) rank = (int)threadIdx.x;  // the padding (copies of the cut, below every survivor) and the empty tail
        best[rank] = (int)threadIdx.x < m ? ((u64)mine << 32) : 0ull;
    } else {
        for (int i = threadIdx.x; i < kSelCap; i += THREADS) best[i] = (i < ns) ? ((u64)surv[i] << 32) : (i < m ? ((u64)cut << 32) : 0ull);
        int P = 2;
        while (P < m) P <<= 1;
        bitonic_sort_desc(best, P, threadIdx.x, THREADS);
    }
    __syncthreads();
    if (wave != 0) return;
    const float thr = level_threshold(a, best, cnt, kk, tail_fit, mean, sd);
    if (lane == 0) a.thr[q] = thr;
