// The int8 screen of the fp32 full pass (TS_MFMA_SCREEN_F32; d = 768 and 1024): what differs from the bf16 screen - the two
// quantisers, which read fp32 values and apply the range rule, and the exact rescore on v_mfma_f32_16x16x4_f32.  The image, the
// tile and query scalars, the fold, the integer thresholds and the tile kernel are those of kernels_screen8.h /
// kernels_screen8_tile.h, whose head also has the derivation ("fp32 rows").
#pragma once
#include "kernels_screen8.h"

namespace ts {

// The range rule (kernels_screen8.h, "fp32 rows"): a tile whose largest finite magnitude a_t is neither 0 nor inside
// [2^-100, 2^64], and a query whose a_q is neither 0 nor inside [2^-40, 2^40], admit everything (1 / s = NaN: threshold INT_MIN).
constexpr float kScreenF32TileMin = 0x1p-100f, kScreenF32TileMax = 0x1p64f;
constexpr float kScreenF32QueryMin = 0x1p-40f, kScreenF32QueryMax = 0x1p40f;
// ... and the absolute term of E_t that covers an underflow in any of the W terms of the chain, for every query in range:
// W 2^-126 (1 + a_q + a_t) / |q| <= W 2^-85 (1 + a_t)
template <int W> constexpr double kScreenF32Floor = (double)W * 0x1p-85;

__device__ __forceinline__ bool screen_f32_in_range(float amax, float lo, float hi) { return amax == 0.0f || (amax >= lo && amax <= hi); }

// quantize_tiles_kernel<W> over fp32 rows: the same image and meta layout, the tile scalars in fp64 and rounded up, E_t with
// the underflow term, and the range rule.  One workgroup (4 waves) per tile: wave w quantises rows 8 w .. 8 w + 7, lane l
// elements l + 64 j of a row.
template <int W>
__global__ void __launch_bounds__(256) quantize_tiles_f32_kernel(const float* __restrict__ rows, signed char* __restrict__ img,
                                                                 float4* __restrict__ meta, int64_t tile0) {
    static_assert(screen_width(W), "widths the int8 screen serves");
    __shared__ float red_max[4];
    __shared__ int red_bad[4];
    __shared__ double red_e[4], red_x[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = tile0 + blockIdx.x;
    const float* src = rows + t * kTileRows * W;
    float amax = 0.0f;
    int bad = 0;
    for (int r = 8 * wave; r < 8 * wave + 8; ++r)
        for (int j = 0; j < W / 64; ++j) {
            const float x = src[r * W + lane + 64 * j];
            if (!(fabsf(x) <= 3.4028235e38f)) bad = 1;
            else amax = fmaxf(amax, fabsf(x));
        }
    for (int o = 32; o > 0; o >>= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, o));
        bad |= __shfl_xor(bad, o);
    }
    if (lane == 0) { red_max[wave] = amax; red_bad[wave] = bad; }
    __syncthreads();
    amax = fmaxf(fmaxf(red_max[0], red_max[1]), fmaxf(red_max[2], red_max[3]));
    bad = red_bad[0] | red_bad[1] | red_bad[2] | red_bad[3];
    if (!screen_f32_in_range(amax, kScreenF32TileMin, kScreenF32TileMax)) bad = 1;
    const float s = (amax > 0.0f && !bad) ? amax / 127.0f : 1.0f;
    double emax = 0.0, xmax = 0.0;
    for (int r = 8 * wave; r < 8 * wave + 8; ++r) {
        double ee = 0.0, xx = 0.0;
        for (int j = 0; j < W / 64; ++j) {
            const int c = lane + 64 * j;
            const float x = src[r * W + c];
            float qx = 0.0f;
            if (fabsf(x) <= 3.4028235e38f) qx = fminf(127.0f, fmaxf(-127.0f, rintf(x / s)));
            img[(t * kTileRows + r) * W + c] = (signed char)(int)qx;
            const double sx = (double)s * (double)qx;
            const double e = (double)x - sx;
            ee += e * e;
            xx += sx * sx;
        }
        ee = wave_sum_f64(ee);
        xx = wave_sum_f64(xx);
        emax = fmax(emax, sqrt(ee));
        xmax = fmax(xmax, sqrt(xx));
    }
    if (lane == 0) { red_e[wave] = emax; red_x[wave] = xmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (bad) {          // a non-finite value or out of range: every pair of the tile is a candidate (the scalars are not read behind a NaN)
            meta[t] = make_float4(__builtin_nanf(""), 0.0f, 0.0f, 0.0f);
        } else {
            emax = fmax(fmax(red_e[0], red_e[1]), fmax(red_e[2], red_e[3])) * (1.0 + 0x1p-40);
            xmax = fmax(fmax(red_x[0], red_x[1]), fmax(red_x[2], red_x[3])) * (1.0 + 0x1p-40);
            const double et = emax + (double)kScreenGamma<W> * (xmax + emax) * (1.0 + 0x1p-20) + kScreenF32Floor<W> * (1.0 + (double)amax);
            meta[t] = make_float4(1.0f / s, f32_up(et), f32_up(xmax), 0.0f);
        }
    }
}

// screen_quantize_query<W> over fp32 queries, as a launch of its own: one wave per query slot of the launch (256 workgroups).
// Row r of q [nrows x W] fp32 -> row r of img [256 x W] int8 and meta[r] = {1 / s_q (NaN: a non-finite value, or out of range),
// |e_q|, |q|, 0}; a zero row past nrows.  Also empties the query's list of screened rows.
template <int W>
__global__ void __launch_bounds__(64) quantize_queries_f32_kernel(const float* __restrict__ q, int nrows, signed char* __restrict__ img,
                                                                  float4* __restrict__ meta, u32* __restrict__ scount) {
    static_assert(screen_width(W), "widths the int8 screen serves");
    const int r = blockIdx.x, lane = threadIdx.x;
    float v[W / 64];
    float amax = 0.0f;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < W / 64; ++j) {
        v[j] = r < nrows ? q[(int64_t)r * W + lane + 64 * j] : 0.0f;
        if (!(fabsf(v[j]) <= 3.4028235e38f)) bad = 1;
        else amax = fmaxf(amax, fabsf(v[j]));
    }
    for (int o = 32; o > 0; o >>= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, o));
        bad |= __shfl_xor(bad, o);
    }
    if (!screen_f32_in_range(amax, kScreenF32QueryMin, kScreenF32QueryMax)) bad = 1;
    const float s = (amax > 0.0f && !bad) ? amax / 127.0f : 1.0f;
    double ee = 0.0, qq = 0.0;
#pragma unroll
    for (int j = 0; j < W / 64; ++j) {
        float qx = 0.0f;
        if (fabsf(v[j]) <= 3.4028235e38f) qx = fminf(127.0f, fmaxf(-127.0f, rintf(v[j] / s)));
        img[(int64_t)r * W + lane + 64 * j] = (signed char)(int)qx;
        const double e = (double)v[j] - (double)s * (double)qx;
        ee += e * e;
        qq += (double)v[j] * (double)v[j];
    }
    ee = wave_sum_f64(ee);
    qq = wave_sum_f64(qq);
    if (lane == 0) {
        if (bad) meta[r] = make_float4(__builtin_nanf(""), 0.0f, 0.0f, 0.0f);
        else meta[r] = make_float4(1.0f / s, f32_up(sqrt(ee) * (1.0 + 0x1p-40)), f32_up(sqrt(qq) * (1.0 + 0x1p-40)), 0.0f);
        scount[r] = 0;
    }
}

// Exact rescore of the screen's pairs on an fp32 index: screen_rescore_kernel's workgroup and chunk scheme (workgroup (q, y), its
// four waves take chunks of 16 of query q's screened rows in turn) with the fp32 pass's arithmetic.  A chunk is the A operand of
// W / 4 v_mfma_f32_16x16x4_f32 from a zero accumulator: k-steps ascending, MFMA i = 0 .. 3 inside each - float i of the 16-byte
// chunk at floats 16 ks + 4 (lane >> 4) of row (lane & 15) times float i of the query's chunk at the same place, the operands
// and lanes of TS16_MMAF (kernels_mfma16.h).  There the four MFMAs of a k-step go to the wave's accumulators in turn (i-major:
// with NB = 2 the other query block's MFMA sits between two of one accumulator), which changes which accumulator is next, never
// the order within one: accumulator (row block, query block) takes (ks, i) in ascending order at NB = 1 and NB = 2 alike, so a
// row's chain - and with it every score bit - is this one, whichever launch of the unscreened pass would have held the query.
// The query sits in all sixteen columns of B (a column of D depends on its own column of B only) and the score is read from
// column q & 15, as in the bf16 rescore.
// Registers: the query's W / 4 floats per lane are pinned in AGPRs (192 or 256: the B operand may come from there, as in the
// pass); a row would be as many again, so its chunks stream through a ring of kRescoreRing k-steps in VGPRs - chunk ks + kRescoreRing
// is asked for behind the MFMAs of k-step ks, into the registers they have just read.
struct ScreenRescoreF32Args {
    const float* rows;            // fp32 [n_pad x W]
    const float* q;               // fp32 queries [>= nq x W], as the pass multiplies them
    const float* thr;             // [nq]
    const u64* scand;             // [256][kScreenCap] screened rows
    const u32* scount;            // [256]
    u64* cand;                    // [256][cap] the final select's lists
    u32* count;                   // [256]
    int cap;
};

// (a row's chunks are read through a pointer spelled as a global-memory pointer: it passes through an empty asm statement that
// pins where the next chunk is asked for, behind which hipcc no longer sees that it came from a kernel argument and would fall
// back to flat loads, which count in both wait queues and return in no order hipcc can count on)
typedef const __attribute__((address_space(1))) f32x4* rescore_row_gptr;
constexpr int kRescoreRing = 16;  // k-steps of a row in flight: 16 x 64 bytes per lane quarter = 1 KB of every row of the chunk

template <int W>
__global__ void __launch_bounds__(256) screen_rescore_f32_kernel(ScreenRescoreF32Args a) {
    static_assert(screen_width(W), "widths the int8 screen serves");
    constexpr int kSteps = W / 16;                        // 16-byte chunks per lane and row: 48 or 64
    static_assert(kSteps % kRescoreRing == 0 && kSteps * 64 <= 4096, "ring slots by k-step, and every chunk within the load's immediate offset");
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 raw = a.scount[q];
    if (raw > (u32)kScreenCap) {
        if (blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(&a.count[q], (u32)a.cap + 1u);
        return;
    }
    const int m = (int)raw;
    const int nchunks = (m + 15) >> 4;
    int c = blockIdx.y * 4 + wave;
    if (c >= nchunks) return;
    const int r16 = lane & 15, kq = lane >> 4;
    auto entry = [&](int cc) { const int e = 16 * cc + r16; return e < m ? (u32)a.scand[(int64_t)q * kScreenCap + e] : 0u; };
    u32 row = entry(c);
    rescore_row_gptr pr = (rescore_row_gptr)(a.rows + (int64_t)row * W + 4 * kq);
    f32x4 ring[kRescoreRing];
#pragma unroll
    for (int j = 0; j < kRescoreRing; ++j) ring[j] = pr[4 * j];
    const float thr = a.thr[q];
    f32x4 qf[kSteps];
    const f32x4* pq = (const f32x4*)(a.q + (int64_t)q * W + 4 * kq);
#pragma unroll
    for (int ks = 0; ks < kSteps; ++ks) qf[ks] = pq[4 * ks];
#pragma unroll
    for (int ks = 0; ks < kSteps; ++ks) asm volatile("" : "+a"(qf[ks]));
    for (bool first = true; c < nchunks; c += gridDim.y * 4, first = false) {
        if (!first) {
            row = entry(c);
            pr = (rescore_row_gptr)(a.rows + (int64_t)row * W + 4 * kq);
#pragma unroll
            for (int j = 0; j < kRescoreRing; ++j) ring[j] = pr[4 * j];
        }
        f32x4 acc;
#pragma unroll
        for (int ks = 0; ks < kSteps; ++ks) {
            const f32x4 av = ring[ks % kRescoreRing];
            if (ks == 0) mfma16f_a_first(acc, av[0], qf[ks][0]);
            else mfma16f_a(acc, av[0], qf[ks][0]);
            mfma16f_a(acc, av[1], qf[ks][1]);
            mfma16f_a(acc, av[2], qf[ks][2]);
            mfma16f_a(acc, av[3], qf[ks][3]);
            if (ks + kRescoreRing < kSteps) {
                asm volatile("" : "+v"(pr));              // the next chunk is asked for here, behind this k-step's MFMAs, not earlier
                ring[ks % kRescoreRing] = pr[4 * (ks + kRescoreRing)];
            }
        }
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc));   // wait states: MFMA result -> VALU reader
        u32 rr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) rr[i] = (u32)__shfl((int)row, 4 * kq + i);
        if (r16 == (q & 15)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float s = acc[i];
                if (16 * c + 4 * kq + i < m && s >= thr) {
                    const u32 pos = atomicAdd(&a.count[q], 1u);
                    if (pos < (u32)a.cap) a.cand[(int64_t)q * a.cap + pos] = make_key(s, rr[i]);
                }
            }
        }
    }
}

}  // namespace ts
