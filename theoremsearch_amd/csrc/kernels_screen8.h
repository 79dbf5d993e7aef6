// The int8 screen of the d = 768 bf16 full pass - and, opt-in (TS_MFMA_SCREEN_WIDE), of the d = 1024 one - (DESIGN.md section
// 3.2): every (row, query) pair is first scored with
// v_mfma_i32_16x16x64_i8 on an int8 image of the corpus (half the bytes, half the matrix cycles of the bf16 pass), and only
// the pairs whose certified upper bound reaches the query's threshold are rescored exactly, from the bf16 rows, with the
// MFMA chain of the bf16 pass.  The pass still only has to guarantee that no row with exact score >= thr is dropped
// (the "estimate, then verify" protocol of search_mfma.hip): the answers are bit for bit those of the unscreened pass.
//
// Quantisation (tile t = 32 rows, one scale; query q, one scale):
//   s_t = max |x| / 127 over the tile, x~ = rint(x / s_t) in [-127, 127], e_x = x - s_t x~   (x = the stored bf16 values)
//   s_q = max |q| / 127,               q~ = rint(q / s_q),                 e_q = q - s_q q~
// so  x.q = s_t s_q (x~.q~) + s_t x~.e_q + e_x.q  and  |x.q - s_t s_q (x~.q~)| <= |s_t x~| |e_q| + |e_x| |q|.
// The fp32 score S of the bf16 pass (exact bf16 products, 768 fp32 additions) is within g = 768 2^-22 |x| |q| of x.q
// (four times the classic (n - 1) u bound on |x| |q| >= sum |x_i q_i|), and |x| <= |s_t x~| + |e_x|.  Hence
//   S >= thr  =>  x~.q~ >= (thr - E_t |q| - X_t |e_q|) / (s_t s_q),   E_t = max|e_x| + 768 2^-22 (X_t + max|e_x|), X_t = max|s_t x~|
// over the rows of the tile.  The tile scalars are computed in fp64 and rounded up (tx = 1 / s_t, ty = E_t, tz = X_t).
//
// The integer threshold (kernels_screen8_tile.h) takes a relative slack of 2^-18 of M = athr + ty qn + tz eq (athr = |thr|, 0 where
// thr is infinite; qn = |q|, eq = |e_q|, rq = 1 / s_q) and one more unit:
//   floor(tx (thr - athr 2^-18 - (ty qn + tz eq)(1 + 2^-18)) rq - 1) = floor(tx (Q1 - ty Q2 - tz Q3) - 1)
// with the query's side folded once per launch (screen_fold_query): Q1 = rq (thr - athr 2^-18), Q2 = rq qn (1 + 2^-18),
// Q3 = rq eq (1 + 2^-18), in fp64 and rounded to fp32 on the admitting side (Q1 down, Q2 and Q3 up).  Per (tile, query) there
// are three fp32 FMAs, fma(-ty, Q2, Q1), fma(-tz, Q3, .), fma(tx, ., -1), each rounded to nearest.  Every operand and partial
// result of the first two is bounded by R = rq M (1 + 2^-17), so each of them is off by at most 2^-24 R; the third adds at most
// 2^-24 (tx R + 1).  Together with the fp32 reciprocals tx and rq (2^-24 each, relative) that is below 6 2^-24 tx R + 2^-24,
// against the slack 2^-18 tx R = 64 2^-24 tx R plus the unit: the computed value stays below the certified bound, and floor
// keeps it there.  (The replaced order, (thr - sub - (athr + sub) 2^-18) tx rq - 1 with sub in fp32, rounded about as often;
// its thresholds and the folded ones differ by at most one unit - tests/test_screen8_fold_cpu.py.)
//
// d = 1024 (W = the screen's width, a template parameter of everything below; the text above reads with 768 -> W):
//   * the i32 accumulator: |x~.q~| <= 1024 127^2 = 16,516,096 < 2^24, far inside i32 (and every partial sum with it), so the
//     integer dot product is exact at either width, whatever order the instruction adds the bytes in;
//   * the summation term: the bf16 products are exact in fp32, and a sum of n fp32 terms added in ANY order (a chain, two
//     half-chains added, the instruction's own tree inside a k-step) is within gamma_(n-1) sum |x_i q_i| of the exact sum,
//     gamma_(n-1) = (n - 1) u / (1 - (n - 1) u) with u = 2^-24: 1023 2^-24 (1 + 2^-14) at n = 1024.  g = 1024 2^-22 is four
//     times that, the same factor as at 768 (it covers a matrix pipe that does not round every addition to nearest);
//   * both forms of the d = 1024 pass are such sums of the same 1024 products - the plain form one chain of 32 k-steps from a
//     zero accumulator, the k-split form two chains of 16 k-steps (k-steps 8 u + 4 h .. 8 u + 4 h + 3 of every unit u, h = 0, 1)
//     added once - so the one bound holds for the score of either, and the rescore below reproduces whichever the call's
//     unscreened pass would have computed (KSPLIT);
//   * nothing else in the derivation knows the width: the tile and query scalars are norms in fp64, the fold and its rounding
//     argument are per (tile, query).
//
// A tile with a NaN / Inf value, or a query with one, has threshold INT_MIN (tx or rq is NaN; the clamp's maxNum turns the NaN
// into -2^31): all of its pairs are candidates and the exact rescore treats them as the bf16 pass does (a NaN score is never a
// candidate).  An infinite thr gives 2^30 (+inf: nothing passes) or INT_MIN (-inf: everything does).
//
// fp32 rows (TS_MFMA_SCREEN_F32; d = 768 and 1024; the quantisers and the rescore are in kernels_screen8_f32.h).  The image, the
// scalars' layout, the fold, the integer threshold and the tile kernel are the ones above; three things differ.
//   * Stored values.  x and q are the stored fp32 values: e_x = x - s_t x~ and e_q = q - s_q q~ are measured against them (in
//     fp64, whatever the fp32 division and rint made of x~), so the decomposition of x.q above holds as it stands.
//   * Score arithmetic.  The fp32 pass does not add exact products: its score S is a chain of W fused multiply-adds from a zero
//     accumulator, S = fma(x_k q_k, S) over k in the kernel's fixed permutation k = 16 s + 4 (lane >> 4) + i (k-step s
//     ascending, then MFMA i = 0 .. 3 of v_mfma_f32_16x16x4_f32, then the four lane groups inside one instruction), with ONE
//     rounding per term.  Term j of the chain passes through at most W - j + 1 roundings, so, u = 2^-24,
//       |S - x.q| <= gamma_W sum |x_k q_k| <= gamma_W |x| |q|,  gamma_W = W u / (1 - W u) <= W 2^-24 (1 + 2^-13)  (W <= 1024)
//     in any order of the terms - one rounding more per term than the bf16 pass, whose products are exact.  g = W 2^-22 is
//     4 (1 - W u) gamma_W: still four times the bound (less 2^-14 of it), the factor that covers a matrix pipe that does not
//     round every addition to nearest.  kScreenGamma<W> stays as it is.
//   * Range.  fp32 values are not pre-shrunk by a bf16 rounding and span 2^-149 .. 2^128.  With a_t = the largest magnitude of a
//     tile and a_q = that of a query:
//       - Overflow.  Every partial sum of the chain is at most W a_t a_q (1 + gamma_W).  Past 2^128 the chain gives +-Inf or NaN
//         where x.q is finite, and the inequality above says nothing.
//       - Underflow.  A product, a partial sum or an operand below 2^-126 is rounded to a multiple of 2^-149 or, in a flushing
//         mode, to zero: per term an absolute error of at most 2^-126 (the result), 2^-126 a_q (an x_k taken as zero) or
//         2^-126 a_t (a q_k), which gamma_W's relative model does not contain: U = W 2^-126 (1 + a_q + a_t) in all.
//       - The scalars.  s_t = a_t / 127 and s_q = a_q / 127 must be normal fp32 numbers with finite reciprocals, and the three
//         FMAs of the threshold must stay clear of underflow themselves: their rounding argument above (2^-24 R per operation)
//         holds while 2^-24 R is far above 2^-126.
//     The rule, decided in the quantisers (the tile loop only ever sees a NaN scalar): a tile is IN RANGE when a_t = 0 or
//     2^-100 <= a_t <= 2^64, a query when a_q = 0 or 2^-40 <= a_q <= 2^40.  Every other tile and every other query gets
//     1 / s = NaN, like a tile or query with a NaN / Inf value: threshold INT_MIN, all of its pairs are candidates and the exact
//     rescore decides.  For a pair of an in-range tile and an in-range query:
//       - W a_t a_q (1 + gamma_W) <= 2^10 2^64 2^40 (1 + 2^-13) < 2^115: nothing in the chain overflows;
//       - |q| >= a_q >= 2^-40 (a zero query has S = 0 = x.q exactly), so U <= |q| W 2^-126 (2^40 + 1 + 2^40 a_t)
//         <= |q| W 2^-85 (1 + a_t): the tile adds that to its coefficient of |q|,
//           E_t = max|e_x| + g (X_t + max|e_x|) + W 2^-85 (1 + a_t)
//         (relative to a_t it is 2^-63 of g: it only shows where the tile is tiny), and S >= thr  =>  x~.q~ >= ... as above;
//       - 127 2^-64 <= 1 / s_t <= 127 2^100 and 127 2^-40 <= 1 / s_q <= 127 2^40: normal, finite (a zero tile or query has s = 1);
//         X_t <= 33 a_t and |q| <= 32 a_q are finite, the fp64 sums of squares are far inside fp64;
//       - R >= Q2 ty >= 127 W 2^-85 > 2^-69 (Q2 = rq |q| (1 + 2^-18) >= 127, ty = E_t >= W 2^-85), so 2^-24 R > 2^-93: an
//         underflow inside the three FMAs (at most 2^-126 each, e.g. tz Q3 with a tiny |e_q|) is 2^-33 of one rounding.  Q1 may
//         overflow fp32 for a huge thr: rounded down it is FLT_MAX or -Inf, both on the admitting side; tx (...) may overflow
//         too: -Inf admits everything, +Inf only arises where the certified bound is itself beyond any integer dot product.
#pragma once
#include "kernels_mfma16.h"

namespace ts {

// widths the screen serves: one int8 row has the bytes of a d = W / 2 bf16 row (384: the d = 768 index; 512: d = 1024)
constexpr bool screen_width(int w) { return w == 768 || w == 1024; }
constexpr int kScreenCap = kScreenListCap;   // screen candidates per query (~490 expected on Gaussian rows at 10M; 8 x the exact lists; more = exact re-run)
template <int W> constexpr float kScreenGamma = (float)W * 0x1p-22f;   // bound of the bf16 pass's fp32 summation, relative to |x| |q|

// One workgroup (4 waves) per tile: wave w quantises rows 8 w .. 8 w + 7, lane l elements l + 64 j of a row.
// img: [tiles x 32 x W] int8; meta: [tiles] {1 / s_t (NaN: non-finite value in the tile), E_t, X_t, 0}.
template <int W>
__global__ void __launch_bounds__(256) quantize_tiles_kernel(const unsigned short* __restrict__ rows, signed char* __restrict__ img,
                                                             float4* __restrict__ meta, int64_t tile0) {
    static_assert(screen_width(W), "widths the int8 screen serves");
    constexpr int kScreenD = W;
    __shared__ float red_max[4];
    __shared__ int red_bad[4];
    __shared__ double red_e[4], red_x[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = tile0 + blockIdx.x;
    const unsigned short* src = rows + t * kTileRows * kScreenD;
    float amax = 0.0f;
    int bad = 0;
    for (int r = 8 * wave; r < 8 * wave + 8; ++r)
        for (int j = 0; j < kScreenD / 64; ++j) {
            const float x = bf16_to_f32(src[r * kScreenD + lane + 64 * j]);
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
    const float s = amax > 0.0f ? amax / 127.0f : 1.0f;
    double emax = 0.0, xmax = 0.0;
    for (int r = 8 * wave; r < 8 * wave + 8; ++r) {
        double ee = 0.0, xx = 0.0;
        for (int j = 0; j < kScreenD / 64; ++j) {
            const int c = lane + 64 * j;
            const float x = bf16_to_f32(src[r * kScreenD + c]);
            float qx = 0.0f;
            if (fabsf(x) <= 3.4028235e38f) qx = fminf(127.0f, fmaxf(-127.0f, rintf(x / s)));
            img[(t * kTileRows + r) * kScreenD + c] = (signed char)(int)qx;
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
        emax = fmax(fmax(red_e[0], red_e[1]), fmax(red_e[2], red_e[3])) * (1.0 + 0x1p-40);
        xmax = fmax(fmax(red_x[0], red_x[1]), fmax(red_x[2], red_x[3])) * (1.0 + 0x1p-40);
        const float rs = bad ? __builtin_nanf("") : 1.0f / s;
        meta[t] = make_float4(rs, f32_up(emax + (double)kScreenGamma<W> * (xmax + emax) * (1.0 + 0x1p-20)), f32_up(xmax), 0.0f);
    }
}

// One wave per query of the launch (256 workgroups): screen_quantize_query (kernels_screen8_tile.h) as a launch of its own - for
// searches whose threshold does not come from the dense sample, whose launch carries this work otherwise (kernels_sample.h).
template <int W>
__global__ void __launch_bounds__(64) quantize_queries_kernel(const unsigned short* __restrict__ q, int nrows,
                                                              signed char* __restrict__ img, float4* __restrict__ meta,
                                                              u32* __restrict__ scount) {
    screen_quantize_query<W>(q, nrows, (int)blockIdx.x, (int)threadIdx.x, img, meta, scount);
}

// Exact rescore of the screen's pairs.  Workgroup (q, y): its four waves take chunks of 16 of query q's screened rows in turn
// (chunk 4 y + wave, then every 4 gridDim.y).  A chunk is the A operand of the bf16 pass's MFMA chain - W / 32 k-steps of
// v_mfma_f32_16x16x32_bf16, k-step ks = elements 32 ks + 8 (lane >> 4) of row (lane & 15), the first with a zero accumulator -
// against the query as B, read from column q & 15 as in its own block of 16 queries: for that column the same operands at the
// same lanes as in mfma16_topk_kernel<W, .>, so every score is bit-identical to the one the unscreened pass computes for that
// row.  (A column of D depends on its own column of B only, so the other fifteen columns hold the query too instead of its
// block's other queries: 1.5 KB of query per wave from one cache line set instead of 24 KB - most waves multiply one chunk,
// and the query block was as many bytes as the rows.)  The chunk's entries and row gathers - the long way, to HBM - go out
// before the query's fragments.  Scores >= thr go into the query's list of the final select.  A query whose screen list
// overflowed gets a count past `cap`: the select sends it to the exact re-run.
// W = 1024: the row's 32 fragments fill 128 VGPRs, so the query's 32 sit in AGPRs (the B operand may, as in the pass), and the
// unscreened pass has two arithmetic forms (kernels_mfma16.h; search_mfma.hip picks one per call, and the host passes the same
// choice here).  KSPLIT = false: the plain form, one chain over k-steps 0 .. 31 from a zero accumulator.  KSPLIT = true: the
// paired k-split form - half h of a workgroup's waves multiplies k-steps 8 u + 4 h .. 8 u + 4 h + 3 of every unit u = 0 .. 3 in
// ascending order from a zero accumulator, and the two half sums are added once (ksplit_add4: v_pk_add_f32, one fp32 addition
// per score, commutative - which wave kept and which handed over does not matter).
struct ScreenRescoreArgs {
    const unsigned short* rows;   // bf16 [n_pad x W]
    const unsigned short* q;      // bf16 queries [>= 16 * ceil(nq / 16) x W], as the pass multiplies them
    const float* thr;             // [nq]
    const u64* scand;             // [256][kScreenCap] screened rows
    const u32* scount;            // [256]
    u64* cand;                    // [256][cap] the final select's lists
    u32* count;                   // [256]
    int cap;
};

constexpr int kRescoreY = 8;      // workgroups per query

template <int W, bool KSPLIT>
__global__ void __launch_bounds__(256) screen_rescore_kernel(ScreenRescoreArgs a) {
    static_assert(screen_width(W) && (!KSPLIT || W == 1024), "the k-split is a form of the d = 1024 pass");
    constexpr int kScreenD = W;
    constexpr bool kQueryInAgprs = W == 1024;
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
    constexpr int kSteps = kScreenD / 32;
    auto entry = [&](int cc) { const int e = 16 * cc + r16; return e < m ? (u32)a.scand[(int64_t)q * kScreenCap + e] : 0u; };
    u32 row = entry(c);
    frag16 rf[kSteps];
    {
        const frag16* pr = (const frag16*)(a.rows + (int64_t)row * kScreenD + 8 * kq);
#pragma unroll
        for (int ks = 0; ks < kSteps; ++ks) rf[ks] = pr[4 * ks];
    }
    const float thr = a.thr[q];
    bf16x8 qf[kSteps];
    const bf16x8* pq = (const bf16x8*)(a.q + (int64_t)q * kScreenD + 8 * kq);
#pragma unroll
    for (int ks = 0; ks < kSteps; ++ks) qf[ks] = pq[4 * ks];
    if constexpr (kQueryInAgprs) {
#pragma unroll
        for (int ks = 0; ks < kSteps; ++ks) asm volatile("" : "+a"(qf[ks]));
    }
    for (bool first = true; c < nchunks; c += gridDim.y * 4, first = false) {
        if (!first) {
            row = entry(c);
            const frag16* pr = (const frag16*)(a.rows + (int64_t)row * kScreenD + 8 * kq);
#pragma unroll
            for (int ks = 0; ks < kSteps; ++ks) rf[ks] = pr[4 * ks];
        }
        f32x4 acc;
        if constexpr (KSPLIT) {
            f32x4 half[2];
#pragma unroll
            for (int ks = 0; ks < kSteps; ++ks) {
                constexpr int kUnitSteps = 8;            // k-steps of a unit of the d = 1024 pass: each half of the waves takes four
                const int h = (ks % kUnitSteps) / (kUnitSteps / 2);
                if (ks < kUnitSteps && ks % (kUnitSteps / 2) == 0) mfma16_a_first(half[h], rf[ks], qf[ks]);
                else mfma16_a(half[h], rf[ks], qf[ks]);
            }
            asm volatile("s_nop 15\n\ts_nop 3" : "+v"(half[0]), "+v"(half[1]));   // wait states: MFMA result -> VALU reader
            ksplit_add4(acc, half[0], half[1]);
        } else if constexpr (kQueryInAgprs) {
            mfma16_a_first(acc, rf[0], qf[0]);
#pragma unroll
            for (int ks = 1; ks < kSteps; ++ks) mfma16_a(acc, rf[ks], qf[ks]);
            asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc));
        } else {
            mfma16_v_first(acc, rf[0], qf[0]);
#pragma unroll
            for (int ks = 1; ks < kSteps; ++ks) mfma16_v(acc, rf[ks], qf[ks]);
            asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc));   // wait states: MFMA result -> VALU reader
        }
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
