// The int8 screen's device side inside mfma16_topk_kernel (kernels_mfma16.h, I8) and in the launch that comes before it:
// the query's fold and image, the tile thresholds in pieces, the block test and the admitted-pair path.  kernels_screen8.h
// has the derivation, the quantiser of the corpus and the exact rescore.
#pragma once
#include "kernels_mfma16_ops.h"
#include "mfma16_variants.h"

namespace ts {

// int8 screen (I8, kernels_screen8.h): the same LDS bytes hold 8-byte entries (row, query), twice as many per wave - a screened
// wave expects ~125 of them against ~40 exact candidates of the bf16 pass
constexpr int kScreenStageCap = 384;      // 2 * kMfma16StageCap (kernels_mfma16.h asserts it)
constexpr int kScreenListCap = 65536;   // entries of a query's global list of screened rows (kScreenCap, kernels_screen8.h)

// The same test on the i32 dot products of the int8 screen against the block's integer threshold of the tile.
__device__ __forceinline__ u64 mfma8_block_test(const f32x4& a0, const f32x4& a1, int thr, int& m) {
    u64 mask;
    asm volatile(
        "v_max3_i32 %0, %2, %3, %4\n\t"
        "v_max3_i32 %0, %0, %5, %6\n\t"
        "v_max3_i32 %0, %0, %7, %8\n\t"
        "v_max_i32 %0, %0, %9\n\t"
        "v_cmp_ge_i32 %1, %0, %10"
        : "=&v"(m), "=s"(mask)
        : "v"(a0[0]), "v"(a0[1]), "v"(a0[2]), "v"(a0[3]), "v"(a1[0]), "v"(a1[1]), "v"(a1[2]), "v"(a1[3]), "v"(thr));
    return mask;
}

// The same test in three pieces of at most two instructions, for the late-test screen (kVariantScreenLate): placed one by one in
// MFMA gaps of the NEXT tile (TS16_LATE, kernels_mfma16.h), where the matrix pipe leaves the vector issue free.  They read the
// other tile parity's accumulators, last written a tile ago: no wait states to add.
__device__ __forceinline__ void late_test_a(int& m, const f32x4& a0, const f32x4& a1) {
    asm volatile("v_max3_i32 %0, %1, %2, %3\n\tv_max3_i32 %0, %0, %4, %5" : "=&v"(m) : "v"(a0[0]), "v"(a0[1]), "v"(a0[2]), "v"(a0[3]), "v"(a1[0]));
}
__device__ __forceinline__ void late_test_b(int& m, const f32x4& a1) {
    asm volatile("v_max3_i32 %0, %0, %1, %2\n\tv_max_i32 %0, %0, %3" : "+v"(m) : "v"(a1[1]), "v"(a1[2]), "v"(a1[3]));
}
__device__ __forceinline__ void late_test_c(u64& mask, int m, int thr) {
    asm volatile("v_cmp_ge_i32 %0, %1, %2" : "=s"(mask) : "v"(m), "v"(thr));
}
// ... and the union of two of the lane masks, placed the same way (a scalar instruction: it writes SCC)
__device__ __forceinline__ void late_or(u64& dst, u64 x, u64 y) {
    asm volatile("s_or_b64 %0, %1, %2" : "=s"(dst) : "s"(x), "s"(y) : "scc");
}

// Integer thresholds of the int8 screen (kernels_screen8.h has the derivation and the rounding argument): every row of a tile
// whose exact fp32 score can reach the query's `thr` has an int8 dot product >= the (tile, query) threshold.  The query's side
// is folded once per launch: with rq = 1 / s_q, eq = |e_q|, qn = |q| (rq = NaN: the query holds a non-finite value) and
// athr = |thr| (0 where thr is infinite),
//   q1 = rq (thr - athr 2^-18),  q2 = rq qn (1 + 2^-18),  q3 = rq eq (1 + 2^-18)
// in fp64, rounded to fp32 on the admitting side (q1 down, q2 and q3 up).
__device__ __forceinline__ void screen_fold_query(float thr, float rq, float eq, float qn, float& q1, float& q2, float& q3) {
    const double athr = __builtin_isinf(thr) ? 0.0 : fabs((double)thr);
    const double v1 = (double)rq * ((double)thr - athr * 0x1p-18);
    const double v2 = (double)rq * (double)qn * (1.0 + 0x1p-18);
    const double v3 = (double)rq * (double)eq * (1.0 + 0x1p-18);
    q1 = (float)v1;
    q2 = (float)v2;
    q3 = (float)v3;
    if ((double)q1 > v1) q1 = nextafterf(q1, -__builtin_inff());      // (NaN compares false and stays NaN)
    if ((double)q2 < v2) q2 = nextafterf(q2, __builtin_inff());
    if ((double)q3 < v3) q3 = nextafterf(q3, __builtin_inff());
}
// fp64 -> fp32, never below the value (non-negative bounds that must not shrink)
__device__ __forceinline__ float f32_up(double v) {
    const float f = (float)v;
    return (double)f >= v ? f : __uint_as_float(__float_as_uint(f) + 1u);
}
// The screen's image of one query, by one wave (kernels_screen8.h has the quantisation; kD = the screen's width, 768 or 1024):
// row r of q [nrows x kD] bf16 -> row r of img [256 x kD] int8 and meta[r] = {1 / s_q (NaN: non-finite value), |e_q|, |q|, 0}; a zero row past nrows.  Also empties
// the query's list of screened rows.  Needs nothing but the prepared queries, so it rides in whatever launch comes before the
// screen: the extra workgroup row of the threshold sample (kernels_sample.h), or quantize_queries_kernel.
template <int kD>
__device__ __forceinline__ void screen_quantize_query(const unsigned short* __restrict__ q, int nrows, int r, int lane,
                                                      signed char* __restrict__ img, float4* __restrict__ meta, u32* __restrict__ scount) {
    static_assert(kD == 768 || kD == 1024, "widths the int8 screen serves");
    float v[kD / 64];
    float amax = 0.0f;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < kD / 64; ++j) {
        v[j] = r < nrows ? bf16_to_f32(q[(int64_t)r * kD + lane + 64 * j]) : 0.0f;
        if (!(fabsf(v[j]) <= 3.4028235e38f)) bad = 1;
        else amax = fmaxf(amax, fabsf(v[j]));
    }
    for (int o = 32; o > 0; o >>= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, o));
        bad |= __shfl_xor(bad, o);
    }
    const float s = amax > 0.0f ? amax / 127.0f : 1.0f;
    double ee = 0.0, qq = 0.0;
#pragma unroll
    for (int j = 0; j < kD / 64; ++j) {
        float qx = 0.0f;
        if (fabsf(v[j]) <= 3.4028235e38f) qx = fminf(127.0f, fmaxf(-127.0f, rintf(v[j] / s)));
        img[(int64_t)r * kD + lane + 64 * j] = (signed char)(int)qx;
        const double e = (double)v[j] - (double)s * (double)qx;
        ee += e * e;
        qq += (double)v[j] * (double)v[j];
    }
    ee = wave_sum_f64(ee);
    qq = wave_sum_f64(qq);
    if (lane == 0) {
        meta[r] = make_float4(bad ? __builtin_nanf("") : 1.0f / s, f32_up(sqrt(ee) * (1.0 + 0x1p-40)), f32_up(sqrt(qq) * (1.0 + 0x1p-40)), 0.0f);
        scount[r] = 0;
    }
}

// The threshold of (tile, query) from the tile's scalars tm = (tx = 1 / s_t, ty = coefficient of |q|, tz = coefficient of
// |e_q|; tx = NaN: the tile holds a non-finite value): floor(clamp(fma(tx, fma(-tz, q3, fma(-ty, q2, q1)), -1))), in four
// pieces of at most two VALU instructions with fixed places between the MFMAs of the tile (TS16_THR8): none of it reads an
// accumulator.  The clamp is v_max / v_min (maxNum: a NaN yields the other operand, so NaN -> INT_MIN: every row of the tile is
// a candidate, the exact rescore decides); the literals are -2^31 and 2^30.
template <int P>
__device__ __forceinline__ void screen_thr_piece(int& t, const f32x4& tm, float q1, float q2, float q3) {
    static_assert(P >= 0 && P < 4, "four pieces");
    if constexpr (P == 0)
        asm volatile("v_fma_f32 %0, -%1, %2, %3\n\tv_fma_f32 %0, -%4, %5, %0" : "=&v"(t) : "s"(tm[1]), "v"(q2), "v"(q1), "s"(tm[2]), "v"(q3));
    else if constexpr (P == 1)
        asm volatile("v_fma_f32 %0, %1, %0, -1.0\n\tv_max_f32 %0, 0xcf000000, %0" : "+v"(t) : "s"(tm[0]));
    else if constexpr (P == 2)
        asm volatile("v_min_f32 %0, 0x4e800000, %0\n\tv_floor_f32 %0, %0" : "+v"(t));
    else
        asm volatile("v_cvt_i32_f32 %0, %0" : "+v"(t));
}

// The int8 screen's form of the rare path: (row, query) pairs whose dot product reaches the tile's integer threshold, staged as
// 8-byte entries (row, query) in the wave's own LDS list; the exact score is the rescore's business.  The screen admits eight
// times the pairs of the bf16 pass, and a wave on this path holds up the other three at the next barrier, so it waits for
// nothing: the list belongs to one wave, hence an entry's place is a wave-uniform fill count (`scnt`, an SGPR that lives through
// the whole tile loop; no LDS counter, no atomic) plus the lane's rank among the passing lanes.  Per accumulator value: one
// compare into a lane mask, a scalar branch over the (usual) empty mask, v_mbcnt, one ds_write_b64, scnt += popcount.  The
// ds_write stays in flight - nobody reads the list before the flush behind the tile loop - and an LDS operation in flight only
// makes the fragment ring's counted lgkmcnt waits stricter, never looser (LDS returns in order: "at most N outstanding" then
// certifies the ring's reads and this write), the argument the tile-scalar load already relies on.
// CHECKED: the tile may hold rows >= n (the corpus's last tile) or the search has a row mask (tested before an entry is
// staged: masked-off rows would fill the list up to ten times faster); everything else takes the unchecked form.  A tile is one
// word of the row mask, so the caller reads it once per tile with a SCALAR load (no vector-memory operation: the DMA ring's
// vmcnt queue is left alone), clears the bits of rows >= n and hands every lane its eight bits: `live` bit (g & 3) + 16 (g >> 2)
// = row g of this lane.  A value is looked up there only once some lane's score has passed.
// Padding queries (qid >= nq_real) have threshold 2^30 except in a tile with a non-finite value (INT_MIN): no dot product of
// 768 or 1,024 int8 pairs reaches INT_MAX, which is what they are compared with here.
// A full list sends the wave's further pairs straight to the queries' global lists (vector memory: the DMA ring's counted
// waits see two operations more and wait longer - slow, rare, exact).
// (The pointers are spelled as global-memory pointers: they come out of pinned SGPRs, where hipcc no longer sees that they were
// kernel arguments and would fall back to flat instructions, which count in both wait queues.)
typedef __attribute__((address_space(1))) u32* screen_u32_gptr;
typedef __attribute__((address_space(1))) u64* screen_u64_gptr;
typedef const __attribute__((address_space(4))) u32* screen_mask_cptr;   // (constant address space: a scalar load)
template <bool CHECKED>
__device__ __forceinline__ void mfma8_append_block(const f32x4& a0, const f32x4& a1, int thr, int qid, u32 row_base, u32& scnt,
                                                   uint2* stage, u32 live, u32 nq_real, screen_u32_gptr count, screen_u64_gptr cand) {
    const int thr_q = (u32)qid < nq_real ? thr : 0x7fffffff;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const int s = __builtin_bit_cast(int, (g < 4) ? a0[g & 3] : a1[g & 3]);
        const u32 row = row_base + (g & 3) + 16 * (g >> 2);
        bool pass = s >= thr_q;
        if constexpr (CHECKED) {
            if (__builtin_amdgcn_ballot_w64(pass) == 0) continue;
            pass = pass && ((live >> ((g & 3) + 16 * (g >> 2))) & 1u) != 0;
        }
        const u64 m = __builtin_amdgcn_ballot_w64(pass);
        if (m == 0) continue;
        const u32 at = scnt + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
        const u32 np = (u32)__builtin_popcountll(m);
        if (__builtin_expect(scnt + np <= (u32)kScreenStageCap, 1)) {
            if (pass) stage[at] = make_uint2(row, (u32)qid);
        } else if (pass) {
            if (at < (u32)kScreenStageCap) {
                stage[at] = make_uint2(row, (u32)qid);
            } else {                                                           // list full: straight to the query's list
                const u32 pos = __hip_atomic_fetch_add(&count[qid], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (pos < (u32)kScreenListCap) cand[(int64_t)qid * kScreenListCap + pos] = (u64)row;
            }
        }
        scnt += np;
    }
}

// The tile's scalars (kernels_screen8.h: 1 / s_t, E_t, X_t) as the kernel reads them: one scalar load of 16 bytes.
// (through the constant address space: the kernel's own stores could alias a global pointer, and hipcc would make it a
// vector load - whose wait, vmcnt(0), drains the DMA ring at every tile)
// (one 16-byte load into one SGPR quadruple: loads of separate words get merged into pairs that the loop-carried registers
// do not line up with, and hipcc copies them - behind a wait for the load it has just issued)
typedef const __attribute__((address_space(4))) f32x4* tile_scalars_ptr;
__device__ __forceinline__ void screen_tile_scalars(f32x4& tm, tile_scalars_ptr scr_tile, int64_t lt) { tm = scr_tile[lt]; }

// The block tests of a tile of the screen (mfma16_topk_kernel, I8: behind the ring's drain at the end of the tile): every query
// block of the wave against its integer threshold of the tile.  hit[b] = the lanes of block b with a passing row; returns their union.
template <int NB>
__device__ __forceinline__ u64 screen_tile_test(const f32x4 (&acc)[2][NB], const int (&ithr)[NB], u64 (&hit)[NB]) {
    int ibest[NB];
    u64 iany = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        hit[b] = mfma8_block_test(acc[0][b], acc[1][b], ithr[b], ibest[b]);
        iany |= hit[b];
    }
    return iany;
}
// The rows of the tile at `tile_row` that may be returned, one bit per row (the CHECKED form of mfma8_append_block): its word of
// the row mask (MASKED and there is one; all rows otherwise), less rows >= n.
template <bool MASKED>
__device__ __forceinline__ u32 screen_tile_live(u32 tile_row, u32 s_n, screen_mask_cptr s_mask) {
    u32 word = 0xffffffffu;
    if (tile_row >= s_n) word = 0u;
    else if (MASKED && s_mask != nullptr) word = s_mask[tile_row >> 5];
    if (tile_row < s_n && s_n - tile_row < (u32)kTileRows) word &= (1u << (s_n - tile_row)) - 1u;
    return word;
}
// Behind the tile loop: the wave's staged pairs -> the queries' lists of screened rows.
// (this wave's own writes, read back by the wave that made them: LDS works them off in order)
// (the scalars come by reference: taken by value, hipcc orders two instructions of the flush differently in every instantiation)
__device__ __forceinline__ void screen_flush_stage(const uint2* stage8, const u32& scnt, const int& lane, const screen_u32_gptr& s_count, const screen_u64_gptr& s_cand) {
    const u32 n = min(scnt, (u32)kScreenStageCap);
    for (u32 e = lane; e < n; e += 64) {
        const uint2 v = stage8[e];
        const u32 pos = __hip_atomic_fetch_add(&s_count[v.y], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (pos < (u32)kScreenListCap) s_cand[(int64_t)v.y * kScreenListCap + pos] = (u64)v.x;
    }
}

}  // namespace ts
