// bf16 attention without a length limit of its own (ts_attention_flash): a flash-style kernel on v_mfma_f32_16x16x32_bf16 for heads
// of 64 / 128 / 256, causal or not, grouped-query or not, at any sequence length up to kAttnBf16TiledMaxSeq.  The wave-per-problem
// kernels of kernels_attention.h keep every key of a row in registers and stop at 128 tokens; head 256 had no bf16 kernel at all.
// The form is attention_f32_tiled_kernel's (kernels_attention_tiled.h): the same host plan, launch order and barrier discipline.
//
//   * one workgroup of four waves per (sequence, query head, block of kAttnBf16TiledQueries = 64 queries): wave w owns the query
//     tile 4 block + w and keeps its Q fragments (HD / 32 x 4 registers), the fp32 O^T accumulators (HD / 16 x 4) and the running
//     maximum m and sum l of its rows in registers for the whole walk;
//   * the K rows [key][HD + 8] and the V rows [key][HD + 16] of a chunk of C = attn_bf16_tiled_chunk(HD) keys (16 KiB each without
//     the pads; zeros for keys >= S) are staged through registers into one of TWO buffers: the rows of chunk c + 1 are requested
//     from global memory before chunk c is multiplied and written into the other buffer after it.  One barrier per chunk: the
//     buffer chunk c + 1 goes to was last read in chunk c - 1, which every wave left through that chunk's barrier;
//   * causal: a block walks the chunks up to the one that holds its last query's key, a wave stops at its own kt_end = qi + 1 (tile
//     qi multiplies key tiles 0 .. qi only); the blocks of a (sequence, head) are launched from the far end, the longest first,
//     and stay neighbours in the grid;
//   * grouped-query: query head h reads key / value head h / (HQ / HKV); the heads of a group are neighbours in the grid (head-major
//     block order), so what one reads of K and V the next finds in the L2.
//
// THE BARRIER RULE.  The number of barriers a workgroup executes is a function of blockIdx, the launch's S and (WINDOW) its W
// alone: nchunk below.  Every wave stages its share of every WALKED chunk and arrives at every walked chunk's barrier - a wave
// whose query tile lies past the sequence (a short last block), a wave that has run out of causal keys, a wave whose rows are
// all padding, a wave whose window has not begun or has ended.  Such a wave walks no key tile (kt_end = 0 or already reached,
// kt_first not yet reached) and stores nothing, but it never returns early, and nothing between the barriers branches around
// one.  A wave that skips a barrier hangs the workgroup, and with it the machine.
//
// WINDOW (a compile-time form; W a run-time argument): query q reads key k only if |q - k| < W, and the mask allows k, and
// k <= q under causal.  The chunks stay aligned to multiples of C from key 0: a block walks chunks c_first .. c_first + nchunk - 1
// of the unwindowed walk (attn_window_range, encoder_plan.h), a wave multiplies the key tiles [kt_first, kt_end) of them, and
// the per-key predicate gains the window as one more select.  A chunk or tile that is skipped and one that is walked with
// every key excluded leave m, l, o with the same bits, so the result is the unwindowed kernel's under the equivalent key mask,
// bit for bit (tests/test_attention_window_gpu.py).  Without WINDOW nothing of this is compiled in.
//
// Arithmetic per (query tile, chunk) - tests/attention_bf16_tiled_common.py models it:
//   1. fp32 scores of the chunk's keys from the bf16 MFMA (HD / 32 chained k-steps per key tile);
//   2. the scores of keys that are masked, past the sequence or causal-excluded are replaced by a select (never a multiply: an
//      excluded key's score may be Inf or NaN);
//   3. m_new = max(m, chunk max over the allowed keys), f = exp2((m - m_new) scale_log2e), exactly 0 while m is still -inf (a
//      chunk without an allowed key in front of the first allowed one never computes -inf - (-inf));
//   4. e = exp2((s - m_new) scale_log2e) for the allowed keys, 0 for the others;
//   5. l = l f + sum e, an fp32 sum of the unrounded e (a lane's keys in ascending order, then the four lane groups);
//   6. P = e rounded to bf16, to nearest even;  7. o = o f + P V in fp32;
//   8. after the last chunk out = bf16(o (1 / l)); a row without a single allowed key is zeros;
//   9. the rescale happens at every chunk (no deferred-max threshold).
//
// The two choices.
//   P -> second MFMA: the SWAPPED product.  The scores are computed as S^T = K Q^T (K rows the A operand, Q rows the B operand), so a
//   lane holds, for ITS query (column r16), keys 4 g .. 4 g + 3 of every key tile: the row maximum and sum are register loops plus two
//   xor-shuffles (16, 32), m / l / f are one scalar per lane, and two packed score tiles are the B fragment of the 32-key step of
//   O^T = V^T P^T as they stand - element j of lane group g is key 32 s + 16 (j >> 2) + 4 g + (j & 3).  No P tile in LDS, no
//   wave_lds_sync between the two products, and the LDS budget stays K + V.  (The rows kernels' P tile would add 4 x 16 x (C + 8) x 2
//   bytes and two LDS round trips per chunk.)
//   V: rows AS THEY LIE, read back with ds_read_b64_tr_b16.  The k order of the step above is what one transposed read delivers:
//   lane group g reads the 4-key x 16-column block of keys 32 s + 16 t + 4 g .. + 3 (t = 0, 1), columns 16 dj .., and lane r16 receives
//   column 16 dj + r16 of those four keys.  Staging V is then K's staging (16-byte row pieces, ds_write_b128); a V^T image written
//   with vt_store_key_pair costs eight 4-byte writes per key pair and lane that fall 8-way on a bank at every pitch a 16-byte
//   fragment read allows (8 columns x pitch = 0 mod 32 banks).  EXEC is all ones at every transposed read: the reads stand under
//   wave-uniform conditions only (scalar loop bounds from readfirstlane(wave), blockIdx and S), keys past the sequence are zero
//   rows (pad, never mask); a lane's address is 8-byte aligned (pitch 2 (HD + 16) bytes, column 4 p), the dynamic LDS 16-byte.
//   The pitch HD + 16 puts the eight rows of a 32-lane half 8 dwords apart mod 64 banks: conflict-free.
//
// Shared steps of kernels_attention.h used here: wave_lds_sync, o_tile_stage, o_row_out16 (whole output rows through a wave-private
// tile in the LDS the last barrier has freed).  attn_key_flags (keys on the lanes r16), v_pair_load / vt_store_key_pair (the V^T image)
// and lds_zero16 (no image to clear) belong to the other orientation and do not fit.
// kAttnBf16TiledMaxSeq, kAttnBf16TiledQueries, attn_bf16_tiled_chunk, attn_bf16_tiled_lds, attn_bf16_tiled_plan: encoder_plan.h
#pragma once
#include "encoder_plan.h"
#include "kernels_attention.h"

namespace ts {

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// four keys x 16 columns of bf16 rows, transposed on the way out (ds_read_b64_tr_b16): lane 4 q + p of a 16-lane group passes the
// address of (row q, columns 4 p ..) and receives column (its index in the group) of rows 0 .. 3.  EXEC must be all ones.
__device__ __forceinline__ bf16x4 lds_read_tr16(const unsigned short* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)p);
}

// grid = B * HQ * ceil(T / 4), T = ceil(S / 16); 256 threads; dynamic LDS attn_bf16_tiled_lds(HD).  Heads of 64 / 128 keep to the 256
// registers of two workgroups per CU, as their LDS does; head 256 (32 + 64 registers of Q and O alone) takes one.
// WINDOW: query q reads key k only if |q - k| < W (ts_attention_flash_window; W is not read without it).
template <int HD, bool CAUSAL, bool WINDOW>
__global__ void __launch_bounds__(256, (HD <= 128 ? 2 : 1))
attention_bf16_tiled_kernel(const unsigned short* __restrict__ qkv, const int64_t* __restrict__ mask, int B, int S, int HQ, int HKV,
                            float scale_log2e, unsigned short* __restrict__ out, int W) {
    constexpr int C = attn_bf16_tiled_chunk(HD);                         // keys per chunk
    constexpr int CT = C / 16;                                           // key tiles per chunk
    constexpr int CS = C / 32;                                           // 32-key steps of the second product per chunk
    constexpr int KS = HD / 32;                                          // 32-deep k-steps of the score product
    constexpr int KC = HD / 16;                                          // 16-column tiles of a row
    constexpr int KP = attn_bf16_tiled_k_pitch(HD), VP = attn_bf16_tiled_v_pitch(HD);   // pitches of the K and V rows (elements)
    constexpr int KBUF = C * KP, BUF = C * (KP + VP);                    // elements: K rows of a buffer, a whole buffer
    constexpr int NV = C * (HD / 8) / 256;                               // 16-byte items per thread, chunk and matrix
    constexpr int OP = HD + 8;                                           // pitch of the O tile
    static_assert(C % 32 == 0 && (C * (HD / 8)) % 256 == 0, "a chunk is whole 32-key steps and whole rounds of the workgroup");
    static_assert(2 * BUF * 2 == attn_bf16_tiled_lds(HD), "the plan's LDS is the two buffers");
    static_assert(4 * 16 * OP <= 2 * BUF, "the waves' O tiles fit the buffers");
    static_assert((KP * 2) % 16 == 0 && (VP * 2) % 16 == 0 && (KBUF * 2) % 16 == 0 && (BUF * 2) % 16 == 0, "16-byte rows, 8-byte transposed reads");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_attn_bf16_tiled[];
    unsigned short* smem = (unsigned short*)smem_attn_bf16_tiled;
    const int T = (S + 15) / 16, QB = (T + 3) / 4;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bh = blockIdx.x / QB, qblk = QB - 1 - (blockIdx.x - bh * QB);     // the far (causal: longest) block of a head first
    const int b = bh / HQ, h = bh - b * HQ;
    const int hk = h / (HQ / HKV);
    const int r16 = lane & 15, g = lane >> 4;
    const int64_t tok = (int64_t)(HQ + 2 * HKV) * HD;                   // elements per token of the projection's output
    const unsigned short* base = qkv + (int64_t)b * S * tok;
    const unsigned short* qb = base + (int64_t)h * HD;
    const unsigned short* kb = base + (int64_t)(HQ + hk) * HD;
    const unsigned short* vb = base + (int64_t)(HQ + HKV + hk) * HD;
    const int64_t* mrow = mask ? mask + (int64_t)b * S : nullptr;

    // key tiles the BLOCK walks (its last wave's, cut at the sequence) and the chunks that hold them: blockIdx and S alone (with a
    // window: and W - chunks c_first .. c_first + nchunk - 1 of the same walk, attn_window_range)
    const AttnWindowRange wr = WINDOW ? attn_window_range(S, W, CAUSAL, C, qblk, wave) : AttnWindowRange{};
    const int kt_blk = CAUSAL ? min(4 * qblk + 4, T) : T;
    const int c_first = WINDOW ? wr.c_first : 0;
    const int nchunk = WINDOW ? wr.nchunk : (kt_blk + CT - 1) / CT;
    // this wave's query tile; past the sequence (qi >= T) it walks no key tile and stores nothing
    const int qi = 4 * qblk + wave;
    const int kt_first = WINDOW ? wr.kt_first : 0;                      // key tiles [kt_first, kt_end) hold an allowed key
    const int kt_end = WINDOW ? wr.kt_end : (qi < T ? (CAUSAL ? qi + 1 : T) : 0);
    const int qrow = min(16 * qi + r16, S - 1);
    const int qpos = 16 * qi + r16;

    // a chunk's K and V rows: item j of a thread is piece i = threadIdx.x + 256 j -> row i / (HD / 8), 16 bytes at column 8 (i % (HD / 8))
    uint4 kst[NV], vst[NV];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = threadIdx.x + 256 * j;
            const int key = c * C + i / (HD / 8), c8 = i % (HD / 8);
            uint4 k4 = make_uint4(0u, 0u, 0u, 0u), v4 = make_uint4(0u, 0u, 0u, 0u);
            if (key < S) {
                k4 = *(const uint4*)(kb + (int64_t)key * tok + 8 * c8);
                v4 = *(const uint4*)(vb + (int64_t)key * tok + 8 * c8);
            }
            kst[j] = k4;
            vst[j] = v4;
        }
    };
    auto store_chunk = [&](unsigned short* dst) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = threadIdx.x + 256 * j;
            const int row = i / (HD / 8), c8 = i % (HD / 8);
            *(uint4*)(dst + row * KP + 8 * c8) = kst[j];
            *(uint4*)(dst + KBUF + row * VP + 8 * c8) = vst[j];
        }
    };

    load_chunk(c_first);
    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const bf16x8*)(qb + (int64_t)qrow * tok + 32 * ks + 8 * g);
    f32x4 o[KC];
#pragma unroll
    for (int dj = 0; dj < KC; ++dj) o[dj] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.0f;                                       // running maximum / sum of query r16 (the same in its four lane groups)
    store_chunk(smem);
    __syncthreads();                                                     // barrier 0 of nchunk + 1

#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        const unsigned short* cK = smem + (c & 1) * BUF;
        const unsigned short* cV = cK + KBUF;
        const int ck = c_first + c;                                      // the chunk's place in the unwindowed walk: keys ck C ..
        if (c + 1 < nchunk) load_chunk(ck + 1);                          // (uniform over the workgroup)
        const int nt = min(CT, kt_end - ck * CT);                        // this wave's key tiles inside the chunk: none (<= t0), some or all
        const int t0 = WINDOW ? max(0, kt_first - ck * CT) : 0;          // ... the first of them (a window's near edge)
        if (nt > t0) {                                                   // (uniform over the wave; no barrier inside)
            // S^T = K Q^T: D[key 4 g + r][query r16] of each key tile.  A tile outside [t0, nt) holds no allowed key: not multiplied
            f32x4 sc[CT];
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
                if (t >= t0 && t < nt) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        const bf16x8 kf = *(const bf16x8*)(cK + (16 * t + r16) * KP + 32 * ks + 8 * g);
                        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], a, 0, 0, 0);
                    }
                }
                sc[t] = a;
            }
            bool ok[CT][4];
            float cmax = -INFINITY;
#pragma unroll
            for (int t = 0; t < CT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = ck * C + 16 * t + 4 * g + r;
                    ok[t][r] = t < nt && key < S && (!CAUSAL || key <= qpos) && (!mrow || mrow[key] != 0);
                    if constexpr (WINDOW) ok[t][r] = ok[t][r] && t >= t0 && key - qpos < W && qpos - key < W;
                    cmax = fmaxf(cmax, ok[t][r] ? sc[t][r] : -INFINITY);
                }
            cmax = fmaxf(cmax, __shfl_xor(cmax, 16, 64));
            cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
            const float m_new = fmaxf(m, cmax);
            // nothing accumulated so far (m = -inf): the factor is exactly 0, never exp2(-inf - -inf)
            const float f = m > -INFINITY ? __builtin_amdgcn_exp2f((m - m_new) * scale_log2e) : 0.0f;
            float psum = 0.0f;
#pragma unroll
            for (int t = 0; t < CT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[t][r] = ok[t][r] ? __builtin_amdgcn_exp2f((sc[t][r] - m_new) * scale_log2e) : 0.0f;
                    psum += sc[t][r];
                }
            psum += __shfl_xor(psum, 16, 64);
            psum += __shfl_xor(psum, 32, 64);
            l = l * f + psum;
            m = m_new;
#pragma unroll
            for (int dj = 0; dj < KC; ++dj) {
                o[dj][0] *= f; o[dj][1] *= f; o[dj][2] *= f; o[dj][3] *= f;
            }
            // O^T += V^T P^T, 32 keys a step: B = the two packed score tiles, A = two transposed reads of V's rows in the same key order
#pragma unroll
            for (int s = 0; s < CS; ++s) {
                if (2 * s < nt && 2 * s + 1 >= t0) {                       // either of the step's two tiles is walked
                    union { uint4 u; bf16x8 v; } pf;
                    pf.u = make_uint4(pack_bf16_hw(sc[2 * s][0], sc[2 * s][1]), pack_bf16_hw(sc[2 * s][2], sc[2 * s][3]),
                                      pack_bf16_hw(sc[2 * s + 1][0], sc[2 * s + 1][1]), pack_bf16_hw(sc[2 * s + 1][2], sc[2 * s + 1][3]));
                    const unsigned short* vrow = cV + (32 * s + 4 * g + (r16 >> 2)) * VP + 4 * (r16 & 3);
#pragma unroll
                    for (int dj = 0; dj < KC; ++dj) {
                        const bf16x4 v0 = lds_read_tr16(vrow + 16 * dj), v1 = lds_read_tr16(vrow + 16 * VP + 16 * dj);
                        const bf16x8 vf = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                        o[dj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf.v, o[dj], 0, 0, 0);
                    }
                }
            }
        }
        // chunk c + 1 into the other buffer (last read in chunk c - 1, behind that chunk's barrier), then THE barrier of chunk c:
        // every wave of the workgroup, whatever it walked above
        if (c + 1 < nchunk) store_chunk(smem + ((c + 1) & 1) * BUF);
        __syncthreads();
    }
    // every wave has left the last chunk: the buffers are free, each wave takes a tile for its rows [query][d] and writes whole rows
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;                        // a query without a single allowed key: zeros
    unsigned short* sO = smem + wave * 16 * OP;
#pragma unroll
    for (int dj = 0; dj < KC; ++dj) {
        const f32x4 y = {o[dj][0] * inv, o[dj][1] * inv, o[dj][2] * inv, o[dj][3] * inv};
        o_tile_stage(sO + r16 * OP + 16 * dj + 4 * g, y);
    }
    wave_lds_sync();
    unsigned short* obase = out + (int64_t)b * S * HQ * HD + (int64_t)h * HD;
#pragma unroll
    for (int i = lane; i < 16 * (HD / 8); i += 64) o_row_out16<HD>(obase, (int64_t)HQ * HD, sO, OP, 16 * qi, S, i);
}

}  // namespace ts
