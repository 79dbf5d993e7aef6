// fp32 attention without the V^T-fits-LDS limit (ts_attention_tiled): attention_f32_kernel (kernels_attention_f32.h) with the V^T image
// fed in chunks of keys, for heads of 64 / 128 / 256 at any sequence length up to kAttnTiledMaxSeq.  The corpus texts are global
// context + statement, up to 512 tokens and more for a checkpoint with a longer max_seq_length; attention_f32_kernel stops at
// 512 / 256 / 128 tokens because it holds the whole V^T of a (sequence, head) in LDS.
//
//   * one workgroup of four waves per (sequence, query head, block of kAttnTiledQueries = 64 queries): wave w owns the query tile
//     4 block + w and keeps that tile's qf, kf, o[KC], m, l in registers, exactly as a wave of attention_f32_kernel does;
//   * V^T [d][key] is staged per chunk of C = attn_tiled_chunk(HD) keys (pitch C + 4 floats, zeros for keys >= S, V's share of
//     the bias added on the way in) into one of TWO buffers: the rows of chunk c + 1 are requested from global memory before the
//     key tiles of chunk c are multiplied and written into the other buffer after them.  One barrier per chunk: the buffer
//     chunk c + 1 goes to was last read in chunk c - 1, which every wave left through that chunk's barrier;
//   * causal: a block walks the chunks up to the one that holds its last query's key, a wave stops at its own kt_end = qi + 1;
//     the blocks of a (sequence, head) are launched from the far end, the longest first (they stay neighbours in the grid: what
//     one reads of K and V, the next finds in the L2).
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
// The arithmetic of a (query tile, key tile) step is attention_f32_kernel's, operation for operation, in the same ascending key
// order: the same two score chains over the same permutation of the head dimension, the same masking to -inf, exp2 with
// scale * log2 e, the same rescale of o, m, l, the same KC output chains, the same 1 / l.  Chunking changes where a V^T fragment is
// read from and nothing else, so wherever both kernels serve a shape the outputs are the same bits
// (tests/test_attention_tiled_gpu.py).  The step is each kernel's own text, not a function the two share, on purpose: with the step (or
// the K fragment load alone) as a __forceinline__ function called here, every instantiation's register assignment moves and
// ts_attention_tiled at head 64 measures 0.4-1.5 % slower than before at 384 / 512 tokens (profiles/HISTORY.md, Round 21).
// Whoever changes the step changes both texts; the test above holds them together.
//
// Staging.  A thread moves 16 bytes of a V row per item: lane -> (key = lane / 4 of 16, columns 4 (lane & 3) ..): a wave's load
// covers 64 contiguous bytes of 16 rows, and its four 4-byte stores (column d, pitch C + 4 = 4 mod 32 banks) fall 2-way on a
// bank per 32-lane half, which a ds_write_b32 does not pay for.  (attention_f32_kernel's order - 16 lanes along a row - is 8-way
// there; it stages once per (sequence, head), this kernel once per query block.)  The fragment reads are the ds_read_b128 of
// attention_f32_kernel; at pitch 132 / 68 floats one 16-byte slot of a lane group is read twice, at pitch 36 (head 256) most
// are: 2-way, behind 128 MFMAs per key tile.
// kAttnTiledMaxSeq, kAttnTiledQueries, attn_tiled_chunk, attn_tiled_lds, attn_tiled_plan: encoder_plan.h
#pragma once
#include "encoder_plan.h"
#include "kernels_mfma16_ops.h"

namespace ts {

// grid = B * HQ * ceil(T / 4), T = ceil(S / 16); 256 threads; dynamic LDS attn_tiled_lds(HD).  Heads of 64 / 128 keep to the 256
// registers of two workgroups per CU, as their LDS does (head 128 takes 286 without the bound; no scratch with it); head 256 needs
// the whole register file of a SIMD for qf, kf, o and the fragments: one workgroup per CU.
// WINDOW: query q reads key k only if |q - k| < W (ts_attention_tiled_window; W is not read without it).  The unwindowed heads of
// 128 / 256 sit at 254 / 511 registers, and the run-time first chunk costs more than what is left: with WINDOW they take 256 / 512
// and 12 / 44 bytes of scratch per lane (causal 36) - staging addresses of load_chunk, written once in front of the chunk loop
// and reloaded once per chunk, none inside the key-tile loop (profiles/HISTORY.md, Round 26, has what was tried against it).
template <int HD, bool CAUSAL, bool WINDOW>
__global__ void __launch_bounds__(256, (HD <= 128 ? 2 : 1))
attention_f32_tiled_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ mask, int B, int S, int HQ, int HKV, float scale_log2e,
                           float* __restrict__ out, unsigned short* __restrict__ pieces, const float* __restrict__ bias, int W) {
    constexpr int C = attn_tiled_chunk(HD);                              // keys per chunk
    constexpr int CT = C / 16;                                           // key tiles per chunk
    constexpr int PP = C + 4;                                            // pitch of a V^T row (floats)
    constexpr int BUF = HD * PP;                                         // floats per buffer
    constexpr int KC = HD / 16;                                          // 16-float chunks of a row
    constexpr int NV = C * (HD / 4) / 256;                               // 16-byte items per thread and chunk
    static_assert(C % 16 == 0 && (C * (HD / 4)) % 256 == 0, "a chunk is whole key tiles and whole rounds of the workgroup");
    static_assert(2 * BUF * 4 == attn_tiled_lds(HD), "the plan's LDS is the two buffers");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_attn_tiled[];
    float* sVT = (float*)smem_attn_tiled;
    const int T = (S + 15) / 16, QB = (T + 3) / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bh = blockIdx.x / QB, qblk = QB - 1 - (blockIdx.x - bh * QB);     // the far (causal: longest) block of a head first
    const int b = bh / HQ, h = bh - b * HQ;
    const int hk = h / (HQ / HKV);
    const int r16 = lane & 15, g = lane >> 4;
    const int64_t tok = (int64_t)(HQ + 2 * HKV) * HD;                   // floats per token of the projection's output
    const float* base = qkv + (int64_t)b * S * tok;
    const float* qb = base + (int64_t)h * HD;
    const float* kb = base + (int64_t)(HQ + hk) * HD;
    const float* vb = base + (int64_t)(HQ + HKV + hk) * HD;
    const float* vbias = bias ? bias + (int64_t)(HQ + HKV + hk) * HD : nullptr;

    // key tiles the BLOCK walks (its last wave's, cut at the sequence) and the chunks that hold them: blockIdx and S alone (with a
    // window: and W - chunks c_first .. c_first + nchunk - 1 of the same walk, attn_window_range)
    const AttnWindowRange wr = WINDOW ? attn_window_range(S, W, CAUSAL, C, qblk, __builtin_amdgcn_readfirstlane(wave)) : AttnWindowRange{};
    const int kt_blk = CAUSAL ? min(4 * qblk + 4, T) : T;
    const int c_first = WINDOW ? wr.c_first : 0;
    const int nchunk = WINDOW ? wr.nchunk : (kt_blk + CT - 1) / CT;
    // this wave's query tile; past the sequence (qi >= T) it walks no key tile and stores nothing
    const int qi = 4 * qblk + wave;
    const int kt_first = WINDOW ? wr.kt_first : 0;                      // key tiles [kt_first, kt_end) hold an allowed key
    const int kt_end = WINDOW ? wr.kt_end : (qi < T ? (CAUSAL ? qi + 1 : T) : 0);
    const int qrow = min(16 * qi + r16, S - 1);
    const int qpos = 16 * qi + r16;

    // a chunk's rows: item j of a thread is wave-item w = wave + 4 j -> 16 keys x 64 bytes (see Staging above)
    float4 vst[NV];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int w = wave + 4 * j;
            const int key = c * C + 16 * (w / (HD / 16)) + (lane >> 2), c4 = 4 * (w % (HD / 16)) + (lane & 3);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (key < S) {
                v = *(const float4*)(vb + (int64_t)key * tok + 4 * c4);
                if (vbias) {
                    const float4 bv = *(const float4*)(vbias + 4 * c4);
                    v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
                }
            }
            vst[j] = v;
        }
    };
    auto store_chunk = [&](float* dst) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int w = wave + 4 * j;
            const int key = 16 * (w / (HD / 16)) + (lane >> 2), c4 = 4 * (w % (HD / 16)) + (lane & 3);
            dst[(4 * c4 + 0) * PP + key] = vst[j].x;
            dst[(4 * c4 + 1) * PP + key] = vst[j].y;
            dst[(4 * c4 + 2) * PP + key] = vst[j].z;
            dst[(4 * c4 + 3) * PP + key] = vst[j].w;
        }
    };

    load_chunk(c_first);
    float4 qf[KC], kf[KC], kbias[KC];
#pragma unroll
    for (int s = 0; s < KC; ++s) {
        qf[s] = *(const float4*)(qb + (int64_t)qrow * tok + 16 * s + 4 * g);
        kbias[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias) {
            const float4 bq = *(const float4*)(bias + (int64_t)h * HD + 16 * s + 4 * g);
            qf[s].x += bq.x; qf[s].y += bq.y; qf[s].z += bq.z; qf[s].w += bq.w;
            kbias[s] = *(const float4*)(bias + (int64_t)(HQ + hk) * HD + 16 * s + 4 * g);
        }
    }
    {
        const int krow = min(16 * kt_first + r16, S - 1);
#pragma unroll
        for (int s = 0; s < KC; ++s) kf[s] = *(const float4*)(kb + (int64_t)krow * tok + 16 * s + 4 * g);
    }
    f32x4 o[KC];
#pragma unroll
    for (int dj = 0; dj < KC; ++dj) o[dj] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.0f;                                       // running maximum / sum of query r16 (the same in its four lane groups)
    store_chunk(sVT);
    __syncthreads();                                                     // barrier 0 of nchunk + 1

#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        const float* cur = sVT + (c & 1) * BUF;
        const int ck = c_first + c;                                      // the chunk's place in the unwindowed walk: keys ck C ..
        if (c + 1 < nchunk) load_chunk(ck + 1);                          // (uniform over the workgroup)
        const int kj_end = min((ck + 1) * CT, kt_end);                   // this wave's key tiles inside the chunk: none, some or all
        for (int kj = WINDOW ? max(ck * CT, kt_first) : ck * CT; kj < kj_end; ++kj) {
            // scores of this tile: two accumulator chains (a dependent 16x16x4 MFMA waits 40 cycles, an independent one 32)
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
            if (bias) {
#pragma unroll
                for (int s = 0; s < KC; ++s) { kf[s].x += kbias[s].x; kf[s].y += kbias[s].y; kf[s].z += kbias[s].z; kf[s].w += kbias[s].w; }
            }
#pragma unroll
            for (int s = 0; s < KC; s += 2) {
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s].x, qf[s].x, a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s + 1].x, qf[s + 1].x, a1, 0, 0, 0);
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s].y, qf[s].y, a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s + 1].y, qf[s + 1].y, a1, 0, 0, 0);
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s].z, qf[s].z, a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s + 1].z, qf[s + 1].z, a1, 0, 0, 0);
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s].w, qf[s].w, a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s + 1].w, qf[s + 1].w, a1, 0, 0, 0);
            }
            // the next tile's K fragments (of the next chunk too: K comes from global memory) and this tile's V^T fragments are
            // on their way while the softmax arithmetic runs
            if (kj + 1 < kt_end) {
                const int krow = min(16 * (kj + 1) + r16, S - 1);
#pragma unroll
                for (int s = 0; s < KC; ++s) kf[s] = *(const float4*)(kb + (int64_t)krow * tok + 16 * s + 4 * g);
            }
            float4 vf[KC];
#pragma unroll
            for (int dj = 0; dj < KC; ++dj) vf[dj] = *(const float4*)(cur + (16 * dj + r16) * PP + 16 * (kj - ck * CT) + 4 * g);
            float sc[4], tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * kj + 4 * g + r;
                bool ok = key < S && (!mask || mask[(int64_t)b * S + key] != 0) && (!CAUSAL || key <= qpos);
                // key - qpos < W && qpos - key < W as one unsigned comparison (W < S here: no overflow)
                if constexpr (WINDOW) ok = ok && (unsigned)(key - qpos + W - 1) < (unsigned)(2 * W - 1);
                sc[r] = ok ? a0[r] + a1[r] : -INFINITY;
                tmax = fmaxf(tmax, sc[r]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float m_new = fmaxf(m, tmax);
            // a tile without a single allowed key so far leaves m = -inf: nothing to rescale, nothing to add
            const float alpha = m_new > -INFINITY ? __builtin_amdgcn_exp2f((m - m_new) * scale_log2e) : 1.0f;
            float psum = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[r] = sc[r] > -INFINITY ? __builtin_amdgcn_exp2f((sc[r] - m_new) * scale_log2e) : 0.0f;
                psum += sc[r];
            }
            psum += __shfl_xor(psum, 16, 64);
            psum += __shfl_xor(psum, 32, 64);
            l = l * alpha + psum;
            m = m_new;
#pragma unroll
            for (int dj = 0; dj < KC; ++dj) {
                o[dj][0] *= alpha; o[dj][1] *= alpha; o[dj][2] *= alpha; o[dj][3] *= alpha;
            }
            // O^T += V^T P^T: KC independent accumulators, MFMA r of the tile takes keys 16 kj + 4 g + r
#pragma unroll
            for (int dj = 0; dj < KC; ++dj) o[dj] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[dj].x, sc[0], o[dj], 0, 0, 0);
#pragma unroll
            for (int dj = 0; dj < KC; ++dj) o[dj] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[dj].y, sc[1], o[dj], 0, 0, 0);
#pragma unroll
            for (int dj = 0; dj < KC; ++dj) o[dj] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[dj].z, sc[2], o[dj], 0, 0, 0);
#pragma unroll
            for (int dj = 0; dj < KC; ++dj) o[dj] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[dj].w, sc[3], o[dj], 0, 0, 0);
        }
        // chunk c + 1 into the other buffer (last read in chunk c - 1, behind that chunk's barrier), then THE barrier of chunk c:
        // every wave of the workgroup, whatever it walked above
        if (c + 1 < nchunk) store_chunk(sVT + ((c + 1) & 1) * BUF);
        __syncthreads();
    }
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;                        // a query without a single allowed key: zeros
    if (qpos < S) {
        float* orow = out ? out + ((int64_t)b * S + qpos) * HQ * HD + (int64_t)h * HD : nullptr;
#pragma unroll
        for (int dj = 0; dj < KC; ++dj) {
            const float y[4] = {o[dj][0] * inv, o[dj][1] * inv, o[dj][2] * inv, o[dj][3] * inv};
            if (orow) *(float4*)(orow + 16 * dj + 4 * g) = make_float4(y[0], y[1], y[2], y[3]);   // (not needed when only the pieces are read)
            if (pieces) {
                const int dtot = HQ * HD;
                store_pieces4(pieces + ((int64_t)b * S + qpos) * 3 * dtot, dtot, (h * HD + 16 * dj + 4 * g) / 4, y);
            }
        }
    }
}

}  // namespace ts
