// attention_f32_kernel: fp32 attention with the whole V^T of a (sequence, head) in LDS.  attention_f32_tiled_kernel
// (kernels_attention_tiled.h) walks the same (query tile, key tile) step operation for operation, as its own text; the bf16 kernels
// are in kernels_attention.h.  The step is NOT a function shared by the two fp32 kernels: written as one, under three spellings,
// the kernels kept their instruction counts and output bits but measured up to 1.5 % slower than before (profiles/HISTORY.md,
// Round 21).  tests/test_attention_tiled_gpu.py holds the two texts to the same bits.
#pragma once
#include "encoder_plan.h"
#include "kernels_mfma16_ops.h"

namespace ts {

// fp32 attention (the encoder at the reference's fp32 storage: SentenceTransformer(name) without a dtype, streamlit_app.py:55,173)
// for sequences of at most 512 (head 64) / 256 (head 128) / 128 (head 256) tokens - the corpus texts of app_create_embeddings.py:48-70
// are global context + statement, up to BERT's 512 positions - any of the three families: softmax(Q K^T * scale + key mask [+ causal]) V with every
// product on v_mfma_f32_16x16x4_f32 - exact fp32 multiplies, fp32 accumulation - straight from the stacked projection's output
// [B][S][(HQ + 2 HKV) HD] into the context layout [B][S][HQ HD] (and, for the fp32-class GEMM behind it, its bf16 pieces).
// torch's attention on this layout first copies q, k, v and the context (four launches of 34 us each per BERT layer at 256 x 128
// tokens, r05_c5 kernel stats) around a 317 us flash launch; here a workgroup per (sequence, query head) holds V^T in LDS and
// each wave walks query tiles of 16:
//   * S^T = K Q^T per key tile: A = K rows (lane (key r16, g): K[key][16 s + 4 g .. + 4), 16 bytes from global / L2), B = Q rows of
//     the tile (same chunks, loaded once per tile); MFMA i of a chunk multiplies float i of both: k = 16 s + 4 g + i - a fixed
//     permutation of the head dimension in the fp32 sum;  D[key 4 g + r][query r16];
//   * softmax over the keys of a query = over r, the key tiles (registers) and the four lane groups (xor 16, 32), in fp32;
//   * O^T = V^T P^T: B = P^T is the score registers as they lie (MFMA r of key tile kj takes keys 16 kj + 4 g + r), A = V^T
//     [d r16][those four keys] = ONE ds_read_b128 of the transposed image (pitch SP + 4 floats: conflict-free);
//     D[d 4 g + r][query r16]: four consecutive d per lane, stored as 16 bytes.
// HD = head size (64 BERT, 128 Qwen3, 256 Gemma3); CAUSAL skips key tiles past the query tile; grouped-query: KV head = h / (HQ / HKV).
// kAttnF32MaxSeq, attn_f32_max_seq, attn_f32_lds: encoder_plan.h

// The key tiles are walked as a RUNNING softmax (one tile's scores in registers at a time: running maximum m, running sum l,
// O rescaled by 2^(m - m') when the maximum moves), so the loop over key tiles is a plain run-time loop over fixed registers: the
// K fragments of tile kj + 1 are requested before the MFMAs of tile kj, the V^T fragments of a tile before its softmax arithmetic.
// (A first cut kept all T score tiles in registers behind `if (kj < kt_end)` branches: no load could move above a branch, every
// key tile paid an L2 round trip in front of its 16 MFMAs, and the launch took as long as torch's attention with its four copies.)
template <int HD, bool CAUSAL>
__global__ void __launch_bounds__(256) attention_f32_kernel(const float* __restrict__ qkv, const int64_t* __restrict__ mask, int B, int S,
                                                             int HQ, int HKV, float scale_log2e, float* __restrict__ out,
                                                             unsigned short* __restrict__ pieces, const float* __restrict__ bias) {
    // bias (may be NULL): the stacked projection's bias [(HQ + 2 HKV) HD], added to q, k and v as they are loaded - the GEMM in
    // front then runs without one (torch.addmm with an output type first copies the broadcast bias into the result: 35 us per
    // GEMM at 256 x 128 tokens, r05 kernel stats)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_attn[];
    float* sVT = (float*)smem_attn;
    const int T = (S + 15) / 16, SP = 16 * T, PP = SP + 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int b = blockIdx.x / HQ, h = blockIdx.x - b * HQ;
    const int hk = h / (HQ / HKV);
    const int r16 = lane & 15, g = lane >> 4;
    const int64_t tok = (int64_t)(HQ + 2 * HKV) * HD;                   // floats per token of the projection's output
    const float* base = qkv + (int64_t)b * S * tok;
    const float* qb = base + (int64_t)h * HD;
    const float* kb = base + (int64_t)(HQ + hk) * HD;
    const float* vb = base + (int64_t)(HQ + HKV + hk) * HD;
    // V^T [d][key] in LDS (keys past the sequence: zeros - 0 x P = 0): 16 bytes of a V row per thread, four 4-byte stores
    for (int i = threadIdx.x; i < SP * (HD / 4); i += blockDim.x) {
        const int key = i / (HD / 4), c = i - key * (HD / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (key < S) {
            v = *(const float4*)(vb + (int64_t)key * tok + 4 * c);
            if (bias) {
                const float4 bv = *(const float4*)(bias + (int64_t)(HQ + HKV + hk) * HD + 4 * c);
                v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
            }
        }
        sVT[(4 * c + 0) * PP + key] = v.x;
        sVT[(4 * c + 1) * PP + key] = v.y;
        sVT[(4 * c + 2) * PP + key] = v.z;
        sVT[(4 * c + 3) * PP + key] = v.w;
    }
    __syncthreads();
    constexpr int KC = HD / 16;                                          // 16-float chunks of a row
    // query tiles of this wave: wave, wave + nwaves, ...  CAUSAL: tile qi walks qi + 1 key tiles, so every second round runs from
    // the far end (rounds of tiles {w, 2 nw - 1 - w}: with eight tiles every wave walks nine key tiles instead of six to twelve)
    for (int it = 0;; ++it) {
        const int lo_ = it * nwaves + wave, hi_ = (it + 1) * nwaves - 1 - wave;
        const int qi = (CAUSAL && (it & 1)) ? hi_ : lo_;
        if (it * nwaves >= T) break;
        if (qi >= T) continue;
        const int qrow = min(16 * qi + r16, S - 1);
        const int qpos = 16 * qi + r16;
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
        const int kt_end = CAUSAL ? qi + 1 : T;                          // key tiles that hold an allowed key
        {
            const int krow = min(r16, S - 1);
#pragma unroll
            for (int s = 0; s < KC; ++s) kf[s] = *(const float4*)(kb + (int64_t)krow * tok + 16 * s + 4 * g);
        }
        f32x4 o[KC];
#pragma unroll
        for (int dj = 0; dj < KC; ++dj) o[dj] = f32x4{0.f, 0.f, 0.f, 0.f};
        float m = -INFINITY, l = 0.0f;                                   // running maximum / sum of query r16 (the same in its four lane groups)
        for (int kj = 0; kj < kt_end; ++kj) {
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
            // the next tile's K fragments and this tile's V^T fragments are on their way while the softmax arithmetic runs
            if (kj + 1 < kt_end) {
                const int krow = min(16 * (kj + 1) + r16, S - 1);
#pragma unroll
                for (int s = 0; s < KC; ++s) kf[s] = *(const float4*)(kb + (int64_t)krow * tok + 16 * s + 4 * g);
            }
            float4 vf[KC];
#pragma unroll
            for (int dj = 0; dj < KC; ++dj) vf[dj] = *(const float4*)(sVT + (16 * dj + r16) * PP + 16 * kj + 4 * g);
            float sc[4], tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * kj + 4 * g + r;
                const bool ok = key < S && (!mask || mask[(int64_t)b * S + key] != 0) && (!CAUSAL || key <= qpos);
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
        const float inv = l > 0.0f ? 1.0f / l : 0.0f;                    // a query without a single allowed key: zeros
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
}

}  // namespace ts
