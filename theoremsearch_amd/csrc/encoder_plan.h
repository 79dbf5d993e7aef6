// The encoder ops' host decisions (encoder_ops.hip) as pure functions of plain values: the limits of the kernels in
// kernels_encoder.h / kernels_attention.h, which kernel form serves a shape, tile counts, grids, blocks and dynamic LDS.  No
// HIP call, nothing from HIP: the C ABI's codes (include/tsearch.h, plain C) and the standard library only, so
// tests/encoder_plan_check.cpp runs all of it on the CPU under the host sanitizers.  A *_plan function takes any values: it
// decides `ok` first and computes a launch shape only for what it accepts; the *_grid functions take validated ones.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/tsearch.h"

namespace ts {

constexpr int enc_vec(int dtype) { return dtype == TS_BF16 ? 8 : 4; }      // elements per 16-byte access

// ---------------------------------------------------------------------------------------------
// the norm family (add_layernorm, embed_layernorm, add_rmsnorm, gemma_norm): one wave per row, four rows per workgroup
// ---------------------------------------------------------------------------------------------
constexpr int kLnMax = 4;               // 16-byte accesses per lane at most: d <= 64 * kLnMax * vec
struct NormPlan {
    bool ok;            // rows >= 0, d a multiple of vec in [vec, max_d]
    int vec, max_d;     // set for every storage type, accepted or not: the refusal's text names them
    int ln;             // accesses per lane: 1, 2 or 4, the smallest that covers the row
    unsigned grid;
};
inline NormPlan norm_plan(int dtype, int64_t rows, int d) {
    NormPlan p = {false, enc_vec(dtype), 64 * kLnMax * enc_vec(dtype), 0, 0};
    p.ok = rows >= 0 && d >= p.vec && d % p.vec == 0 && d <= p.max_d;
    if (!p.ok) return p;
    const int per_lane = (d / p.vec + 63) / 64;
    p.ln = per_lane <= 1 ? 1 : (per_lane <= 2 ? 2 : 4);
    p.grid = (unsigned)((rows + 3) / 4);
    return p;
}

// ---------------------------------------------------------------------------------------------
// pooling: the vector kernel (16-byte loads, tokens dealt over thread groups) serves the encoders' shapes, the general
// one anything else
// ---------------------------------------------------------------------------------------------
constexpr int kPoolVecSeq = 1024;       // mask bytes the vector kernel keeps in LDS
inline bool pool_vec_form(int h_dtype, int d, int seq, bool hidden_aligned16) {
    const int vec = enc_vec(h_dtype);
    return d % vec == 0 && d / vec <= 256 && seq <= kPoolVecSeq && hidden_aligned16;
}

// ---------------------------------------------------------------------------------------------
// attention: LDS bytes of each kernel at T = ceil(seq / 16) key tiles, and the launch of each entry point
// ---------------------------------------------------------------------------------------------
constexpr int kAttnMaxSeq = 64;         // attention_short_kernel: every score tile in registers
constexpr int attn_wave_lds(int T) {
    const int sp = 16 * T, ks = (sp + 31) / 32;
    const int p_bytes = sp * (32 * ks + 8) * 2, o_bytes = sp * (64 + 8) * 2;
    return (p_bytes > o_bytes ? p_bytes : o_bytes) + 64 * (32 * ks + 8) * 2;      // + V^T [64][keys]
}
constexpr int kAttnRowsMaxSeq = 128;    // attention_rows_kernel: one query tile at a time
constexpr int attn_rows_wave_lds(int T) {
    const int sp = 16 * T, ks = (sp + 31) / 32, pp = 32 * ks + 8;
    return 64 * pp * 2;
}
constexpr int kAttnGqaMaxSeq = 64;      // attention_gqa_kernel
constexpr int attn_gqa_wave_lds(int T) {
    const int sp = 16 * T, ks = (sp + 31) / 32, pp = 32 * ks + 8;
    return 128 * pp * 2 + sp * pp * 2;
}
constexpr int kAttnGqaRowsMaxSeq = 128; // attention_gqa_rows_kernel
constexpr int attn_gqa_rows_tile_bytes(int T) {
    const int sp = 16 * T, ks = (sp + 31) / 32, pp = 32 * ks + 8;
    return 16 * (pp > 136 ? pp : 136) * 2;
}
constexpr int attn_gqa_rows_lds(int T, int R) {            // one V^T image per workgroup + one tile per wave
    const int sp = 16 * T, ks = (sp + 31) / 32, pp = 32 * ks + 8;
    return 128 * pp * 2 + R * attn_gqa_rows_tile_bytes(T);
}
constexpr int kAttnF32MaxSeq = 128;                                  // every head size; smaller heads go further:
constexpr int attn_f32_max_seq(int HD) { return HD == 64 ? 512 : HD == 128 ? 256 : 128; }   // V^T must fit the CU's LDS (<= 133 KB)
constexpr int attn_f32_lds(int HD, int T) { return HD * (16 * T + 4) * 4; }
// what attention_f32_kernel<HD>'s dynamic LDS limit is raised to, once: what the longest sequence of the head size needs
constexpr int attn_f32_lds_limit(int HD) { return attn_f32_lds(HD, attn_f32_max_seq(HD) / 16); }

struct AttnPlan {
    bool ok;            // the head size and the sequence are served (the caller has refused seq < 1 and heads < 1)
    int tiles;          // T of the kernel; ts_attention_float: a run-time value
    bool rows;          // short / gqa past 64 tokens: the one-query-tile-at-a-time kernel
    int r;              // gqa rows form: query heads of a key / value head that one workgroup of r waves serves (1, 2, 4)
    unsigned grid, block;
    int lds;            // dynamic LDS bytes (attention_short_kernel's is static: 0)
};

// ts_attention_short: head size 64; one wave per (sequence, head), four to a workgroup
inline AttnPlan attn_short_plan(int batch, int seq, int heads, int head_dim) {
    AttnPlan p = {};
    p.ok = head_dim == 64 && seq <= kAttnRowsMaxSeq;
    if (!p.ok) return p;
    p.tiles = (seq + 15) / 16;
    p.rows = seq > kAttnMaxSeq;
    p.grid = (unsigned)(((int64_t)batch * heads + 3) / 4);
    p.block = 256;
    p.lds = p.rows ? 4 * attn_rows_wave_lds(p.tiles) : 0;
    return p;
}

// ts_attention_gqa: head size 128.  Up to 64 tokens one wave per (sequence, query head); beyond, the r query heads of a key /
// value group are the r waves of one workgroup and share its V^T image
inline AttnPlan attn_gqa_plan(int batch, int seq, int q_heads, int kv_heads, int head_dim) {
    AttnPlan p = {};
    p.ok = head_dim == 128 && seq <= kAttnGqaRowsMaxSeq;
    if (!p.ok) return p;
    p.tiles = (seq + 15) / 16;
    p.rows = seq > kAttnGqaMaxSeq;
    if (!p.rows) {
        p.grid = (unsigned)(((int64_t)batch * q_heads + 3) / 4);
        p.block = 256;
        p.lds = 4 * attn_gqa_wave_lds(p.tiles);
        return p;
    }
    const int per_kv = q_heads / kv_heads;
    p.r = per_kv % 4 == 0 ? 4 : (per_kv % 2 == 0 ? 2 : 1);
    p.grid = (unsigned)((int64_t)batch * kv_heads * (per_kv / p.r));
    p.block = 64u * (unsigned)p.r;
    p.lds = attn_gqa_rows_lds(p.tiles, p.r);
    return p;
}

// ts_attention_float: head sizes 64 / 128 / 256; one workgroup per (sequence, query head), a wave per query tile up to four
inline AttnPlan attn_float_plan(int batch, int seq, int q_heads, int head_dim) {
    AttnPlan p = {};
    p.ok = (head_dim == 64 || head_dim == 128 || head_dim == 256) && seq <= attn_f32_max_seq(head_dim);
    if (!p.ok) return p;
    p.tiles = (seq + 15) / 16;
    p.grid = (unsigned)((int64_t)batch * q_heads);
    p.block = 64u * (unsigned)std::min(p.tiles, 4);
    p.lds = attn_f32_lds(head_dim, p.tiles);
    return p;
}

// ts_attention_tiled (kernels_attention_tiled.h): the same heads at any length up to kAttnTiledMaxSeq.  One workgroup of four
// waves per (sequence, query head, block of kAttnTiledQueries queries); V^T goes through two LDS buffers of attn_tiled_chunk keys
// each (pitch chunk + 4 floats), about 68 - 74 KB together: two workgroups share a CU's 160 KiB
constexpr int kAttnTiledMaxSeq = 32768;                             // Qwen3's max_position_embeddings
constexpr int kAttnTiledQueries = 64;                               // four query tiles of 16, one per wave
constexpr int attn_tiled_chunk(int HD) { return HD == 64 ? 128 : HD == 128 ? 64 : HD == 256 ? 32 : 0; }
constexpr int attn_tiled_lds(int HD) { return 2 * HD * (attn_tiled_chunk(HD) + 4) * 4; }
static_assert(attn_tiled_lds(64) <= 80 * 1024 && attn_tiled_lds(128) <= 80 * 1024 && attn_tiled_lds(256) <= 80 * 1024,
              "two workgroups per CU");

struct AttnTiledPlan {
    bool ok;            // the head size and the sequence are served and the grid fits 31 bits (the caller has refused seq < 1 and heads < 1)
    int tiles;          // T = ceil(seq / 16)
    int qblocks;        // ceil(T / 4): blocks of kAttnTiledQueries queries
    unsigned grid, block;
    int lds;
};
inline AttnTiledPlan attn_tiled_plan(int batch, int seq, int q_heads, int head_dim) {
    AttnTiledPlan p = {};
    if (!(head_dim == 64 || head_dim == 128 || head_dim == 256) || seq > kAttnTiledMaxSeq) return p;
    p.tiles = (seq + 15) / 16;
    p.qblocks = (p.tiles + 3) / 4;
    const int64_t grid = (int64_t)batch * q_heads * p.qblocks;
    if (grid > INT32_MAX) return p;
    p.ok = true;
    p.grid = (unsigned)grid;
    p.block = 256;
    p.lds = attn_tiled_lds(head_dim);
    return p;
}

// ts_attention_flash (kernels_attention_bf16_tiled.h): bf16 in / out at the same heads and lengths, the same workgroup shape.  The K
// rows (pitch HD + 8 elements) and the V rows (pitch HD + 16: the transposed reads' conflict-free pitch) of a chunk go through two
// LDS buffers, 16 KiB of K and 16 KiB of V each before the pads: 68 - 76 KB together, two workgroups share a CU's 160 KiB
constexpr int kAttnBf16TiledMaxSeq = 32768;
constexpr int kAttnBf16TiledQueries = 64;
constexpr int attn_bf16_tiled_chunk(int HD) { return attn_tiled_chunk(HD); }
constexpr int attn_bf16_tiled_k_pitch(int HD) { return HD + 8; }
constexpr int attn_bf16_tiled_v_pitch(int HD) { return HD + 16; }
constexpr int attn_bf16_tiled_lds(int HD) {
    return 2 * attn_bf16_tiled_chunk(HD) * (attn_bf16_tiled_k_pitch(HD) + attn_bf16_tiled_v_pitch(HD)) * 2;
}
static_assert(attn_bf16_tiled_lds(64) <= 80 * 1024 && attn_bf16_tiled_lds(128) <= 80 * 1024 && attn_bf16_tiled_lds(256) <= 80 * 1024,
              "two workgroups per CU");
static_assert(attn_bf16_tiled_chunk(64) * 64 * 2 == 16 * 1024 && attn_bf16_tiled_chunk(128) * 128 * 2 == 16 * 1024 &&
                  attn_bf16_tiled_chunk(256) * 256 * 2 == 16 * 1024,
              "16 KiB of K and of V per buffer at every head size");

// the launch shape is attn_tiled_plan's: one workgroup per (sequence, query head, block of 64 queries)
inline AttnTiledPlan attn_bf16_tiled_plan(int batch, int seq, int q_heads, int head_dim) {
    AttnTiledPlan p = {};
    if (!(head_dim == 64 || head_dim == 128 || head_dim == 256) || seq < 1 || seq > kAttnBf16TiledMaxSeq || batch < 0 || q_heads < 1) return p;
    p.tiles = (seq + 15) / 16;
    p.qblocks = (p.tiles + 3) / 4;
    const int64_t grid = (int64_t)batch * q_heads * p.qblocks;
    if (grid > INT32_MAX) return p;
    p.ok = true;
    p.grid = (unsigned)grid;
    p.block = 256;
    p.lds = attn_bf16_tiled_lds(head_dim);
    return p;
}

// ts_attention_flash_window / ts_attention_tiled_window: the same kernels with a sliding window - query q reads key k only if
// |q - k| < window (transformers' convention on both sides).  What the workgroup of query block `qblk` (64 queries, chunks of C keys
// aligned to multiples of C from key 0) and its wave `wave` (query tile qi = 4 qblk + wave) walk:
//   chunks  c_first .. c_first + nchunk - 1: the ones that hold a key some query of the block may read - blockIdx, seq and window
//           alone, so every wave of the workgroup counts the same barriers;
//   tiles   [kt_first, kt_end) of 16 keys: the ones that hold a key some query of the WAVE's tile may read; a wave past the
//           sequence (qi >= T) walks none.  They decide what a wave multiplies between the barriers, never how many it meets.
// window >= seq hides nothing: the ranges are the unwindowed kernels' (c_first = 0, nchunk = ceil(kt_blk / CT), kt_first = 0).
struct AttnWindowRange {
    int c_first, nchunk;    // chunks of the block
    int kt_first, kt_end;   // key tiles of the wave
};
constexpr AttnWindowRange attn_window_range(int seq, int window, bool causal, int C, int qblk, int wave) {
    const int T = (seq + 15) / 16;
    const int w1 = (window < seq ? window : seq) - 1;                  // |q - k| < seq always: no overflow at any window
    const int q_first = 64 * qblk, q_last = q_first + 63 < seq - 1 ? q_first + 63 : seq - 1;
    const int k_last = causal ? q_last : (q_last + w1 < seq - 1 ? q_last + w1 : seq - 1);
    AttnWindowRange r = {};
    r.c_first = (q_first - w1 > 0 ? q_first - w1 : 0) / C;
    r.nchunk = k_last / C - r.c_first + 1;
    const int qi = 4 * qblk + wave;
    if (qi >= T) return r;                                              // kt_first = kt_end = 0
    const int t_last = 16 * qi + 15 < seq - 1 ? 16 * qi + 15 : seq - 1;
    const int kt_far = (t_last + w1) / 16 + 1;
    r.kt_first = (16 * qi - w1 > 0 ? 16 * qi - w1 : 0) / 16;
    r.kt_end = causal ? qi + 1 : (kt_far < T ? kt_far : T);
    return r;
}

// ---------------------------------------------------------------------------------------------
// the other grids
// ---------------------------------------------------------------------------------------------
// *_qk_norm_rope: a head is head_dim / vec lanes of a wave; 4 waves x heads per wave to a workgroup
inline unsigned qk_norm_rope_grid(int dtype, int64_t tokens, int q_heads, int kv_heads, int head_dim) {
    const int64_t items = tokens * (q_heads + kv_heads);
    const int per_wg = 4 * (64 / (head_dim / enc_vec(dtype)));
    return (unsigned)((items + per_wg - 1) / per_wg);
}
// act_pieces, split_pieces, swiglu, geglu: grid-stride loops over `total` 16-byte items
inline unsigned elementwise_grid(int64_t total) { return (unsigned)std::min<int64_t>((total + 255) / 256, 16384); }

}  // namespace ts
