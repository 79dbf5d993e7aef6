// libtsearch.so - C ABI (include/tsearch.h), part 3: the encoder-side kernels: pooling + L2
// normalisation + cast, residual add + LayerNorm, the input layer, short-sequence attention.
// Every entry point: validate (every refusal, then "nothing to do", before the device is touched) -> plan (encoder_plan.h:
// kernel form, grid, block, LDS) -> launch (dispatch_value, host.h, turns the plan's run-time values into template arguments).
#include <initializer_list>

#include "host.h"
#include "kernels_attention.h"
#include "kernels_attention_bf16_tiled.h"
#include "kernels_attention_f32.h"
#include "kernels_attention_tiled.h"
#include "kernels_encoder.h"

// ---- validators: TS_OK, or the refusal (code and text set) ---------------------------------------------------------------------
static int require(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (!p) return fail(TS_ERR_INVALID, "NULL argument");
    return TS_OK;
}

static int aligned16(std::initializer_list<const void*> ptrs, const char* refusal) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;          // NULL (an optional operand) is aligned
    return (bits & 15) != 0 ? fail(TS_ERR_INVALID, "%s", refusal) : TS_OK;
}

static int pieces_from_f32(const void* pieces, int dtype) {
    if (pieces && (dtype != TS_F32 || ((uintptr_t)pieces & 7) != 0)) return fail(TS_ERR_INVALID, "pieces come from fp32 rows, 8-byte aligned");
    return TS_OK;
}

static int storage_dtype(int dtype) {
    return dtype != TS_F32 && dtype != TS_BF16 ? fail(TS_ERR_INVALID, "dtype %d", dtype) : TS_OK;
}

static int norm_refusal(const NormPlan& p, int d, const char* more = "") {
    return fail(TS_ERR_INVALID, "d = %d must be a multiple of %d and at most %d%s", d, p.vec, p.max_d, more);
}

// ---- the device side of an entry point ------------------------------------------------------------------------------------------
static int enter_device(int device, void* stream, hipStream_t* st) {
    TS_TRY(check_device(device));
    HIP_TRY(hipSetDevice(device));
    *st = (hipStream_t)stream;
    return TS_OK;
}

// one launch of 256 threads without dynamic LDS (with: launch_lds, host.h)
template <auto Kernel, class... A>
static int launch(unsigned grid, hipStream_t st, const A&... args) {
    Kernel<<<grid, 256, 0, st>>>(args...);
    HIP_TRY(hipGetLastError());
    return TS_OK;
}

// go(storage type, accesses per lane) of a norm launch, both as variant_c
template <class Go>
static int dispatch_norm(int dtype, const NormPlan& p, Go&& go) {
    return dispatch_value<0, 1>(dtype, [&](auto dt) { return dispatch_value<1, 2, 4>(p.ln, [&](auto ln) { return go(dt, ln); }); });
}

extern "C" int ts_pool_normalize(int device, const void* hidden, int h_dtype, const int64_t* attention_mask, int64_t n,
                                 int32_t seq, int32_t d, int pooling, int normalize, void* out, int out_dtype, int64_t out_ld,
                                 void* stream) {
    TS_TRY(require({hidden, attention_mask, out}));
    if ((h_dtype != TS_F32 && h_dtype != TS_BF16) || (out_dtype != TS_F32 && out_dtype != TS_BF16))
        return fail(TS_ERR_INVALID, "dtype");
    if (n < 0 || seq < 1 || d < 1 || d > 4096 || out_ld < d) return fail(TS_ERR_INVALID, "bad shape (d must be <= 4096)");
    if (pooling < TS_POOL_MEAN || pooling > TS_POOL_CLS) return fail(TS_ERR_INVALID, "pooling %d", pooling);
    if (n == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    // the encoders' shapes take the vector form (16-byte loads, tokens dealt over thread groups); anything else the general one
    const bool vform = pool_vec_form(h_dtype, d, seq, ((uintptr_t)hidden & 15) == 0);
    return dispatch_value<0, 1>(h_dtype, [&](auto h) {
        return dispatch_value<0, 1>(out_dtype, [&](auto o) {
            if (vform) return launch<pool_normalize_vec_kernel<h, o>>((unsigned)n, st, hidden, attention_mask, seq, d, pooling, normalize, out, out_ld);
            return launch<pool_normalize_kernel<h, o>>((unsigned)n, st, hidden, attention_mask, seq, d, pooling, normalize, out, out_ld);
        });
    });
}

static int add_layernorm_impl(int device, const void* a, const void* b, const void* gamma, const void* beta, float eps, int64_t rows,
                              int32_t d, int dtype, void* out, unsigned short* pieces, void* stream, const float* a_bias = nullptr) {
    if (a_bias && (dtype != TS_F32 || ((uintptr_t)a_bias & 15) != 0)) return fail(TS_ERR_INVALID, "a_bias: fp32 rows only, 16-byte aligned");
    TS_TRY(require({a, b, gamma, beta, out}));
    TS_TRY(pieces_from_f32(pieces, dtype));
    TS_TRY(storage_dtype(dtype));
    const NormPlan p = norm_plan(dtype, rows, d);
    if (!p.ok) return norm_refusal(p, d);
    TS_TRY(aligned16({a, b, gamma, beta, out}, "buffers must be 16-byte aligned"));
    if (rows == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    return dispatch_norm(dtype, p, [&](auto dt, auto ln) {
        return launch<add_layernorm_kernel<dt, ln>>(p.grid, st, a, b, gamma, beta, eps, rows, d, out, pieces, a_bias);
    });
}

extern "C" int ts_add_layernorm(int device, const void* a, const void* b, const void* gamma, const void* beta, float eps, int64_t rows,
                                int32_t d, int dtype, void* out, void* stream) {
    return add_layernorm_impl(device, a, b, gamma, beta, eps, rows, d, dtype, out, nullptr, stream);
}

extern "C" int ts_add_layernorm_pieces(int device, const void* a, const void* a_bias, const void* b, const void* gamma, const void* beta,
                                       float eps, int64_t rows, int32_t d, void* out, void* pieces, void* stream) {
    TS_TRY(require({pieces}));
    return add_layernorm_impl(device, a, b, gamma, beta, eps, rows, d, TS_F32, out, (unsigned short*)pieces, stream, (const float*)a_bias);
}

extern "C" int ts_embed_layernorm(int device, const int64_t* ids, const int64_t* type_ids, const void* word, const void* pos,
                                  const void* type, int64_t n_word, int64_t n_pos, int64_t n_type, const void* gamma, const void* beta,
                                  float eps, int64_t tokens, int32_t seq, int32_t d, int dtype, void* out, void* stream) {
    TS_TRY(require({ids, word, pos, type, gamma, beta, out}));
    TS_TRY(storage_dtype(dtype));
    const NormPlan p = norm_plan(dtype, tokens, d);
    if (!p.ok || seq < 1) return norm_refusal(p, d, "; seq >= 1");
    if (n_word < 1 || n_pos < 1 || n_type < 1) return fail(TS_ERR_INVALID, "empty embedding table");
    TS_TRY(aligned16({word, pos, type, gamma, beta, out}, "tables and output must be 16-byte aligned"));
    if (tokens == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    return dispatch_norm(dtype, p, [&](auto dt, auto ln) {
        return launch<embed_layernorm_kernel<dt, ln>>(p.grid, st, ids, type_ids, word, pos, type, n_word, n_pos, n_type, gamma, beta, eps,
                                                            tokens, seq, d, out);
    });
}

extern "C" int ts_attention_short(int device, const void* qkv, const int64_t* attention_mask, int32_t batch, int32_t seq, int32_t heads,
                                 int32_t head_dim, void* out, void* stream) {
    TS_TRY(require({qkv, out}));
    if (batch < 0 || seq < 1 || heads < 1) return fail(TS_ERR_INVALID, "batch = %d, seq = %d, heads = %d", batch, seq, heads);
    const AttnPlan p = attn_short_plan(batch, seq, heads, head_dim);
    if (!p.ok)
        return fail(TS_ERR_UNSUPPORTED, "head size %d / %d tokens: this kernel serves head size 64 and at most %d tokens", head_dim, seq,
                    kAttnRowsMaxSeq);
    TS_TRY(aligned16({qkv, out}, "qkv and out must be 16-byte aligned"));
    if (batch == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    const unsigned short* in = (const unsigned short*)qkv;
    unsigned short* o = (unsigned short*)out;
    return dispatch_value<1, 2, 3, 4, 5, 6, 7, 8>(p.tiles, [&](auto t) {
        // 65 .. 128 tokens: one query tile at a time (attention_rows_kernel, dynamic LDS: 4 waves x up to 17 KB, two workgroups per CU)
        if constexpr (t > kAttnMaxSeq / 16)
            return launch_lds<attention_rows_kernel<t>>(device, p.grid, p.block, p.lds, st, in, attention_mask, batch, seq, heads, o);
        else
            return launch<attention_short_kernel<t>>(p.grid, st, in, attention_mask, batch, seq, heads, o);
    });
}

static int add_rmsnorm_impl(int device, const void* a, const void* b, const void* gamma, float eps, int64_t rows, int32_t d, int dtype,
                            void* out_sum, void* out_norm, unsigned short* pieces, void* stream) {
    TS_TRY(require({a, gamma, out_norm}));
    TS_TRY(pieces_from_f32(pieces, dtype));
    TS_TRY(storage_dtype(dtype));
    const NormPlan p = norm_plan(dtype, rows, d);
    if (!p.ok) return norm_refusal(p, d);
    TS_TRY(aligned16({a, b, gamma, out_sum, out_norm}, "buffers must be 16-byte aligned"));
    if (rows == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    return dispatch_norm(dtype, p, [&](auto dt, auto ln) {
        return launch<add_rmsnorm_kernel<dt, ln>>(p.grid, st, a, b, gamma, eps, rows, d, out_sum, out_norm, pieces);
    });
}

extern "C" int ts_add_rmsnorm(int device, const void* a, const void* b, const void* gamma, float eps, int64_t rows, int32_t d, int dtype,
                              void* out_sum, void* out_norm, void* stream) {
    return add_rmsnorm_impl(device, a, b, gamma, eps, rows, d, dtype, out_sum, out_norm, nullptr, stream);
}

extern "C" int ts_add_rmsnorm_pieces(int device, const void* a, const void* b, const void* gamma, float eps, int64_t rows, int32_t d,
                                     void* out_sum, void* out_norm, void* pieces, void* stream) {
    TS_TRY(require({pieces}));
    return add_rmsnorm_impl(device, a, b, gamma, eps, rows, d, TS_F32, out_sum, out_norm, (unsigned short*)pieces, stream);
}

extern "C" int ts_attention_float(int device, const void* qkv, const void* qkv_bias, const int64_t* attention_mask, int32_t batch, int32_t seq,
                                  int32_t q_heads, int32_t kv_heads, int32_t head_dim, int causal, float scale, void* out, void* pieces,
                                  void* stream) {
    if (!qkv || (!out && !pieces)) return fail(TS_ERR_INVALID, "NULL argument");
    TS_TRY(aligned16({qkv_bias}, "qkv_bias must be 16-byte aligned"));
    if (batch < 0 || seq < 1 || q_heads < 1 || kv_heads < 1 || q_heads % kv_heads != 0)
        return fail(TS_ERR_INVALID, "batch = %d, seq = %d, heads = %d over %d", batch, seq, q_heads, kv_heads);
    const AttnPlan p = attn_float_plan(batch, seq, q_heads, head_dim);
    if (!p.ok)
        return fail(TS_ERR_UNSUPPORTED, "head size %d / %d tokens: this kernel serves head sizes 64 / 128 / 256 up to 512 / 256 / 128 tokens",
                    head_dim, seq);
    if ((((uintptr_t)qkv | (uintptr_t)out) & 15) != 0 || (((uintptr_t)pieces) & 7) != 0)
        return fail(TS_ERR_INVALID, "qkv and out must be 16-byte aligned, pieces 8-byte");
    if (!(scale > 0.0f)) return fail(TS_ERR_INVALID, "scale must be positive");
    if (batch == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    const float scale_log2e = scale * 1.4426950408889634f;
    return dispatch_value<64, 128, 256>(head_dim, [&](auto hd) {
        return dispatch_value<0, 1>(causal != 0, [&](auto c) {
            // the limit: what the longest sequence of the head size needs
            return launch_lds<attention_f32_kernel<hd, c != 0>, attn_f32_lds_limit(hd)>(
                device, p.grid, p.block, p.lds, st, (const float*)qkv, attention_mask, batch, seq, q_heads, kv_heads, scale_log2e,
                (float*)out, (unsigned short*)pieces, (const float*)qkv_bias);
        });
    });
}

// window = 0: none (ts_attention_tiled).  A window that reaches the sequence's length hides nothing and takes the same instantiation
static int attention_tiled_impl(int device, const void* qkv, const void* qkv_bias, const int64_t* attention_mask, int32_t batch, int32_t seq,
                                int32_t q_heads, int32_t kv_heads, int32_t head_dim, int causal, int32_t window, float scale, void* out,
                                void* pieces, void* stream) {
    // ts_attention_float's checks, in its order, with its texts
    if (!qkv || (!out && !pieces)) return fail(TS_ERR_INVALID, "NULL argument");
    TS_TRY(aligned16({qkv_bias}, "qkv_bias must be 16-byte aligned"));
    if (batch < 0 || seq < 1 || q_heads < 1 || kv_heads < 1 || q_heads % kv_heads != 0)
        return fail(TS_ERR_INVALID, "batch = %d, seq = %d, heads = %d over %d", batch, seq, q_heads, kv_heads);
    const AttnTiledPlan p = attn_tiled_plan(batch, seq, q_heads, head_dim);
    if (!p.ok)
        return fail(TS_ERR_UNSUPPORTED,
                    "head size %d / %d tokens: this kernel serves head sizes 64 / 128 / 256 up to %d tokens (and 2^31 - 1 query blocks of %d)",
                    head_dim, seq, kAttnTiledMaxSeq, kAttnTiledQueries);
    if ((((uintptr_t)qkv | (uintptr_t)out) & 15) != 0 || (((uintptr_t)pieces) & 7) != 0)
        return fail(TS_ERR_INVALID, "qkv and out must be 16-byte aligned, pieces 8-byte");
    if (!(scale > 0.0f)) return fail(TS_ERR_INVALID, "scale must be positive");
    if (batch == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    const float scale_log2e = scale * 1.4426950408889634f;
    return dispatch_value<64, 128, 256>(head_dim, [&](auto hd) {
        return dispatch_value<0, 1>(causal != 0, [&](auto c) {
            return dispatch_value<0, 1>(window > 0 && window < seq, [&](auto w) {
                return launch_lds<attention_f32_tiled_kernel<hd, c != 0, w != 0>, attn_tiled_lds(hd)>(
                    device, p.grid, p.block, p.lds, st, (const float*)qkv, attention_mask, batch, seq, q_heads, kv_heads, scale_log2e,
                    (float*)out, (unsigned short*)pieces, (const float*)qkv_bias, (int)window);
            });
        });
    });
}

extern "C" int ts_attention_tiled(int device, const void* qkv, const void* qkv_bias, const int64_t* attention_mask, int32_t batch, int32_t seq,
                                  int32_t q_heads, int32_t kv_heads, int32_t head_dim, int causal, float scale, void* out, void* pieces,
                                  void* stream) {
    return attention_tiled_impl(device, qkv, qkv_bias, attention_mask, batch, seq, q_heads, kv_heads, head_dim, causal, 0, scale, out, pieces,
                                stream);
}

extern "C" int ts_attention_tiled_window(int device, const void* qkv, const void* qkv_bias, const int64_t* attention_mask, int32_t batch,
                                         int32_t seq, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int causal, int32_t window,
                                         float scale, void* out, void* pieces, void* stream) {
    if (window < 1) return fail(TS_ERR_INVALID, "window = %d must be at least 1", window);
    return attention_tiled_impl(device, qkv, qkv_bias, attention_mask, batch, seq, q_heads, kv_heads, head_dim, causal, window, scale, out,
                                pieces, stream);
}

// window = 0: none (ts_attention_flash), as in attention_tiled_impl
static int attention_flash_impl(int device, const void* qkv, const int64_t* attention_mask, int32_t batch, int32_t seq, int32_t q_heads,
                                int32_t kv_heads, int32_t head_dim, int causal, int32_t window, float scale, void* out, void* stream) {
    // ts_attention_tiled's checks, in its order, with its texts where they apply (no bias, no pieces)
    TS_TRY(require({qkv, out}));
    if (batch < 0 || seq < 1 || q_heads < 1 || kv_heads < 1 || q_heads % kv_heads != 0)
        return fail(TS_ERR_INVALID, "batch = %d, seq = %d, heads = %d over %d", batch, seq, q_heads, kv_heads);
    const AttnTiledPlan p = attn_bf16_tiled_plan(batch, seq, q_heads, head_dim);
    if (!p.ok)
        return fail(TS_ERR_UNSUPPORTED,
                    "head size %d / %d tokens: this kernel serves head sizes 64 / 128 / 256 up to %d tokens (and 2^31 - 1 query blocks of %d)",
                    head_dim, seq, kAttnBf16TiledMaxSeq, kAttnBf16TiledQueries);
    TS_TRY(aligned16({qkv, out}, "qkv and out must be 16-byte aligned"));
    if (!(scale > 0.0f)) return fail(TS_ERR_INVALID, "scale must be positive");
    if (batch == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    const float scale_log2e = scale * 1.4426950408889634f;
    return dispatch_value<64, 128, 256>(head_dim, [&](auto hd) {
        return dispatch_value<0, 1>(causal != 0, [&](auto c) {
            return dispatch_value<0, 1>(window > 0 && window < seq, [&](auto w) {
                return launch_lds<attention_bf16_tiled_kernel<hd, c != 0, w != 0>, attn_bf16_tiled_lds(hd)>(
                    device, p.grid, p.block, p.lds, st, (const unsigned short*)qkv, attention_mask, batch, seq, q_heads, kv_heads,
                    scale_log2e, (unsigned short*)out, (int)window);
            });
        });
    });
}

extern "C" int ts_attention_flash(int device, const void* qkv, const int64_t* attention_mask, int32_t batch, int32_t seq, int32_t q_heads,
                                 int32_t kv_heads, int32_t head_dim, int causal, float scale, void* out, void* stream) {
    return attention_flash_impl(device, qkv, attention_mask, batch, seq, q_heads, kv_heads, head_dim, causal, 0, scale, out, stream);
}

extern "C" int ts_attention_flash_window(int device, const void* qkv, const int64_t* attention_mask, int32_t batch, int32_t seq,
                                        int32_t q_heads, int32_t kv_heads, int32_t head_dim, int causal, int32_t window, float scale,
                                        void* out, void* stream) {
    if (window < 1) return fail(TS_ERR_INVALID, "window = %d must be at least 1", window);
    return attention_flash_impl(device, qkv, attention_mask, batch, seq, q_heads, kv_heads, head_dim, causal, window, scale, out, stream);
}

extern "C" int ts_attention_gqa(int device, const void* qkv, const int64_t* attention_mask, int32_t batch, int32_t seq, int32_t q_heads,
                               int32_t kv_heads, int32_t head_dim, int causal, void* out, void* stream) {
    TS_TRY(require({qkv, out}));
    if (batch < 0 || seq < 1 || q_heads < 1 || kv_heads < 1 || q_heads % kv_heads != 0)
        return fail(TS_ERR_INVALID, "batch = %d, seq = %d, heads = %d over %d", batch, seq, q_heads, kv_heads);
    const AttnPlan p = attn_gqa_plan(batch, seq, q_heads, kv_heads, head_dim);
    if (!p.ok)
        return fail(TS_ERR_UNSUPPORTED, "head size %d / %d tokens: this kernel serves head size 128 and at most %d tokens", head_dim, seq,
                    kAttnGqaRowsMaxSeq);
    TS_TRY(aligned16({qkv, out}, "qkv and out must be 16-byte aligned"));
    if (batch == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    const unsigned short* in = (const unsigned short*)qkv;
    unsigned short* o = (unsigned short*)out;
    return dispatch_value<0, 1>(causal != 0, [&](auto c) {
        return dispatch_value<1, 2, 3, 4, 5, 6, 7, 8>(p.tiles, [&](auto t) {
            if constexpr (t <= kAttnGqaMaxSeq / 16) {
                return launch_lds<attention_gqa_kernel<t, c != 0>>(device, p.grid, p.block, p.lds, st, in, attention_mask, batch, seq,
                                                                         q_heads, kv_heads, o);
            } else {
                // 65 .. 128 tokens: one query tile at a time against K fragments in registers and a V^T image in LDS that the R query
                // heads of a key / value group (R waves of one workgroup) share
                return dispatch_value<1, 2, 4>(p.r, [&](auto r) {
                    static_assert(attn_gqa_rows_lds(t, r) <= 160 * 1024, "the image and the waves' tiles fit the CU's LDS");
                    return launch_lds<attention_gqa_rows_kernel<t, c != 0, r>>(device, p.grid, p.block, p.lds, st, in, attention_mask,
                                                                                       batch, seq, q_heads, kv_heads, o);
                });
            }
        });
    });
}

static int qk_norm_rope_launch(int device, void* qkv, const void* q_weight, const void* k_weight, const void* cos_table,
                               const void* sin_table, float eps, int64_t tokens, int32_t seq, int32_t q_heads, int32_t kv_heads,
                               int32_t head_dim, int dtype, bool gemma, void* stream) {
    TS_TRY(require({qkv, q_weight, k_weight, cos_table, sin_table}));
    TS_TRY(storage_dtype(dtype));
    if (tokens < 0 || seq < 1 || q_heads < 1 || kv_heads < 1) return fail(TS_ERR_INVALID, "bad shape");
    if (head_dim != (gemma ? 256 : 128))
        return fail(TS_ERR_UNSUPPORTED, "head size %d: this kernel serves head size %d", head_dim, gemma ? 256 : 128);
    TS_TRY(aligned16({qkv, q_weight, k_weight, cos_table, sin_table}, "buffers must be 16-byte aligned"));
    if (tokens == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    const unsigned grid = qk_norm_rope_grid(dtype, tokens, q_heads, kv_heads, head_dim);
    return dispatch_value<0, 1>(dtype, [&](auto dt) {
        return dispatch_value<0, 1>(gemma, [&](auto g) {
            return launch<qk_norm_rope_kernel<dt, g != 0 ? 256 : 128, g != 0>>(grid, st, qkv, q_weight, k_weight, cos_table, sin_table, eps, tokens,
                                                                                   seq, q_heads, kv_heads);
        });
    });
}

extern "C" int ts_qk_norm_rope(int device, void* qkv, const void* q_weight, const void* k_weight, const void* cos_table,
                               const void* sin_table, float eps, int64_t tokens, int32_t seq, int32_t q_heads, int32_t kv_heads,
                               int32_t head_dim, int dtype, void* stream) {
    return qk_norm_rope_launch(device, qkv, q_weight, k_weight, cos_table, sin_table, eps, tokens, seq, q_heads, kv_heads, head_dim, dtype,
                               false, stream);
}

extern "C" int ts_gemma_qk_norm_rope(int device, void* qkv, const void* q_weight, const void* k_weight, const void* cos_table,
                                     const void* sin_table, float eps, int64_t tokens, int32_t seq, int32_t q_heads, int32_t kv_heads,
                                     int32_t head_dim, int dtype, void* stream) {
    return qk_norm_rope_launch(device, qkv, q_weight, k_weight, cos_table, sin_table, eps, tokens, seq, q_heads, kv_heads, head_dim, dtype,
                               true, stream);
}

static int gemma_norm_impl(int device, const void* y, const void* x, const void* w_post, const void* w_next, float eps, int64_t rows,
                           int32_t d, int dtype, void* out_sum, void* out_norm, unsigned short* pieces, void* stream) {
    if (!x || !w_next || !out_norm || (y && !w_post)) return fail(TS_ERR_INVALID, "NULL argument");
    TS_TRY(pieces_from_f32(pieces, dtype));
    TS_TRY(storage_dtype(dtype));
    const NormPlan p = norm_plan(dtype, rows, d);
    if (!p.ok) return norm_refusal(p, d);
    TS_TRY(aligned16({y, x, w_post, w_next, out_sum, out_norm}, "buffers must be 16-byte aligned"));
    if (rows == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    return dispatch_norm(dtype, p, [&](auto dt, auto ln) {
        return launch<gemma_norm_kernel<dt, ln>>(p.grid, st, y, x, w_post, w_next, eps, rows, d, out_sum, out_norm, pieces);
    });
}

extern "C" int ts_gemma_norm(int device, const void* y, const void* x, const void* w_post, const void* w_next, float eps, int64_t rows,
                             int32_t d, int dtype, void* out_sum, void* out_norm, void* stream) {
    return gemma_norm_impl(device, y, x, w_post, w_next, eps, rows, d, dtype, out_sum, out_norm, nullptr, stream);
}

extern "C" int ts_gemma_norm_pieces(int device, const void* y, const void* x, const void* w_post, const void* w_next, float eps,
                                    int64_t rows, int32_t d, void* out_sum, void* out_norm, void* pieces, void* stream) {
    TS_TRY(require({pieces}));
    return gemma_norm_impl(device, y, x, w_post, w_next, eps, rows, d, TS_F32, out_sum, out_norm, (unsigned short*)pieces, stream);
}

extern "C" int ts_act_pieces(int device, const void* x, const void* bias, int64_t rows, int32_t n, int kind, void* pieces, void* stream) {
    TS_TRY(require({x, pieces}));
    TS_TRY(aligned16({bias}, "bias must be 16-byte aligned"));
    if (rows < 0 || n < 4 || n % 4 || kind < 0 || kind > 2) return fail(TS_ERR_INVALID, "n = %d must be a multiple of 4, kind 0 / 1 / 2", n);
    if ((((uintptr_t)x) & 15) != 0 || (((uintptr_t)pieces) & 7) != 0) return fail(TS_ERR_INVALID, "x must be 16-byte, pieces 8-byte aligned");
    if (rows == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    return dispatch_value<0, 1, 2>(kind, [&](auto k) {
        return launch<act_pieces_kernel<k>>(elementwise_grid(rows * (n / 4)), st, (const float*)x, rows, n, (unsigned short*)pieces, (const float*)bias);
    });
}

static int gated_act_launch(int device, const void* gate_up, int64_t rows, int32_t inter, int dtype, bool gelu_tanh, void* out, void* stream) {
    TS_TRY(require({gate_up, out}));
    TS_TRY(storage_dtype(dtype));
    const int vec = enc_vec(dtype);
    if (rows < 0 || inter < vec || inter % vec) return fail(TS_ERR_INVALID, "inter = %d must be a multiple of %d", inter, vec);
    TS_TRY(aligned16({gate_up, out}, "buffers must be 16-byte aligned"));
    if (rows == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    const unsigned grid = elementwise_grid(rows * (inter / vec));
    return dispatch_value<0, 1>(dtype, [&](auto dt) {
        if (gelu_tanh) return launch<geglu_kernel<dt>>(grid, st, gate_up, rows, inter, out);
        return launch<swiglu_kernel<dt>>(grid, st, gate_up, rows, inter, out);
    });
}

extern "C" int ts_split_pieces(int device, const void* x, int64_t rows, int32_t k, int pattern, void* out, void* stream) {
    TS_TRY(require({x, out}));
    if (rows < 0 || k < 4 || k % 4 || (pattern != 0 && pattern != 1)) return fail(TS_ERR_INVALID, "k = %d must be a multiple of 4, pattern 0 or 1", k);
    if ((((uintptr_t)x) & 15) != 0 || (((uintptr_t)out) & 7) != 0) return fail(TS_ERR_INVALID, "x must be 16-byte, out 8-byte aligned");
    if (rows == 0) return TS_OK;
    hipStream_t st;
    TS_TRY(enter_device(device, stream, &st));
    return dispatch_value<0, 1>(pattern, [&](auto pat) {
        return launch<split3_kernel<pat>>(elementwise_grid(rows * (k / 4)), st, (const float*)x, rows, k, (unsigned short*)out);
    });
}

extern "C" int ts_swiglu(int device, const void* gate_up, int64_t rows, int32_t inter, int dtype, void* out, void* stream) {
    return gated_act_launch(device, gate_up, rows, inter, dtype, false, out, stream);
}

extern "C" int ts_geglu(int device, const void* gate_up, int64_t rows, int32_t inter, int dtype, void* out, void* stream) {
    return gated_act_launch(device, gate_up, rows, inter, dtype, true, out, stream);
}
