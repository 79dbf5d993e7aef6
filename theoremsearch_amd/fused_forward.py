"""Fused forwards of the three encoder families the reference embeds with: the GEMMs stay
in the BLAS library (north_star: the encoder forward is PyTorch-ROCm), everything around them is kernels of libtsearch.

* `FusedBertForward`   - BERT family: math-similarity/Bert-MLM_arXiv-MP-class_zbMath (compare_embeddings.py:11-12,
  app_create_embeddings.py:8, parsed_papers_to_vector_rds/embeddings.py:29)
* `FusedQwen3Forward`  - Qwen/Qwen3-Embedding-0.6B, the production embedder (streamlit_app.py:55, ec2/generate_embeddings/embedders.py:1-4)
* `FusedGemma3Forward` - google/embeddinggemma-300m, the `gemma` alias of ec2/generate_embeddings/embedders.py:1-4

Each keeps the model's weights (stacked projections are rebuilt when a parameter changes), its order of operations and the
roundings of the modules it replaces; `covers(model)` says whether a loaded model can take the fused path, `SentenceEncoder`
(encoder.py) asks.  Tested against the models' own forwards in tests/test_mirrors_gpu.py.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _ffi


def split_pieces(x: torch.Tensor, pattern: int) -> torch.Tensor:
    """``x`` fp32 ``[rows x k]`` -> bf16 ``[rows x 3k]``: ``[hi | lo | hi]`` (pattern 0, activations) or ``[hi | hi | lo]``
    (pattern 1, weights), hi = bf16(x), lo = bf16(x - hi) (``ts_split_pieces``)."""
    x = x.contiguous()
    rows, k = x.shape
    out = torch.empty((rows, 3 * k), dtype=torch.bfloat16, device=x.device)
    _ffi.encoder_op("ts_split_pieces", x, x, rows, k, pattern, out)
    return out


def pieces_linear(x: torch.Tensor, w_pieces: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear(x, w, bias)`` for fp32 ``x`` and an fp32 weight given as its pieces (``split_pieces(w, 1)``), computed on the
    bf16 matrix pipe: ONE bf16 GEMM with fp32 accumulation over the three-fold depth (hipBLASLt through ``torch.mm(..,
    out_dtype=float32)``) = x_hi w_hi + x_lo w_hi + x_hi w_lo - the fp32 product up to ~2^-17 |x||w| per term, at a third of
    the bf16 GEMM rate instead of the fp32 matrix rate (157 TF against 2.5 PF dense on MI355X).  The encoder forward at the
    reference's fp32 storage (SentenceTransformer(name) without a dtype, streamlit_app.py:55,173) with ``fp32_gemm="bf16x3"``."""
    shape = x.shape
    x3 = split_pieces(x.reshape(-1, shape[-1]), 0)
    if bias is not None:
        y = torch.addmm(bias, x3, w_pieces.t(), out_dtype=torch.float32)
    else:
        y = torch.mm(x3, w_pieces.t(), out_dtype=torch.float32)
    return y.view(*shape[:-1], w_pieces.shape[0])


def pieces_mm(x_pieces: torch.Tensor, w_pieces: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The GEMM of `pieces_linear` on operands that already are pieces (``[rows x 3k]`` bf16 each): fp32 ``[rows x n]``."""
    if bias is not None:
        return torch.addmm(bias, x_pieces, w_pieces.t(), out_dtype=torch.float32)
    return torch.mm(x_pieces, w_pieces.t(), out_dtype=torch.float32)


def act_pieces(x: torch.Tensor, kind: int, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 activation straight into pieces (``ts_act_pieces``): kind 0 = gelu (erf) of ``[rows x n]``; 1 = silu(gate) * up,
    2 = gelu_tanh(gate) * up of ``[rows x 2n]``; ``bias`` (over the input's width) is added first.  Returns bf16 ``[rows x 3n]``."""
    x = x.contiguous()
    rows = x.numel() // x.shape[-1]
    n = x.shape[-1] if kind == 0 else x.shape[-1] // 2
    out = torch.empty((rows, 3 * n), dtype=torch.bfloat16, device=x.device)
    _ffi.encoder_op("ts_act_pieces", x, x, bias, rows, n, kind, out)
    return out


def attention_float(qkv: torch.Tensor, key_mask: Optional[torch.Tensor], B: int, S: int, hq: int, hkv: int, hd: int, causal: bool,
                    scale: float, want_pieces: bool = False, bias: Optional[torch.Tensor] = None, want_context: bool = True):
    """fp32 attention of at most 512 / 256 / 128 tokens (head size 64 / 128 / 256) on the exact-fp32 matrix instructions, straight from the stacked projection's output
    ``qkv [B x S x (hq + 2 hkv) hd]`` (``ts_attention_float``; ``bias``: the projection's bias when its GEMM ran without one):
    ``(context fp32 [B x S x hq hd] - None with ``want_context=False`` - , its bf16 pieces or None)``."""
    qkv = qkv.contiguous()
    ctx = torch.empty((B, S, hq * hd), dtype=torch.float32, device=qkv.device) if (want_context or not want_pieces) else None
    pieces = torch.empty((B * S, 3 * hq * hd), dtype=torch.bfloat16, device=qkv.device) if want_pieces else None
    _ffi.encoder_op("ts_attention_float", qkv, qkv, bias, key_mask, B, S, hq, hkv, hd, 1 if causal else 0, float(scale), ctx, pieces)
    return ctx, pieces


def attention_tiled(qkv: torch.Tensor, key_mask: Optional[torch.Tensor], B: int, S: int, hq: int, hkv: int, hd: int, causal: bool,
                    scale: float, want_pieces: bool = False, bias: Optional[torch.Tensor] = None, want_context: bool = True,
                    window: int = 0):
    """`attention_float` at any length from 1 to 32,768 tokens (``ts_attention_tiled``: V^T through LDS in chunks of keys, a
    workgroup per 64 queries): the same arguments, the same return value, the same bits where both serve a shape.  ``window`` > 0:
    a query reads the keys at a distance below ``window`` only (``ts_attention_tiled_window``, which walks only their chunks)."""
    qkv = qkv.contiguous()
    ctx = torch.empty((B, S, hq * hd), dtype=torch.float32, device=qkv.device) if (want_context or not want_pieces) else None
    pieces = torch.empty((B * S, 3 * hq * hd), dtype=torch.bfloat16, device=qkv.device) if want_pieces else None
    if window:
        _ffi.encoder_op("ts_attention_tiled_window", qkv, qkv, bias, key_mask, B, S, hq, hkv, hd, 1 if causal else 0, int(window),
                        float(scale), ctx, pieces)
    else:
        _ffi.encoder_op("ts_attention_tiled", qkv, qkv, bias, key_mask, B, S, hq, hkv, hd, 1 if causal else 0, float(scale), ctx, pieces)
    return ctx, pieces


def attention_bf16(qkv: torch.Tensor, key_mask: Optional[torch.Tensor], B: int, S: int, hq: int, hkv: int, hd: int, causal: bool,
                   scale: float, window: int = 0) -> torch.Tensor:
    """bf16 attention at any length from 1 to 32,768 tokens for heads of 64 / 128 / 256 (``ts_attention_flash``: K and V through LDS in
    chunks of keys, a workgroup per 64 queries, online softmax), straight from the stacked projection's output ``qkv [B x S x (hq + 2
    hkv) hd]``: the context, bf16 ``[B x S x hq hd]``.  ``window`` > 0: a query reads the keys at a distance below ``window`` only
    (``ts_attention_flash_window``, which walks only their chunks)."""
    qkv = qkv.contiguous()
    ctx = torch.empty((B, S, hq * hd), dtype=torch.bfloat16, device=qkv.device)
    if window:
        _ffi.encoder_op("ts_attention_flash_window", qkv, qkv, key_mask, B, S, hq, hkv, hd, 1 if causal else 0, int(window), float(scale), ctx)
    else:
        _ffi.encoder_op("ts_attention_flash", qkv, qkv, key_mask, B, S, hq, hkv, hd, 1 if causal else 0, float(scale), ctx)
    return ctx


# The limits of the library's kernels (csrc/encoder_plan.h; tests/test_encoder_ref_cpu.py holds each against the library's refusals)
_FLOAT_ATTENTION_MAX_SEQ = {64: 512, 128: 256, 256: 128}      # what fits the CU's LDS as V^T (attn_f32_max_seq)
_TILED_MAX_SEQ = 32768                                        # ts_attention_tiled: tokens (kAttnTiledMaxSeq)
_TILED_CHUNK = {64: 128, 128: 64, 256: 32}                    # keys per staged chunk of V^T by head size (attn_tiled_chunk)
# Where the forwards take ts_attention_tiled: only where it was at least as fast as torch's attention with its layout copies
# (tools/attention_tiled_timing.py, profiles/attention_tiled_timing.jsonl, 256 sequences, us per call, tiled against torch):
# heads of 128 (Qwen3, causal) 2,229 / 8,184 at 384 tokens, 5,685 / 12,900 at 512, 5,523 / 11,552 at 64 x 1,024: every length;
# heads of 256 (Gemma3) 628 / 768 at 192 tokens, 1,085 / 1,114 at 256, but 2,373 / 2,105 at 384: up to 256 tokens, torch's beyond;
# heads of 64 (BERT) have no length past ts_attention_float's 512 (the position table ends there): not measured, every length.
_TILED_ROUTED_MAX_SEQ = {64: _TILED_MAX_SEQ, 128: _TILED_MAX_SEQ, 256: 256}
_SHORT_HEAD, _SHORT_MAX_SEQ = 64, 128                         # ts_attention_short (bf16): head size, tokens (kAttnRowsMaxSeq)
_GQA_HEAD, _GQA_MAX_SEQ = 128, 128                            # ts_attention_gqa (bf16): head size, tokens (kAttnGqaRowsMaxSeq)
_BF16_TILED_MAX_SEQ = 32768                                   # ts_attention_flash: tokens (kAttnBf16TiledMaxSeq)
_BF16_TILED_CHUNK = {64: 128, 128: 64, 256: 32}               # keys per staged chunk of K and V by head size (attn_bf16_tiled_chunk)
# Where the bf16 forwards take ts_attention_flash: up to the longest measured length at which it was at least as fast as what the
# forward did before - torch's attention with its layout copies - there and at every shorter measured length; 0: not routed
# (tools/attention_bf16_timing.py, profiles/attention_bf16_timing.jsonl, 256 sequences - 64 from 1,024 tokens on -, us per call,
# ts_attention_flash against torch).  Two tables, because torch runs two different kernels.
# A batch WITH padding (torch gets the forward's additive mask and leaves its flash kernel):
# heads of 256 (Gemma3) 20 / 153 at 32 tokens, 99 / 527 at 128, 331 / 1,356 at 256, 1,355 / 4,042 at 512: every measured length;
# heads of 128 (Qwen3, causal) 265 / 2,097 at 129, 728 / 4,703 at 256, 2,523 / 14,721 at 512, 8,735 / 47,648 at 64 x 2,048: every one;
# heads of 64 (BERT) 265 / 312 at 192, 448 / 514 at 256, but 930 / 609 at 384: up to 256.
_BF16_TILED_ROUTED_MAX_SEQ = {64: 256, 128: 2048, 256: 512}
# A batch WITHOUT padding (no mask: torch's tuned flash kernel, is_causal for Qwen3):
# heads of 256: 18.4 / 21.2 at 32 tokens in isolation, 30.7 / 29.8 at 64 (and 259 / 186 at 256) - but the encoder-in-loop step at 32
# tokens (bench.py --workload c5 --encoder gemma --encoder-dtype bf16, same box, three alternating pairs) ran 5.83 ms with it against
# 5.70 without: the 3 us a layer do not survive the forward, not routed;
# heads of 128: 202 / 604 at 129, 501 / 719 at 256, 712 / 1,161 at 384, but 1,702 / 1,672 at 512 (5,913 / 2,885 at 64 x 2,048): up to 384;
# heads of 64: 180 / 152 at 192 already: not routed.
_BF16_TILED_ROUTED_MAX_SEQ_NO_PADDING = {64: 0, 128: 384, 256: 0}
# Where a sliding layer of FusedGemma3Forward (S > window) takes the windowed entries, by head size: up to the longest measured
# length at which the entry was at least as fast as what the forward runs otherwise - torch's attention with the additive mask of
# padding and window and its layout copies - there and at every shorter measured length; 0: not routed
# (tools/attention_window_timing.py, profiles/attention_window_timing.jsonl: heads of 256, 3 / 1 heads, window 257, 256 sequences -
# 64 from 1,024 tokens on -, us per call with padding, windowed entry / unwindowed parent entry / torch;
# tests/test_attention_window_timing_cpu.py derives both tables from the rows).  One table per type: torch gets an additive mask
# with padding and without, and runs the same kernel (1,893 and 1,885 us at 258 tokens).
# bf16 (ts_attention_flash_window): 454 / 429 / 1,893 at 258 tokens, 711 / 785 / 2,627 at 384, 1,251 / 1,361 / 4,092 at 512,
# 698 / 1,163 / 3,462 at 64 x 1,024, 1,442 / 4,782 / 12,353 at 64 x 2,048: every measured length.
# fp32 (ts_attention_tiled_window): 1,632 / 1,630 / 1,706 at 258 tokens, but 2,664 / 3,107 / 2,298 at 384 and 4,860 / 5,506 / 3,613 at
# 512: up to 258.  (It wins again at 64 x 1,024 - 2,711 / 5,312 / 3,144 - and 64 x 2,048 - 5,409 / 20,552 / 11,460 -, where the window
# leaves a half and a quarter of the chunks; the rule does not count a win behind a loss.)
_WINDOW_ROUTED_MAX_SEQ_BF16 = {256: 2048}
_WINDOW_ROUTED_MAX_SEQ_F32 = {256: 258}
_NORM_MAX_VECS = 256                                          # the norm kernels: 16-byte accesses per row (64 lanes x kLnMax)


def float_attention_applies(x: torch.Tensor, S: int, hd: int) -> bool:
    """fp32 hidden states, a head size the kernel serves and a sequence whose V^T fits the LDS (512 / 256 / 128 tokens for heads
    of 64 / 128 / 256); TS_ENCODER_ATTENTION=0 keeps torch's attention."""
    return (x.dtype == torch.float32 and S <= _FLOAT_ATTENTION_MAX_SEQ.get(hd, 0) and os.environ.get("TS_ENCODER_ATTENTION", "1") != "0")


def fp32_attention_kind(x: torch.Tensor, S: int, hd: int) -> Optional[str]:
    """Which of the library's fp32 attentions serves fp32 hidden states ``x`` at ``S`` tokens and head size ``hd``: ``"float"``
    where `float_attention_applies` (ts_attention_float, routing unchanged), ``"tiled"`` beyond that up to 32,768 tokens
    (ts_attention_tiled) - for heads of 256 up to 256 tokens only: at 384 it measured slower than torch's attention, see
    `_TILED_ROUTED_MAX_SEQ` -, ``None`` - torch's attention - otherwise, for another head size, for bf16 or with
    TS_ENCODER_ATTENTION=0."""
    if float_attention_applies(x, S, hd):
        return "float"
    if x.dtype == torch.float32 and S <= _TILED_ROUTED_MAX_SEQ.get(hd, 0) and os.environ.get("TS_ENCODER_ATTENTION", "1") != "0":
        return "tiled"
    return None


_FP32_ATTENTION = {"float": attention_float, "tiled": attention_tiled}


def bf16_attention_kind(x: torch.Tensor, S: int, hd: int, causal: bool, padding: bool = True) -> Optional[str]:
    """Which of the library's bf16 attentions serves bf16 hidden states ``x`` at ``S`` tokens and head size ``hd``: ``"short"``
    (ts_attention_short: heads of 64, not causal, at most 128 tokens) and ``"gqa"`` (ts_attention_gqa: heads of 128, causal, at most
    128 tokens, contiguous hidden states) exactly where the forwards took them before; ``"tiled"`` (ts_attention_flash) where
    `_BF16_TILED_ROUTED_MAX_SEQ` routes the head size - `_BF16_TILED_ROUTED_MAX_SEQ_NO_PADDING` for a batch the caller knows to
    have no padding (``padding=False``) -, heads of 64 / 128 past 128 tokens only; ``None`` - torch's attention - otherwise, for
    another head size, for fp32 or with TS_ENCODER_ATTENTION=0.  TS_ENCODER_FLASH=0 takes out the ``"tiled"`` answer alone: the
    routing of the commit before ts_attention_flash, for same-box comparisons."""
    if x.dtype != torch.bfloat16 or os.environ.get("TS_ENCODER_ATTENTION", "1") == "0":
        return None
    if hd == _SHORT_HEAD and not causal and S <= _SHORT_MAX_SEQ:
        return "short"
    if hd == _GQA_HEAD and causal and S <= _GQA_MAX_SEQ and x.is_contiguous():
        return "gqa"
    if hd in (_SHORT_HEAD, _GQA_HEAD) and S <= max(_SHORT_MAX_SEQ, _GQA_MAX_SEQ):
        return None
    if os.environ.get("TS_ENCODER_FLASH", "1") == "0":       # same-box A/B against torch's attention (tools/ab_env.sh)
        return None
    routed = _BF16_TILED_ROUTED_MAX_SEQ if padding else _BF16_TILED_ROUTED_MAX_SEQ_NO_PADDING
    if S <= min(routed.get(hd, 0), _BF16_TILED_MAX_SEQ):
        return "tiled"
    return None


class FusedBertForward:
    """The forward of a BERT-family encoder (``BertModel``: what ``math-similarity/Bert-MLM_arXiv-MP-class_zbMath`` is,
    compare_embeddings.py:11) with the launches that do not pay for themselves folded together:

    * query / key / value projections as ONE GEMM over the concatenated weight (three 8,192 x 768 x 768 GEMMs fill the
      chip a third each: 24 us apiece against 41 us for the fused one, measured per layer at 256 x 32 tokens);
    * ``LayerNorm(dense_out + input)`` as ONE HIP kernel (``ts_add_layernorm``) instead of an add and a layer_norm launch
      (18 + 7 us of device time twice per layer);
    * the input layer (three embedding gathers, two adds, LayerNorm) as ONE HIP kernel (``ts_embed_layernorm``);
    * for bf16 models with 64-wide heads and at most 128 tokens, the attention as ONE wave per (sequence, head)
      (``ts_attention_short``; ``TS_ENCODER_ATTENTION=0`` keeps ``scaled_dot_product_attention``).

    Same weights, same order of operations, exact erf GELU (whatever ``config.hidden_act`` names); the attention is
    ``scaled_dot_product_attention`` with the padding mask, as the model's own ``sdpa`` path.  Used on a GPU for bf16 / fp32
    models whose config this form covers; anything else runs the model's own forward."""

    def __init__(self, model):
        cfg = model.config
        self.model, self.cfg = model, cfg
        self.heads = cfg.num_attention_heads
        self.eps = float(cfg.layer_norm_eps)
        from transformers.activations import ACT2FN
        self.act = ACT2FN[cfg.hidden_act] if isinstance(cfg.hidden_act, str) else cfg.hidden_act
        self.pieces = False           # fp32 models: the GEMMs on the bf16 matrix pipe from bf16 pieces (pieces_linear)
        self._stamp = None
        self._refresh()

    def _sources(self):
        """The parameters the stacked projection weights are copies of."""
        for layer in self.model.encoder.layer:
            att = layer.attention.self
            yield from (att.query.weight, att.key.weight, att.value.weight, att.query.bias, att.key.bias, att.value.bias)

    def _refresh(self):
        """(Re)build the stacked query / key / value weights when the model's own have changed (load_state_dict, .to(dtype),
        an edit in place): the other weights are live references, the stacked ones are copies."""
        stamp = tuple((p.data_ptr(), p._version, p.dtype) for p in self._sources()) + (self.pieces,)
        if stamp == self._stamp:
            return
        self._stamp = stamp
        self.layers = []
        for layer in self.model.encoder.layer:
            att, so = layer.attention.self, layer.attention.output
            self.layers.append({
                "wqkv": torch.cat([att.query.weight, att.key.weight, att.value.weight], dim=0).contiguous(),
                "bqkv": torch.cat([att.query.bias, att.key.bias, att.value.bias], dim=0).contiguous(),
                "wo": so.dense.weight, "bo": so.dense.bias, "ln1": so.LayerNorm,
                "w1": layer.intermediate.dense.weight, "b1": layer.intermediate.dense.bias,
                "w2": layer.output.dense.weight, "b2": layer.output.dense.bias, "ln2": layer.output.LayerNorm,
            })
            if self.pieces and self.layers[-1]["wo"].dtype == torch.float32:
                L = self.layers[-1]
                for name in ("wqkv", "wo", "w1", "w2"):
                    L[name + "_p"] = split_pieces(L[name].detach(), 1)

    @staticmethod
    def covers(model) -> bool:
        cfg = getattr(model, "config", None)
        if cfg is None or getattr(cfg, "model_type", "") != "bert" or not hasattr(model, "encoder"):
            return False
        if getattr(cfg, "position_embedding_type", "absolute") != "absolute" or getattr(cfg, "is_decoder", False):
            return False
        p = next(model.parameters())
        return (p.is_cuda and p.dtype in (torch.float32, torch.bfloat16) and cfg.hidden_size % 8 == 0 and cfg.hidden_size <= _NORM_MAX_VECS * 4
                and cfg.hidden_size % cfg.num_attention_heads == 0)

    def _embed(self, input_ids: torch.Tensor, token_type_ids: Optional[torch.Tensor]) -> torch.Tensor:
        """BertEmbeddings (word + token type + position, LayerNorm; dropout is the identity in eval) as ONE HIP kernel
        (``ts_embed_layernorm``) instead of three gathers, two adds and a layer_norm launch.  Anything the kernel's form does not
        cover (a sequence longer than the position table, a module without the three tables) runs the module itself."""
        emb = self.model.embeddings
        tables = [getattr(emb, n, None) for n in ("word_embeddings", "position_embeddings", "token_type_embeddings")]
        ln = getattr(emb, "LayerNorm", None)
        B, S = input_ids.shape
        if any(t is None for t in tables) or ln is None or S > tables[1].weight.shape[0] or input_ids.dtype != torch.int64:
            return emb(input_ids=input_ids, token_type_ids=token_type_ids)
        w, p, t = (m.weight for m in tables)
        ids = input_ids.contiguous()
        tt = token_type_ids.contiguous().to(torch.int64) if token_type_ids is not None else None
        H = w.shape[1]
        out = torch.empty((B, S, H), dtype=w.dtype, device=w.device)
        _ffi.encoder_op("ts_embed_layernorm", w, ids, tt, w, p, t, w.shape[0], p.shape[0], t.shape[0], ln.weight, ln.bias, self.eps,
                        B * S, S, H, 1 if w.dtype == torch.bfloat16 else 0, out)
        return out

    def _attention(self, qkv: torch.Tensor, key_mask: Optional[torch.Tensor], B: int, S: int) -> torch.Tensor:
        qkv = qkv.contiguous()
        out = torch.empty((B, S, self.heads * _SHORT_HEAD), dtype=torch.bfloat16, device=qkv.device)
        _ffi.encoder_op("ts_attention_short", qkv, qkv, key_mask, B, S, self.heads, _SHORT_HEAD, out)
        return out

    def _add_ln_pieces(self, a: torch.Tensor, b: torch.Tensor, ln, a_bias: Optional[torch.Tensor] = None):
        """`_add_ln` of fp32 operands (``a + a_bias + b``) that also writes the pieces of its output: ``(out fp32, pieces bf16
        [rows x 3d])``."""
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty_like(a)
        rows, d = a.numel() // a.shape[-1], a.shape[-1]
        pieces = torch.empty((rows, 3 * d), dtype=torch.bfloat16, device=a.device)
        _ffi.encoder_op("ts_add_layernorm_pieces", a, a, a_bias, b, ln.weight, ln.bias, self.eps, rows, d, out, pieces)
        return out, pieces

    def _add_ln(self, a: torch.Tensor, b: torch.Tensor, ln) -> torch.Tensor:
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty_like(a)
        rows, d = a.numel() // a.shape[-1], a.shape[-1]
        _ffi.encoder_op("ts_add_layernorm", a, a, b, ln.weight, ln.bias, self.eps, rows, d, 1 if a.dtype == torch.bfloat16 else 0, out)
        return out

    def __call__(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, token_type_ids: Optional[torch.Tensor] = None,
                 no_padding: bool = False):
        F = torch.nn.functional
        self._refresh()
        x = self._embed(input_ids, token_type_ids)
        B, S, H = x.shape
        hd = H // self.heads
        # padding keys are never attended to: ONE additive mask per forward (a boolean mask is expanded to a bias inside every
        # scaled_dot_product_attention call: two fill launches per layer); none at all when the caller knows the batch has no
        # padding (every sequence as long as the batch: 50 instead of 60 us per layer for projections + attention)
        # short sequences (one sentence per query: app_showcase_model.py:92) of a bf16 model with 64-wide heads: the attention as
        # ONE wave per (sequence, head), straight from the fused projection to the context layout (``ts_attention_short``)
        kind16 = bf16_attention_kind(x, S, hd, False, not no_padding)        # bf16: ts_attention_short, past 128 tokens ts_attention_flash where routed
        short = kind16 is not None
        # (the most negative finite value, not -inf: a sequence without a single token would otherwise soften to NaN)
        kind32 = fp32_attention_kind(x, S, hd)               # fp32: the library's fp32 attention (ts_attention_float / _tiled)
        short32 = kind32 is not None
        mask = None if (no_padding or short or short32) else torch.zeros((B, 1, 1, S), dtype=x.dtype, device=x.device).masked_fill_(
            ~attention_mask[:, None, None, :].to(torch.bool), torch.finfo(x.dtype).min)
        key_mask = None if (no_padding or not (short or short32)) else attention_mask.to(torch.int64).contiguous()
        pieces = self.pieces and x.dtype == torch.float32 and "wo_p" in self.layers[0]
        if pieces:
            return self._forward_pieces(x, mask, key_mask, kind32, B, S, H, hd)
        for L in self.layers:
            qkv = F.linear(x, L["wqkv"], L["bqkv"])
            if kind16 == "short":
                ctx = self._attention(qkv, key_mask, B, S)
            elif kind16 == "tiled":
                ctx = attention_bf16(qkv, key_mask, B, S, self.heads, self.heads, hd, False, hd ** -0.5)
            elif short32:
                ctx = _FP32_ATTENTION[kind32](qkv, key_mask, B, S, self.heads, self.heads, hd, False, hd ** -0.5)[0]
            else:
                qkv = qkv.view(B, S, 3, self.heads, hd).permute(2, 0, 3, 1, 4)
                ctx = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], attn_mask=mask)
                ctx = ctx.transpose(1, 2).reshape(B, S, H)
            x = self._add_ln(F.linear(ctx, L["wo"], L["bo"]), x, L["ln1"])
            h = self.act(F.linear(x, L["w1"], L["b1"]))
            x = self._add_ln(F.linear(h, L["w2"], L["b2"]), x, L["ln2"])
        return x

    def _forward_pieces(self, x: torch.Tensor, mask: Optional[torch.Tensor], key_mask: Optional[torch.Tensor], kind32: Optional[str],
                        B: int, S: int, H: int, hd: int) -> torch.Tensor:
        """The layers of an fp32 model with every GEMM on the bf16 matrix pipe (``fp32_gemm="bf16x3"``): weights are pieces
        (``_refresh``), every activation reaches its GEMM as pieces written by the kernel that produced it (LayerNorm, GELU, the
        library's fp32 attention ``kind32``; without one, torch's attention output passes through ``ts_split_pieces``)."""
        F = torch.nn.functional
        exact_gelu = self.cfg.hidden_act == "gelu"
        xp = split_pieces(x.view(B * S, H), 0)
        for L in self.layers:
            # every GEMM runs WITHOUT its bias: the kernel that reads its output adds it on the way in (torch.addmm with an output
            # type first copies the broadcast bias into the result: one more pass over every GEMM's output)
            qkv = pieces_mm(xp, L["wqkv_p"])
            if kind32:                 # the attention writes the pieces of its output itself
                cp = _FP32_ATTENTION[kind32](qkv, key_mask, B, S, self.heads, self.heads, hd, False, hd ** -0.5, want_pieces=True, bias=L["bqkv"], want_context=False)[1]
            else:
                qkv = (qkv + L["bqkv"]).view(B, S, 3, self.heads, hd).permute(2, 0, 3, 1, 4)
                ctx = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], attn_mask=mask)
                cp = split_pieces(ctx.transpose(1, 2).reshape(B * S, H), 0)
            x, xp = self._add_ln_pieces(pieces_mm(cp, L["wo_p"]).view(B, S, H), x, L["ln1"], a_bias=L["bo"])
            h = pieces_mm(xp, L["w1_p"])
            hp = act_pieces(h, 0, bias=L["b1"]) if exact_gelu else split_pieces(self.act(h + L["b1"]), 0)
            x, xp = self._add_ln_pieces(pieces_mm(hp, L["w2_p"]).view(B, S, H), x, L["ln2"], a_bias=L["b2"])
        return x


class FusedQwen3Forward:
    """The forward of a Qwen3-family encoder (``Qwen3Model``: what ``Qwen/Qwen3-Embedding-0.6B`` is, the embedder of the
    production app, streamlit_app.py:55) with everything around its GEMMs as kernels of libtsearch:

    * query / key / value projections as ONE GEMM over the stacked weight, gate / up projections as ONE;
    * ``residual + sublayer`` followed by the next RMSNorm as ONE kernel (``ts_add_rmsnorm``: PyTorch runs an add and six
      launches per norm, twice per layer);
    * the per-head RMSNorm of queries and keys + the rotary embedding as ONE kernel, in place (``ts_qk_norm_rope``:
      twenty-two launches per layer in PyTorch);
    * ``silu(gate) * up`` as ONE kernel (``ts_swiglu``).

    * causal grouped-query attention of short sequences (bf16, up to 128 tokens) as ONE kernel straight from the stacked
      projection (``ts_attention_gqa``: one wave per (sequence, query head); torch's flash-attention launch took 202 us per
      layer at 256 sequences x 32 tokens, 504 us at 128); longer bf16 sequences keep ``scaled_dot_product_attention``;
    * in fp32 the library's fp32 attention at every length: ``ts_attention_float`` up to 256 tokens, ``ts_attention_tiled`` beyond
      (`fp32_attention_kind`) - no additive mask, no layout copies, and in the pieces path the pieces straight from the kernel.

    Same weights, same order of operations, the roundings of the modules replaced."""

    def __init__(self, model):
        cfg = model.config
        self.model, self.cfg = model, cfg
        self.hq, self.hkv, self.hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        self.eps = float(cfg.rms_norm_eps)
        self.pieces = False           # fp32 models: the GEMMs on the bf16 matrix pipe from bf16 pieces (pieces_linear)
        self._stamp = None
        self._gqa_native = True
        self._refresh()

    def _sources(self):
        for layer in self.model.layers:
            att, mlp = layer.self_attn, layer.mlp
            yield from (att.q_proj.weight, att.k_proj.weight, att.v_proj.weight, mlp.gate_proj.weight, mlp.up_proj.weight)

    def _refresh(self):
        stamp = tuple((p.data_ptr(), p._version, p.dtype) for p in self._sources()) + (self.pieces,)
        if stamp == self._stamp:
            return
        self._stamp = stamp
        self.layers = []
        for layer in self.model.layers:
            att, mlp = layer.self_attn, layer.mlp
            self.layers.append({
                "wqkv": torch.cat([att.q_proj.weight, att.k_proj.weight, att.v_proj.weight], dim=0).contiguous(),
                "wo": att.o_proj.weight, "qn": att.q_norm.weight, "kn": att.k_norm.weight,
                "wgu": torch.cat([mlp.gate_proj.weight, mlp.up_proj.weight], dim=0).contiguous(), "wd": mlp.down_proj.weight,
                "ln1": layer.input_layernorm.weight, "ln2": layer.post_attention_layernorm.weight,
            })
            if self.pieces and self.layers[-1]["wo"].dtype == torch.float32:
                L = self.layers[-1]
                for name in ("wqkv", "wo", "wgu", "wd"):
                    L[name + "_p"] = split_pieces(L[name].detach(), 1)

    @staticmethod
    def covers(model) -> bool:
        cfg = getattr(model, "config", None)
        if cfg is None or getattr(cfg, "model_type", "") != "qwen3" or not hasattr(model, "layers"):
            return False
        if getattr(cfg, "attention_bias", False) or getattr(cfg, "head_dim", 0) != 128:
            return False
        if any(t != "full_attention" for t in (getattr(cfg, "layer_types", None) or [])):
            return False
        if getattr(cfg, "hidden_act", "silu") != "silu":
            return False
        p = next(model.parameters())
        vec = 8 if p.dtype == torch.bfloat16 else 4
        return (p.is_cuda and p.dtype in (torch.float32, torch.bfloat16) and cfg.hidden_size % vec == 0 and
                cfg.hidden_size <= _NORM_MAX_VECS * vec and cfg.intermediate_size % vec == 0 and
                cfg.num_attention_heads % cfg.num_key_value_heads == 0)

    def _add_rmsnorm(self, a: torch.Tensor, b: Optional[torch.Tensor], gamma: torch.Tensor, want_sum: bool):
        d = a.shape[-1]
        rows = a.numel() // d
        out = torch.empty_like(a)
        new_res = torch.empty_like(a) if (want_sum and b is not None) else None
        _ffi.encoder_op("ts_add_rmsnorm", a, a, b, gamma, self.eps, rows, d, 1 if a.dtype == torch.bfloat16 else 0, new_res, out)
        return (new_res if new_res is not None else a), out

    def _add_rmsnorm_pieces(self, a: torch.Tensor, b: Optional[torch.Tensor], gamma: torch.Tensor, want_sum: bool):
        """`_add_rmsnorm` of fp32 operands that also writes the pieces of the normalised rows: ``(residual, normed, pieces)``."""
        d = a.shape[-1]
        rows = a.numel() // d
        out = torch.empty_like(a)
        new_res = torch.empty_like(a) if (want_sum and b is not None) else None
        pieces = torch.empty((rows, 3 * d), dtype=torch.bfloat16, device=a.device)
        _ffi.encoder_op("ts_add_rmsnorm_pieces", a, a, b, gamma, self.eps, rows, d, new_res, out, pieces)
        return (new_res if new_res is not None else a), out, pieces

    def _sdpa(self, qkv: torch.Tensor, mask: Optional[torch.Tensor], B: int, S: int, nq: int, nkv: int, hd: int) -> torch.Tensor:
        """torch's attention on the stacked projection (longer sequences, fp32): causal, grouped-query, as the model's own sdpa path."""
        F = torch.nn.functional
        q = qkv[..., :nq].view(B, S, self.hq, hd).transpose(1, 2)
        k = qkv[..., nq:nq + nkv].view(B, S, self.hkv, hd).transpose(1, 2)
        v = qkv[..., nq + nkv:].view(B, S, self.hkv, hd).transpose(1, 2)
        ctx = None
        if self._gqa_native:
            try:
                ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, is_causal=mask is None, enable_gqa=True)
            except (RuntimeError, TypeError):
                self._gqa_native = False
        if ctx is None:
            rep = self.hq // self.hkv
            ctx = F.scaled_dot_product_attention(q, k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1),
                                                 attn_mask=mask, is_causal=mask is None)
        return ctx.transpose(1, 2).reshape(B, S, nq)

    def __call__(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, token_type_ids: Optional[torch.Tensor] = None,
                 no_padding: bool = False):
        F = torch.nn.functional
        self._refresh()
        m = self.model
        x = m.embed_tokens(input_ids).contiguous()
        B, S, H = x.shape
        dt = 1 if x.dtype == torch.bfloat16 else 0
        pos = torch.arange(S, device=x.device).unsqueeze(0)              # positions count from the left edge, padding included
        cos, sin = m.rotary_emb(x, pos)                                  # [1 x S x 128] of the model's type
        cos, sin = cos[0].contiguous(), sin[0].contiguous()
        mask = None
        # short sequences in bf16: the library's own causal grouped-query attention (TS_ENCODER_ATTENTION=0 keeps torch's)
        kind16 = bf16_attention_kind(x, S, self.hd, True, not no_padding)    # ts_attention_gqa, past 128 tokens ts_attention_flash where routed
        short = kind16 is not None
        kind32 = fp32_attention_kind(x, S, self.hd)           # fp32: the library's fp32 attention (causal, grouped-query)
        short32 = kind32 is not None
        key_mask = None if (no_padding or not (short or short32)) else attention_mask.to(torch.int64).contiguous()
        if not no_padding and not short and not short32:
            # causal, and padding keys are never attended to (the most negative finite value: rows of padding stay finite)
            neg = torch.finfo(x.dtype).min
            causal = torch.ones((S, S), dtype=torch.bool, device=x.device).tril_()
            keep = causal[None, None] & attention_mask[:, None, None, :].to(torch.bool)
            mask = torch.zeros((B, 1, S, S), dtype=x.dtype, device=x.device).masked_fill_(~keep, neg)
        nq, nkv, hd = self.hq * self.hd, self.hkv * self.hd, self.hd
        pieces = self.pieces and x.dtype == torch.float32 and "wo_p" in self.layers[0]
        if pieces:
            # every GEMM on the bf16 matrix pipe from pieces: weights split once (`_refresh`), activations written as pieces by
            # the kernel that produces them (RMSNorm, SwiGLU); only torch's attention output passes through ts_split_pieces
            _, h, hp = self._add_rmsnorm_pieces(x, None, self.layers[0]["ln1"], False)
            for li, L in enumerate(self.layers):
                qkv = pieces_mm(hp, L["wqkv_p"]).view(B, S, -1)
                _ffi.encoder_op("ts_qk_norm_rope", x, qkv, L["qn"], L["kn"], cos, sin, self.eps, B * S, S, self.hq, self.hkv, hd, dt)
                if short32:
                    cp = _FP32_ATTENTION[kind32](qkv, key_mask, B, S, self.hq, self.hkv, hd, True, hd ** -0.5, want_pieces=True, want_context=False)[1]
                else:
                    cp = split_pieces(self._sdpa(qkv, mask, B, S, nq, nkv, hd).reshape(B * S, nq), 0)
                x, h, hp = self._add_rmsnorm_pieces(x, pieces_mm(cp, L["wo_p"]).view(B, S, H), L["ln2"], True)
                ap = act_pieces(pieces_mm(hp, L["wgu_p"]), 1)
                last = li + 1 == len(self.layers)
                gamma = m.norm.weight if last else self.layers[li + 1]["ln1"]
                x, h, hp = self._add_rmsnorm_pieces(x, pieces_mm(ap, L["wd_p"]).view(B, S, H), gamma, not last)
            return h
        h = self._add_rmsnorm(x, None, self.layers[0]["ln1"], False)[1]
        for li, L in enumerate(self.layers):
            qkv = F.linear(h, L["wqkv"])
            _ffi.encoder_op("ts_qk_norm_rope", x, qkv, L["qn"], L["kn"], cos, sin, self.eps, B * S, S, self.hq, self.hkv, hd, dt)
            if kind16 == "tiled":
                ctx = attention_bf16(qkv, key_mask, B, S, self.hq, self.hkv, hd, True, hd ** -0.5)
            elif short:
                # one wave per (sequence, query head), straight from the stacked projection's output (ts_attention_gqa)
                ctx = torch.empty((B, S, nq), dtype=x.dtype, device=x.device)
                _ffi.encoder_op("ts_attention_gqa", x, qkv, key_mask, B, S, self.hq, self.hkv, hd, 1, ctx)
            elif short32:
                ctx = _FP32_ATTENTION[kind32](qkv, key_mask, B, S, self.hq, self.hkv, hd, True, hd ** -0.5)[0]
            else:
                ctx = self._sdpa(qkv, mask, B, S, nq, nkv, hd)
            x, h = self._add_rmsnorm(x, F.linear(ctx, L["wo"]), L["ln2"], True)
            gu = F.linear(h, L["wgu"])
            inter = gu.shape[-1] // 2
            act = torch.empty((B, S, inter), dtype=x.dtype, device=x.device)
            _ffi.encoder_op("ts_swiglu", x, gu, B * S, inter, dt, act)
            last = li + 1 == len(self.layers)
            gamma = m.norm.weight if last else self.layers[li + 1]["ln1"]
            x, h = self._add_rmsnorm(x, F.linear(act, L["wd"]), gamma, not last)
        return h


class FusedGemma3Forward:
    """The forward of a Gemma3 text encoder with bidirectional attention (``Gemma3TextModel``: what
    ``google/embeddinggemma-300m`` is, the reference's second embedder, ec2/generate_embeddings/embedders.py:1-4) with everything
    around its GEMMs and its attention as kernels of libtsearch:

    * query / key / value projections as ONE GEMM over the stacked weight, gate / up projections as ONE;
    * the post-sublayer RMSNorm, the residual add and the pre-norm of the next sublayer as ONE kernel (``ts_gemma_norm``:
      PyTorch runs two norms of seven launches each and an add, twice per layer);
    * the per-head RMSNorm of queries and keys + the rotary embedding as ONE kernel, in place (``ts_gemma_qk_norm_rope``;
      sliding and full attention layers have their own cos / sin tables);
    * ``gelu_tanh(gate) * up`` as ONE kernel (``ts_geglu``).

    The attention (heads of 256, grouped-query) of a full-attention layer, and of a sliding layer whose window hides nothing
    (``S <= sliding_window``), is the library's in fp32 - ``ts_attention_float`` up to 128 tokens, ``ts_attention_tiled`` up to 256
    (`fp32_attention_kind`) -, ``ts_attention_flash`` in bf16 where `bf16_attention_kind` routes it, and
    ``scaled_dot_product_attention`` otherwise.  A sliding layer of a longer sequence (a query reads the keys at a distance below
    ``sliding_window``: 257 for ``embeddinggemma-300m``) takes ``ts_attention_flash_window`` / ``ts_attention_tiled_window`` where
    `_WINDOW_ROUTED_MAX_SEQ_BF16` / `_WINDOW_ROUTED_MAX_SEQ_F32` route its length, and ``scaled_dot_product_attention`` with one
    additive mask of the padding and the window, built once per forward, otherwise.  Same weights, same order of operations, the
    roundings of the modules replaced, at every length: the forward never hands a batch back to the model's own."""

    def __init__(self, model):
        cfg = model.config
        self.model, self.cfg = model, cfg
        self.hq, self.hkv, self.hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
        self.eps = float(cfg.rms_norm_eps)
        self.scaling = float(cfg.query_pre_attn_scalar) ** -0.5
        self.pieces = False           # fp32 models: the GEMMs on the bf16 matrix pipe from bf16 pieces (pieces_linear)
        self._stamp = None
        self._gqa_native = True
        self._refresh()

    def _sources(self):
        for layer in self.model.layers:
            att, mlp = layer.self_attn, layer.mlp
            yield from (att.q_proj.weight, att.k_proj.weight, att.v_proj.weight, mlp.gate_proj.weight, mlp.up_proj.weight)

    def _refresh(self):
        stamp = tuple((p.data_ptr(), p._version, p.dtype) for p in self._sources()) + (self.pieces,)
        if stamp == self._stamp:
            return
        self._stamp = stamp
        self.layers = []
        for layer in self.model.layers:
            att, mlp = layer.self_attn, layer.mlp
            self.layers.append({
                "wqkv": torch.cat([att.q_proj.weight, att.k_proj.weight, att.v_proj.weight], dim=0).contiguous(),
                "wo": att.o_proj.weight, "qn": att.q_norm.weight, "kn": att.k_norm.weight,
                "wgu": torch.cat([mlp.gate_proj.weight, mlp.up_proj.weight], dim=0).contiguous(), "wd": mlp.down_proj.weight,
                "ln_in": layer.input_layernorm.weight, "ln_post_attn": layer.post_attention_layernorm.weight,
                "ln_pre_ffn": layer.pre_feedforward_layernorm.weight, "ln_post_ffn": layer.post_feedforward_layernorm.weight,
                "type": att.layer_type,
            })
            if self.pieces and self.layers[-1]["wo"].dtype == torch.float32:
                L = self.layers[-1]
                for name in ("wqkv", "wo", "wgu", "wd"):
                    L[name + "_p"] = split_pieces(L[name].detach(), 1)

    @staticmethod
    def covers(model) -> bool:
        cfg = getattr(model, "config", None)
        if cfg is None or getattr(cfg, "model_type", "") != "gemma3_text" or not hasattr(model, "layers"):
            return False
        if not getattr(cfg, "use_bidirectional_attention", False) or getattr(cfg, "attention_bias", False):
            return False
        if getattr(cfg, "attn_logit_softcapping", None) or getattr(cfg, "head_dim", 0) != 256:
            return False
        if getattr(cfg, "hidden_activation", "") != "gelu_pytorch_tanh":
            return False
        p = next(model.parameters())
        vec = 8 if p.dtype == torch.bfloat16 else 4
        return (p.is_cuda and p.dtype in (torch.float32, torch.bfloat16) and cfg.hidden_size % vec == 0 and
                cfg.hidden_size <= _NORM_MAX_VECS * vec and cfg.intermediate_size % vec == 0 and
                cfg.num_attention_heads % cfg.num_key_value_heads == 0)

    def _norm(self, y: Optional[torch.Tensor], x: torch.Tensor, w_post: Optional[torch.Tensor], w_next: torch.Tensor, want_sum: bool):
        d = x.shape[-1]
        rows = x.numel() // d
        out = torch.empty_like(x)
        new_res = torch.empty_like(x) if (want_sum and y is not None) else None
        _ffi.encoder_op("ts_gemma_norm", x, y, x, w_post, w_next, self.eps, rows, d, 1 if x.dtype == torch.bfloat16 else 0, new_res, out)
        return (new_res if new_res is not None else x), out

    def _sdpa(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
        """torch's attention (where no kernel of the library is routed): the keys the additive ``mask`` leaves - every key, the
        real tokens, or those within a sliding layer's window -, grouped-query, Gemma3's own scaling."""
        F = torch.nn.functional
        if self._gqa_native:
            try:
                return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=self.scaling, enable_gqa=True)
            except (RuntimeError, TypeError):
                self._gqa_native = False
        rep = self.hq // self.hkv
        return F.scaled_dot_product_attention(q, k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1), attn_mask=mask,
                                              scale=self.scaling)

    def _norm_pieces(self, y: Optional[torch.Tensor], x: torch.Tensor, w_post: Optional[torch.Tensor], w_next: torch.Tensor, want_sum: bool):
        """`_norm` of fp32 operands that also writes the pieces of the pre-normed rows: ``(residual, normed, pieces)``."""
        d = x.shape[-1]
        rows = x.numel() // d
        out = torch.empty_like(x)
        new_res = torch.empty_like(x) if (want_sum and y is not None) else None
        pieces = torch.empty((rows, 3 * d), dtype=torch.bfloat16, device=x.device)
        _ffi.encoder_op("ts_gemma_norm_pieces", x, y, x, w_post, w_next, self.eps, rows, d, new_res, out, pieces)
        return (new_res if new_res is not None else x), out, pieces

    def __call__(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, token_type_ids: Optional[torch.Tensor] = None,
                 no_padding: bool = False):
        F = torch.nn.functional
        B, S = input_ids.shape
        self._refresh()
        m = self.model
        x = m.embed_tokens(input_ids).contiguous()                    # scaled by sqrt(hidden) in the storage type, as the module does
        dt = 1 if x.dtype == torch.bfloat16 else 0
        pos = torch.arange(S, device=x.device).unsqueeze(0)
        tables = {}
        for lt in set(self.cfg.layer_types):
            cos, sin = m.rotary_emb(x, pos, lt)                       # [1 x S x 256] of the model's type
            tables[lt] = (cos[0].contiguous(), sin[0].contiguous())
        mask = None
        kind32 = fp32_attention_kind(x, S, self.hd)           # fp32: the library's fp32 attention (every key visible, heads of 256)
        kind16 = bf16_attention_kind(x, S, self.hd, False, not no_padding)   # bf16: ts_attention_flash where routed
        short32 = kind32 is not None
        # the sliding layers hide keys once S > window: the windowed entries where routed, else torch's attention with ONE additive
        # mask of padding and window for all of them
        window = int(self.cfg.sliding_window or 0)
        windowed = 0 < window < S and any(L["type"] == "sliding_attention" for L in self.layers)
        win_routed = _WINDOW_ROUTED_MAX_SEQ_BF16 if x.dtype == torch.bfloat16 else _WINDOW_ROUTED_MAX_SEQ_F32
        win_lib = windowed and S <= win_routed.get(self.hd, 0) and os.environ.get("TS_ENCODER_ATTENTION", "1") != "0"
        key_mask = attention_mask.to(torch.int64).contiguous() if ((short32 or kind16 or win_lib) and not no_padding) else None
        neg = torch.finfo(x.dtype).min
        if not no_padding and not short32 and not kind16:
            mask = torch.zeros((B, 1, 1, S), dtype=x.dtype, device=x.device).masked_fill_(~attention_mask[:, None, None, :].to(torch.bool), neg)
        wmask = None
        if windowed and not win_lib:
            far = (pos[0, :, None] - pos[0, None, :]).abs() >= window        # [S x S]: |q - k| >= window
            hidden = far[None, None] if no_padding else far[None, None] | ~attention_mask[:, None, None, :].to(torch.bool)
            wmask = torch.zeros(hidden.shape, dtype=x.dtype, device=x.device).masked_fill_(hidden, neg)
        nq, nkv, hd = self.hq * self.hd, self.hkv * self.hd, self.hd
        pieces = self.pieces and x.dtype == torch.float32 and "wo_p" in self.layers[0]
        H = x.shape[-1]
        hp = None
        if pieces:
            _, h, hp = self._norm_pieces(None, x, None, self.layers[0]["ln_in"], False)
        else:
            h = self._norm(None, x, None, self.layers[0]["ln_in"], False)[1]
        for li, L in enumerate(self.layers):
            qkv = pieces_mm(hp, L["wqkv_p"]).view(B, S, -1) if pieces else F.linear(h, L["wqkv"])
            cos, sin = tables[L["type"]]
            _ffi.encoder_op("ts_gemma_qk_norm_rope", x, qkv, L["qn"], L["kn"], cos, sin, self.eps, B * S, S, self.hq, self.hkv, hd, dt)
            cp = None
            win = windowed and L["type"] == "sliding_attention"
            if win and win_lib and dt:
                ctx = attention_bf16(qkv, key_mask, B, S, self.hq, self.hkv, hd, False, self.scaling, window=window)
            elif win and win_lib:
                ctx, cp = attention_tiled(qkv, key_mask, B, S, self.hq, self.hkv, hd, False, self.scaling, want_pieces=pieces,
                                          want_context=not pieces, window=window)
            elif win:
                q = qkv[..., :nq].view(B, S, self.hq, hd).transpose(1, 2)
                k = qkv[..., nq:nq + nkv].view(B, S, self.hkv, hd).transpose(1, 2)
                v = qkv[..., nq + nkv:].view(B, S, self.hkv, hd).transpose(1, 2)
                ctx = self._sdpa(q, k, v, wmask).transpose(1, 2).reshape(B, S, nq)
            elif short32:
                ctx, cp = _FP32_ATTENTION[kind32](qkv, key_mask, B, S, self.hq, self.hkv, hd, False, self.scaling, want_pieces=pieces, want_context=not pieces)
            elif kind16 == "tiled":
                ctx = attention_bf16(qkv, key_mask, B, S, self.hq, self.hkv, hd, False, self.scaling)
            else:
                q = qkv[..., :nq].view(B, S, self.hq, hd).transpose(1, 2)
                k = qkv[..., nq:nq + nkv].view(B, S, self.hkv, hd).transpose(1, 2)
                v = qkv[..., nq + nkv:].view(B, S, self.hkv, hd).transpose(1, 2)
                ctx = self._sdpa(q, k, v, mask).transpose(1, 2).reshape(B, S, nq)
            last = li + 1 == len(self.layers)
            w_next = m.norm.weight if last else self.layers[li + 1]["ln_in"]
            if pieces:
                # GEMMs on the bf16 matrix pipe from pieces; the norms and the GeGLU write the pieces of what they produce
                if cp is None:
                    cp = split_pieces(ctx.reshape(B * S, nq), 0)
                x, h, hp = self._norm_pieces(pieces_mm(cp, L["wo_p"]).view(B, S, H), x, L["ln_post_attn"], L["ln_pre_ffn"], True)
                ap = act_pieces(pieces_mm(hp, L["wgu_p"]), 2)
                x, h, hp = self._norm_pieces(pieces_mm(ap, L["wd_p"]).view(B, S, H), x, L["ln_post_ffn"], w_next, not last)
                continue
            x, h = self._norm(F.linear(ctx, L["wo"]), x, L["ln_post_attn"], L["ln_pre_ffn"], True)
            gu = F.linear(h, L["wgu"])
            inter = gu.shape[-1] // 2
            act = torch.empty((B, S, inter), dtype=x.dtype, device=x.device)
            _ffi.encoder_op("ts_geglu", x, gu, B * S, inter, dt, act)
            x, h = self._norm(F.linear(act, L["wd"]), x, L["ln_post_ffn"], w_next, not last)
        return h
