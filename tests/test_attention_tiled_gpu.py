"""ts_attention_tiled (theoremsearch_amd/csrc/kernels_attention_tiled.h): ts_attention_float with V^T fed through LDS in chunks of
keys, for heads of 64 / 128 / 256 at any length up to 32,768 tokens.
1. Wherever both entries serve a shape they return the same bits: every length next to a 16-token tile edge, a 64-query block edge
   and a chunk edge, causal and not, under every mask kind, context and pieces, into guarded buffers.
2. Past ts_attention_float's limits: against fp64 on N(0, 1.5^2) inputs, under the masks of encoder_common and two made here (a
   whole chunk of left padding; right padding that leaves one key).
3. The refusals, with real device pointers.
4. The fused fp32 forwards of the Qwen3 and Gemma3 stand-ins take it where they took torch's attention before: with
   scaled_dot_product_attention patched to raise, the forward completes.
Every output the tests allocate lies in a sentinel-filled buffer whose margins must come back untouched."""
import ctypes as C

import pytest
import torch

import encoder_common as ec
from theoremsearch_amd import _ffi
from theoremsearch_amd import fused_forward as ff

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
HEADS = ((2, 2, 64), (4, 2, 128), (3, 1, 256))                # (query heads, key / value heads, head size)
OLD_LIMIT = ff._FLOAT_ATTENTION_MAX_SEQ
CHUNK = ff._TILED_CHUNK
# |context - fp64| on N(0, 1.5^2) inputs.  Up to 512 tokens: the project's bound for ts_attention_float (test_mirrors_gpu.py,
# test_encoder_edges_gpu.py).  Beyond: measured on an MI355X at 513 / 1025 / 2049 tokens (profiles/HISTORY.md), at most half of
# 2e-5 for every head shape, so the same 2e-5 - a factor 2 to spare, as tests/test_encoder_ref_cpu.py keeps.  That scalar comes
# from the kernel itself; the bound that does not is tests/attention_f32_common.py's (per element, in units of 2^-24 (A + |want|),
# from a model of the arithmetic), which tests/test_attention_f32_gpu.py holds at 1,025 and 2,049 tokens too
BOUND, BOUND_LONG = 2e-5, 2e-5


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, qkv, mask, B, S, hq, hkv, hd, causal, scale, out, pieces, bias=None):
    return getattr(_ffi.load(), name)(0, P(qkv), P(bias), P(mask), B, S, hq, hkv, hd, 1 if causal else 0, scale, P(out), P(pieces), stream())


def guarded_pair(B, S, hq, hd):
    return ec.guarded((B, S, hq * hd), F32), ec.guarded((B * S, 3 * hq * hd), BF16, align=8)


def guarded_split(x):
    rows, k = x.shape
    out = ec.guarded((rows, 3 * k), BF16, align=8)
    _ffi.check(_ffi.load().ts_split_pieces(0, P(x), rows, k, 0, P(out), stream()))
    return out


def has_key_rows(mask, B, S, causal):
    """[B x S] bool: the query rows with at least one allowed key (encoder_common.attention_ref's rule, without the arithmetic)."""
    keys = torch.ones((B, S), dtype=torch.bool, device="cuda") if mask is None else mask != 0
    return (keys.cumsum(1) > 0) if causal else keys.any(1, keepdim=True).expand(B, S)


# ---- 1. the same bits as ts_attention_float -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hq,hkv,hd", HEADS, ids=lambda v: str(v))
def test_tiled_and_float_attention_return_the_same_bits(hq, hkv, hd, capsys):
    B, scale, Cn = 3, hd ** -0.5, CHUNK[hd]
    g = torch.Generator(device="cpu").manual_seed(31000 + hd)
    lengths = sorted({1, 15, 16, 17, 63, 64, 65, Cn - 1, Cn, Cn + 1, 2 * Cn + 1, OLD_LIMIT[hd]})
    assert max(lengths) == OLD_LIMIT[hd]
    cases = zero_rows = 0
    for S in lengths:
        qkv = (torch.randn(B, S, (hq + 2 * hkv) * hd, generator=g) * 1.5).cuda()
        bias = torch.randn((hq + 2 * hkv) * hd, generator=g).cuda()
        masks = ec.attention_masks(B, S, g)
        assert tuple(masks) == ec.ATTN_MASK_KINDS
        for kind, mask in masks.items():
            mask = None if mask is None else mask.cuda()
            for causal in (False, True):
                # the projection's bias: once per head shape and causal flag, at the length with a ragged last chunk
                for b in ((None, bias) if (S == 2 * Cn + 1 and kind == "left") else (None,)):
                    tag = (hq, hkv, hd, S, kind, causal, b is not None)
                    f_out, f_pieces = guarded_pair(B, S, hq, hd)
                    t_out, t_pieces = guarded_pair(B, S, hq, hd)
                    _ffi.check(call("ts_attention_float", qkv, mask, B, S, hq, hkv, hd, causal, scale, f_out, f_pieces, b))
                    _ffi.check(call("ts_attention_tiled", qkv, mask, B, S, hq, hkv, hd, causal, scale, t_out, t_pieces, b))
                    torch.cuda.synchronize()
                    # every element was written (the sentinel is NaN) and every one holds the other entry's bits
                    assert torch.isfinite(t_out).all() and torch.isfinite(f_out).all(), tag
                    assert torch.equal(ec.bits(t_out), ec.bits(f_out)), (tag, int((ec.bits(t_out) != ec.bits(f_out)).sum()))
                    assert torch.equal(ec.bits(t_pieces), ec.bits(f_pieces)), tag
                    ec.assert_margins(f_out, f_pieces, t_out, t_pieces)
                    has_key = has_key_rows(mask, B, S, causal)
                    if not has_key.all():
                        for t in (t_out, f_out, t_pieces.view(B, S, -1), f_pieces.view(B, S, -1)):
                            assert not t[~has_key].any(), (tag, "a query row without an allowed key must be zeros")
                        zero_rows += int((~has_key).sum())
                    cases += 1
    assert zero_rows > 0
    with capsys.disabled():
        print(f"\nts_attention_tiled {hq}/{hkv} x {hd}: {cases} cases at {len(lengths)} lengths up to {OLD_LIMIT[hd]} tokens bit for bit "
              f"ts_attention_float's, {zero_rows} keyless rows exactly zero", end="")


# ---- 2. past the old limits, against fp64 ---------------------------------------------------------------------------------------------
def long_masks(B, S, Cn, g):
    """none, right, left, holes, keyless of encoder_common, and two more: left padding of Cn + 3 keys on every sequence (a whole
    chunk without an allowed key in front of every query), right padding that leaves key 0 alone."""
    m = ec.attention_masks(B, S, g)
    out = {k: m[k] for k in ("none", "right", "left", "holes", "keyless")}
    ar = torch.arange(S)[None, :].expand(B, S)
    out["chunk_of_padding"] = (ar >= Cn + 3).to(torch.int64)
    out["one_key"] = (ar == 0).to(torch.int64)
    return out


def check_against_fp64(hq, hkv, hd, B, S, kind, mask, causal, qkv, worst):
    scale = hd ** -0.5
    tag = (hq, hkv, hd, B, S, kind, causal)
    want, has_key = ec.attention_ref(qkv, mask, hq, hkv, hd, causal, scale)
    out, pieces = guarded_pair(B, S, hq, hd)
    only = ec.guarded((B * S, 3 * hq * hd), BF16, align=8)
    _ffi.check(call("ts_attention_tiled", qkv, mask, B, S, hq, hkv, hd, causal, scale, out, pieces))
    _ffi.check(call("ts_attention_tiled", qkv, mask, B, S, hq, hkv, hd, causal, scale, None, only))
    sp = guarded_split(out.view(B * S, -1))
    torch.cuda.synchronize()
    ec.assert_margins(out, pieces, only, sp)
    assert torch.isfinite(out).all(), tag
    if has_key.any():
        err = (out.double() - want)[has_key].abs().max().item()
        key = "long" if S > 512 else "short"
        worst[key] = max(worst[key], err)
        assert err < (BOUND_LONG if S > 512 else BOUND), (tag, err)
    if not has_key.all():
        assert not out[~has_key].any() and not pieces.view(B, S, -1)[~has_key].any(), (tag, "a query row without an allowed key must be zeros")
    assert ec.same_bits(pieces, sp), (tag, "pieces differ from ts_split_pieces(context)")
    assert ec.same_bits(only, pieces), (tag, "pieces without the context differ")
    return int((~has_key).sum())


@pytest.mark.parametrize("hq,hkv,hd", HEADS, ids=lambda v: str(v))
def test_tiled_attention_past_the_old_limits_matches_fp64(hq, hkv, hd, capsys):
    B, Cn, old = 3, CHUNK[hd], OLD_LIMIT[hd]
    g = torch.Generator(device="cpu").manual_seed(32000 + hd)
    worst, zero_rows = {"short": 0.0, "long": 0.0}, 0
    lengths = sorted({old + 1, old + 17, 3 * Cn + 5, 512, 513, 1025})
    for S in lengths:
        qkv = (torch.randn(B, S, (hq + 2 * hkv) * hd, generator=g) * 1.5).cuda()
        for kind, mask in long_masks(B, S, Cn, g).items():
            mask = None if mask is None else mask.cuda()
            for causal in (False, True):
                zero_rows += check_against_fp64(hq, hkv, hd, B, S, kind, mask, causal, qkv, worst)
    # one long sequence: 33 query blocks, 17 / 33 / 65 chunks
    S = 2049
    qkv = (torch.randn(1, S, (hq + 2 * hkv) * hd, generator=g) * 1.5).cuda()
    holes = long_masks(1, S, Cn, g)["holes"].cuda()
    zero_rows += check_against_fp64(hq, hkv, hd, 1, S, "holes", holes, True, qkv, worst)
    assert zero_rows > 0
    # the projection's bias added on the way in: the answer on qkv + bias, within the 1e-5 of ts_attention_float's test
    S = old + 17
    qb = torch.randn(B, S, (hq + 2 * hkv) * hd, generator=g).cuda()
    bias = torch.randn((hq + 2 * hkv) * hd, generator=g).cuda()
    mask = long_masks(B, S, Cn, g)["left"].cuda()
    for causal in (False, True):
        want = ff.attention_tiled(qb + bias, mask, B, S, hq, hkv, hd, causal, hd ** -0.5)[0]
        got, gp = ff.attention_tiled(qb, mask, B, S, hq, hkv, hd, causal, hd ** -0.5, want_pieces=True, bias=bias)
        ref, has_key = ec.attention_ref(qb, mask, hq, hkv, hd, causal, hd ** -0.5, bias=bias)
        sp = guarded_split(got.view(B * S, -1))
        torch.cuda.synchronize()
        assert (got - want).abs().max().item() < 1e-5, (hd, S, causal)
        assert (got.double() - ref)[has_key].abs().max().item() < BOUND and not got[~has_key].any(), (hd, S, causal)
        assert ec.same_bits(gp, sp), (hd, S, causal)
    with capsys.disabled():
        print(f"\nts_attention_tiled {hq}/{hkv} x {hd} against fp64: worst error {worst['short']:.3e} up to 512 tokens ({worst['short'] / BOUND:.3f} of "
              f"{BOUND:g}), {worst['long']:.3e} at 513 / 1025 / 2049 tokens ({worst['long'] / BOUND_LONG:.3f} of {BOUND_LONG:g}); "
              f"{zero_rows} keyless rows exactly zero", end="")


# ---- 3. refusals, with device pointers ----------------------------------------------------------------------------------------------
def test_tiled_attention_refusals_on_the_device():
    qkv = torch.zeros(4096, dtype=F32, device="cuda")
    out = torch.zeros(4096 + 4, dtype=F32, device="cuda")

    def ok(**kw):
        args = dict(qkv=qkv, mask=None, B=1, S=4, hq=1, hkv=1, hd=64, causal=False, scale=0.125, out=out[:256], pieces=None)
        return call("ts_attention_tiled", **{**args, **kw})

    assert ok() == 0
    assert ok(S=32769) == ec.TS_ERR_UNSUPPORTED and b"32768 tokens" in _ffi.load().ts_last_error()
    assert ok(hd=32) == ec.TS_ERR_UNSUPPORTED and b"head size" in _ffi.load().ts_last_error()
    assert ok(out=out[1:257]) == ec.TS_ERR_INVALID and b"16-byte aligned" in _ffi.load().ts_last_error()
    assert ok(out=None) == ec.TS_ERR_INVALID and ok(scale=0.0) == ec.TS_ERR_INVALID and ok(hq=3, hkv=2) == ec.TS_ERR_INVALID
    torch.cuda.synchronize()
    assert not out[256:].any()


# ---- 4. the forwards take it ------------------------------------------------------------------------------------------------------
# The Qwen3 stand-in's bound is test_long_corpus_texts_take_the_float_attention_in_the_fused_fp32_forward's: 1e-4 of the largest
# hidden value on real tokens.  The Gemma3 stand-in had no bound at these lengths: measured on an MI355X (profiles/HISTORY.md) the
# worst difference is below half of 1e-4, so the same 1e-4 is pinned.  fp32_gemm="bf16x3": the full-depth test's hmax <= 1e-3.
FORWARD_TOL = {"blas": 1e-4, "bf16x3": 1e-3}
FAMILIES = {"qwen3": ("Qwen/Qwen3-Embedding-0.6B", 3, 5, 256, 512), "gemma3": ("google/embeddinggemma-300m", 1, 3, 128, 511)}


@pytest.mark.parametrize("gemm", ("blas", "bf16x3"))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_fused_fp32_forwards_take_the_tiled_attention_past_the_old_limits(family, gemm, monkeypatch, capsys):
    from theoremsearch_amd.encoder import SentenceEncoder
    name, num, den, lo, hi = FAMILIES[family]
    texts = [("Let $X_%d$ be a compact Hausdorff space and $f$ a continuous map. " % i) * (12 + 3 * (i % 7)) for i in range(9)]
    texts = [t[: len(t) * num // den] for t in texts]
    enc = SentenceEncoder(name, num_layers=2, allow_random_init=True, dtype=torch.float32, fp32_gemm=gemm)
    assert enc._fused is not None and enc._fused.pieces == (gemm == "bf16x3")
    tok = {k: v.cuda() for k, v in enc._tokenize(texts).items()}
    ids, am = tok["input_ids"], tok["attention_mask"]
    S = ids.shape[1]
    assert lo < S <= hi and not bool(am.all()), S
    if family == "gemma3":
        assert S < int(enc.model.config.sliding_window)
    called = []
    real_op = _ffi.encoder_op
    monkeypatch.setattr(_ffi, "encoder_op", lambda op, *a: (called.append(op), real_op(op, *a))[1])

    def no_sdpa(*a, **kw):
        raise AssertionError("torch's scaled_dot_product_attention was called")

    with torch.inference_mode():
        want = enc.model(input_ids=ids, attention_mask=am).last_hidden_state
        with monkeypatch.context() as m:
            m.setenv("TS_ENCODER_ATTENTION", "0")
            torch_way = enc.forward_hidden(ids, am)
            assert "ts_attention_tiled" not in called and "ts_attention_float" not in called
            m.setattr(torch.nn.functional, "scaled_dot_product_attention", no_sdpa)
            with pytest.raises(AssertionError, match="scaled_dot_product_attention was called"):
                enc.forward_hidden(ids, am)                                # TS_ENCODER_ATTENTION=0 still takes torch's attention
        del called[:]
        with monkeypatch.context() as m:
            m.setattr(torch.nn.functional, "scaled_dot_product_attention", no_sdpa)
            got = enc.forward_hidden(ids, am)                              # ... and without it nothing does
    assert called.count("ts_attention_tiled") == len(enc.model.layers) and "ts_attention_float" not in called, called
    assert "ts_split_pieces" not in called, "bf16x3: the attention writes the pieces of its output itself"
    real = am.bool()
    scale = want[real].abs().max().item()
    d_own, d_torch = (want - got)[real].abs().max().item() / scale, (torch_way - got)[real].abs().max().item() / scale
    with capsys.disabled():
        print(f"\n{family} stand-in, fp32 / {gemm}, {S} tokens: fused forward with ts_attention_tiled against the model's own {d_own:.3e}, "
              f"against torch's attention {d_torch:.3e} of the largest hidden value (bound {FORWARD_TOL[gemm]:g})", end="")
    assert d_own < FORWARD_TOL[gemm] and d_torch < FORWARD_TOL[gemm], (family, gemm, S, d_own, d_torch)
