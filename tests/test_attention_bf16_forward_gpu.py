"""The fused bf16 forwards of the BERT, Qwen3 and Gemma3 stand-ins (two layers, random weights) take ts_attention_flash wherever
fused_forward routes it (bf16_attention_kind: _BF16_TILED_ROUTED_MAX_SEQ for a batch with padding,
_BF16_TILED_ROUTED_MAX_SEQ_NO_PADDING for one without - the measured rows of profiles/attention_bf16_timing.jsonl): 129 and 200 tokens
for heads of 64 / 128, 32 and 200 for heads of 256, with right padding and - where that is routed - without.  With
scaled_dot_product_attention patched to raise the forward completes, calls the new entry once per layer, and agrees with the same
forward under TS_ENCODER_ATTENTION=0 (torch's attention) within the bf16 fused-against-own tolerance of tests/test_fulldepth_gpu.py
for that model: 0.08 (max) and 0.008 (mean) of the largest hidden value on the real tokens.  Cases the measurement does not route
(BERT and Gemma3 without padding) are not parametrised."""
import functools

import pytest
import torch

from theoremsearch_amd import _ffi
from theoremsearch_amd import fused_forward as ff

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
TOL = dict(hmax=0.08, hmean=0.008)                      # tests/test_fulldepth_gpu.py TOL[(family, "bf16")], the same for the three
FAMILIES = {"bert": ("math-similarity/Bert-MLM_arXiv-MP-class_zbMath", 64, False, (129, 200)),
            "qwen3": ("Qwen/Qwen3-Embedding-0.6B", 128, True, (129, 200)),
            "gemma3": ("google/embeddinggemma-300m", 256, False, (32, 200))}
CASES = tuple((family, S, padded) for family, (_, hd, causal, lengths) in sorted(FAMILIES.items()) for S in lengths for padded in (True, False)
              if (S <= (ff._BF16_TILED_ROUTED_MAX_SEQ if padded else ff._BF16_TILED_ROUTED_MAX_SEQ_NO_PADDING)[hd]))
B = 6


@functools.lru_cache(maxsize=None)
def encoder(family):
    from theoremsearch_amd.encoder import SentenceEncoder
    enc = SentenceEncoder(FAMILIES[family][0], num_layers=2, allow_random_init=True, dtype=BF16)
    assert enc._fused is not None
    return enc


def test_the_routed_cases_are_what_the_measurement_gives():
    assert set(CASES) == {("bert", 129, True), ("bert", 200, True), ("qwen3", 129, True), ("qwen3", 200, True), ("qwen3", 129, False),
                          ("qwen3", 200, False), ("gemma3", 32, True), ("gemma3", 200, True)}


@pytest.mark.parametrize("family,S,padded", CASES, ids=lambda v: str(v))
def test_fused_bf16_forward_takes_the_flash_attention(family, S, padded, monkeypatch, capsys):
    _, hd, causal, _ = FAMILIES[family]
    enc = encoder(family)
    layers = enc.model.encoder.layer if family == "bert" else enc.model.layers
    if family == "gemma3":
        assert S < int(enc.model.config.sliding_window)
    g = torch.Generator(device="cpu").manual_seed(41000 + S)
    ids = torch.randint(0, int(enc.model.config.vocab_size), (B, S), generator=g).cuda()
    lens = torch.randint(max(1, S // 2), S, (B,), generator=g) if padded else torch.full((B,), S)
    lens[0] = S
    am = (torch.arange(S)[None, :] < lens[:, None]).to(torch.int64).cuda()
    assert bool(am.all()) == (not padded)
    assert ff.bf16_attention_kind(torch.empty(0, dtype=BF16), S, hd, causal, padded) == "tiled"
    called = []
    real_op = _ffi.encoder_op
    monkeypatch.setattr(_ffi, "encoder_op", lambda op, *a: (called.append(op), real_op(op, *a))[1])

    def no_sdpa(*a, **kw):
        raise AssertionError("torch's scaled_dot_product_attention was called")

    with torch.inference_mode():
        with monkeypatch.context() as m:
            m.setenv("TS_ENCODER_ATTENTION", "0")
            torch_way = enc.forward_hidden(ids, am, no_padding=not padded).float()
            assert "ts_attention_flash" not in called
        del called[:]
        with monkeypatch.context() as m:
            m.setattr(torch.nn.functional, "scaled_dot_product_attention", no_sdpa)
            got = enc.forward_hidden(ids, am, no_padding=not padded).float()
    assert called.count("ts_attention_flash") == len(layers), called
    assert "ts_attention_short" not in called and "ts_attention_gqa" not in called, called
    real = am.bool()
    assert torch.isfinite(got[real]).all()
    scale = torch_way[real].abs().max().item()
    hmax, hmean = (torch_way - got)[real].abs().max().item() / scale, (torch_way - got)[real].abs().mean().item() / scale
    with capsys.disabled():
        print(f"\n{family} stand-in, bf16, {S} tokens, {'right padding' if padded else 'no padding'}: ts_attention_flash against torch's attention "
              f"max {hmax:.4f}, mean {hmean:.5f} of the largest hidden value (bounds {TOL['hmax']}, {TOL['hmean']})", end="")
    assert hmax <= TOL["hmax"] and hmean <= TOL["hmean"], (family, S, padded, hmax, hmean)
