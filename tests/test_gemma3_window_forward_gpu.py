"""FusedGemma3Forward past the sliding window.  The Gemma3 stand-in (random weights; seven layers in bf16, so that sliding and full
attention layers both occur; two layers in fp32, also with the GEMMs from bf16 pieces) at B = 4, S = 300 > sliding_window = 257, right
padding with one full-length row: the fused forward completes WITHOUT the model's own forward (patched to raise) and agrees with it
on the real tokens within the tolerances of tests/test_mirrors_gpu.py::test_fused_gemma3_forward_matches_the_models_own - max < 0.06
and mean < 0.01 of the largest hidden value in bf16, 5e-4 in fp32 (1e-3 with the GEMMs from pieces, the full-depth test's) -
* as fused_forward routes it (_WINDOW_ROUTED_MAX_SEQ_BF16 / _F32: the windowed entry once per sliding layer with
  window == cfg.sliding_window where the table reaches 300 tokens, torch's attention with the additive window mask otherwise),
* with the tables set to route 300 tokens (the windowed entries inside the forward, whatever the measurement routes),
* under TS_ENCODER_ATTENTION=0 (the torch form, no library attention).
At S = 200 the window hides nothing and the calls are today's: no windowed entry, the parents' entries where they were."""
import functools

import pytest
import torch

from theoremsearch_amd import _ffi
from theoremsearch_amd import fused_forward as ff

pytestmark = pytest.mark.gpu

NAME = "google/embeddinggemma-300m"
B, S = 4, 300
WINDOW_OPS = {"bf16": "ts_attention_flash_window", "fp32": "ts_attention_tiled_window", "fp32x3": "ts_attention_tiled_window"}
TABLE = {"bf16": "_WINDOW_ROUTED_MAX_SEQ_BF16", "fp32": "_WINDOW_ROUTED_MAX_SEQ_F32", "fp32x3": "_WINDOW_ROUTED_MAX_SEQ_F32"}
ATTENTION_OPS = ("ts_attention_flash", "ts_attention_tiled", "ts_attention_float", "ts_attention_flash_window", "ts_attention_tiled_window")


@functools.lru_cache(maxsize=None)
def encoder(mode):
    from theoremsearch_amd.encoder import SentenceEncoder
    if mode == "bf16":
        enc = SentenceEncoder(NAME, num_layers=7, allow_random_init=True, dtype=torch.bfloat16)
    else:
        enc = SentenceEncoder(NAME, num_layers=2, allow_random_init=True, dtype=torch.float32, fp32_gemm="bf16x3" if mode == "fp32x3" else "blas")
    assert isinstance(enc._fused, ff.FusedGemma3Forward) and enc._fused.pieces == (mode == "fp32x3")
    return enc


def batch(enc, length):
    g = torch.Generator(device="cpu").manual_seed(52000 + length)
    ids = torch.randint(0, int(enc.model.config.vocab_size), (B, length), generator=g).cuda()
    lens = torch.randint(length // 2, length, (B,), generator=g)
    lens[0] = length
    am = (torch.arange(length)[None, :] < lens[:, None]).to(torch.int64).cuda()
    return ids, am


def fused_without_the_models_forward(enc, ids, am, monkeypatch):
    """(hidden states, the encoder ops called with their arguments) of the fused forward while the model's own forward raises."""
    called = []
    real_op = _ffi.encoder_op

    def refuse(*a, **kw):
        raise AssertionError("the model's own forward was called")

    with monkeypatch.context() as m:
        m.setattr(_ffi, "encoder_op", lambda op, *a: (called.append((op, a)), real_op(op, *a))[1])
        m.setattr(enc.model, "forward", refuse)
        with torch.inference_mode():
            got = enc.forward_hidden(ids, am).float()
    return got, called


def check_close(mode, got, want, am, capsys, what):
    real = am.bool()
    assert torch.isfinite(got[real]).all()
    err = (want - got)[real].abs()
    scale = want[real].abs().max().item()
    with capsys.disabled():
        print(f"\n  gemma3 stand-in {mode}, {got.shape[1]} tokens, {what}: max {err.max().item() / scale:.5f}, mean {err.mean().item() / scale:.6f} "
              f"of the largest hidden value", end="")
    if mode == "bf16":
        assert err.max().item() < 0.06 * scale and err.mean().item() < 0.01 * scale, (mode, what)
    else:
        # fp32: test_fused_gemma3_forward_matches_the_models_own's 5e-4; GEMMs from bf16 pieces: the full-depth test's 1e-3
        # (tests/test_attention_tiled_gpu.py FORWARD_TOL), of the largest hidden value
        assert err.max().item() < (1e-3 if mode == "fp32x3" else 5e-4) * max(1.0, scale), (mode, what)


@pytest.mark.parametrize("mode", ("bf16", "fp32", "fp32x3"))
def test_the_fused_forward_serves_300_tokens_without_the_models_own(mode, monkeypatch, capsys):
    enc = encoder(mode)
    cfg = enc.model.config
    W = int(cfg.sliding_window)
    assert W == 257 < S
    sliding = sum(1 for L in enc._fused.layers if L["type"] == "sliding_attention")
    assert sliding >= 2 and (mode != "bf16" or sliding < len(enc._fused.layers))
    ids, am = batch(enc, S)
    with torch.inference_mode():
        want = enc.model(input_ids=ids, attention_mask=am).last_hidden_state.float()
    monkeypatch.delenv("TS_ENCODER_ATTENTION", raising=False)
    op, where = WINDOW_OPS[mode], (9 if mode == "bf16" else 10)          # the window's place among encoder_op's arguments
    # as the measurement routes it
    routed = S <= getattr(ff, TABLE[mode]).get(256, 0)
    got, called = fused_without_the_models_forward(enc, ids, am, monkeypatch)
    windows = [a[where] for name, a in called if name == op]
    assert windows == ([W] * sliding if routed else []), (mode, routed, windows)
    check_close(mode, got, want, am, capsys, "as routed: " + ("the windowed entry" if routed else "torch's attention with the window mask"))
    # the windowed entries inside the forward, whatever the measurement routes
    with monkeypatch.context() as m:
        m.setattr(ff, TABLE[mode], {256: 2048})
        got, called = fused_without_the_models_forward(enc, ids, am, monkeypatch)
    windows = [a[where] for name, a in called if name == op]
    assert windows == [W] * sliding, (mode, windows)
    assert not any(name in WINDOW_OPS.values() and name != op for name, _ in called)
    check_close(mode, got, want, am, capsys, "the windowed entry")
    # the torch form everywhere
    with monkeypatch.context() as m:
        m.setenv("TS_ENCODER_ATTENTION", "0")
        m.setattr(ff, TABLE[mode], {256: 2048})
        got, called = fused_without_the_models_forward(enc, ids, am, monkeypatch)
    assert not any(name in ATTENTION_OPS for name, _ in called), [name for name, _ in called if name in ATTENTION_OPS]
    check_close(mode, got, want, am, capsys, "TS_ENCODER_ATTENTION=0")


@pytest.mark.parametrize("mode", ("bf16", "fp32"))
def test_at_200_tokens_the_calls_are_todays(mode, monkeypatch, capsys):
    enc = encoder(mode)
    ids, am = batch(enc, 200)
    monkeypatch.delenv("TS_ENCODER_ATTENTION", raising=False)
    with torch.inference_mode():
        want = enc.model(input_ids=ids, attention_mask=am).last_hidden_state.float()
    with monkeypatch.context() as m:
        m.setattr(ff, TABLE[mode], {256: 2048})                          # even a table that routes every length: the window hides nothing
        got, called = fused_without_the_models_forward(enc, ids, am, monkeypatch)
    attention = [name for name, _ in called if name in ATTENTION_OPS]
    parent = "ts_attention_flash" if mode == "bf16" else "ts_attention_tiled"
    assert attention == [parent] * len(enc._fused.layers), attention
    check_close(mode, got, want, am, capsys, "no key hidden")
