#!/usr/bin/env python3
"""ts_attention_tiled past ts_attention_float's limits against what the fused fp32 forwards ran there before: torch's
scaled_dot_product_attention on views of the stacked projection with the context transposed back (grouped-query through
enable_gqa, repeat_interleave where torch refuses it - FusedQwen3Forward._sdpa / FusedGemma3Forward._sdpa), and, for the
fp32x3 forward, ts_split_pieces of that context against the kernel's own pieces.  For the record also against ts_attention_float
at each head size's old limit, where both serve.

fp32, hipEvents around 30 calls; every shape and side warmed up; the two sides of a pair alternate inside every round and the
figure is the median of the rounds (--rounds, at least 5); max_abs_diff of the two contexts stands beside every pair.  One JSON
line per row (also appended to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from theoremsearch_amd.fused_forward import attention_float, attention_tiled, split_pieces  # noqa: E402

F = torch.nn.functional
CALLS = 30


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3


def alternate(sides, rounds):
    """us per call of each side: every side warmed up, then `rounds` rounds of one window per side, in turn; the medians."""
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    seen = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            seen[name].append(window(fn))
    return {name: round(statistics.median(v), 1) for name, v in seen.items()}, {name: round(max(v) - min(v), 1) for name, v in seen.items()}


def torch_attention(qkv, B, S, hq, hkv, hd, causal, scale):
    nq, nkv = hq * hd, hkv * hd
    q = qkv[..., :nq].view(B, S, hq, hd).transpose(1, 2)
    k = qkv[..., nq:nq + nkv].view(B, S, hkv, hd).transpose(1, 2)
    v = qkv[..., nq + nkv:].view(B, S, hkv, hd).transpose(1, 2)
    try:
        ctx = F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=scale, enable_gqa=hq != hkv)
    except (RuntimeError, TypeError):
        rep = hq // hkv
        ctx = F.scaled_dot_product_attention(q, k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1), is_causal=causal, scale=scale)
    return ctx.transpose(1, 2).reshape(B, S, nq)


FAMILIES = {"bert": (12, 12, 64, False, 0.125), "qwen3": (16, 8, 128, True, 128 ** -0.5), "gemma3": (3, 1, 256, False, 0.0625)}
PAST_THE_LIMIT = (("qwen3", 384, 256), ("qwen3", 512, 256), ("qwen3", 1024, 64), ("gemma3", 192, 256), ("gemma3", 256, 256), ("gemma3", 384, 256))
AT_THE_LIMIT = (("bert", 512, 256), ("qwen3", 256, 256), ("gemma3", 128, 256))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--families", default="bert,qwen3,gemma3", help="comma-separated subset of the rows' families")
    ap.add_argument("--note", default="", help="copied into every row (which build of the library this is)")
    args = ap.parse_args()
    assert args.rounds >= 5
    families = args.families.split(",")

    def emit(row):
        if args.note:
            row["note"] = args.note
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for name, S, B in (r for r in PAST_THE_LIMIT if r[0] in families):
        hq, hkv, hd, causal, scale = FAMILIES[name]
        qkv = torch.randn(B, S, (hq + 2 * hkv) * hd, device="cuda")
        shape = (qkv, None, B, S, hq, hkv, hd, causal, scale)
        want = torch_attention(qkv, B, S, hq, hkv, hd, causal, scale)
        got = attention_tiled(*shape)[0]
        diff = float((got - want).abs().max())
        del want, got
        us, spread = alternate({
            "torch_us": lambda: torch_attention(qkv, B, S, hq, hkv, hd, causal, scale),
            "ts_attention_tiled_us": lambda: attention_tiled(*shape),
            "torch_split_pieces_us": lambda: split_pieces(torch_attention(qkv, B, S, hq, hkv, hd, causal, scale).view(B * S, -1), 0),
            "tiled_pieces_only_us": lambda: attention_tiled(*shape, want_pieces=True, want_context=False)}, args.rounds)
        emit({"pair": "tiled vs torch", "family": name, "batch": B, "tokens": S, "heads": f"{hq}/{hkv} x {hd}", "causal": causal, "max_abs_diff": diff,
              **us, "spread_us": spread, "rounds": args.rounds, "gflop": round(4.0 * B * hq * S * S * hd / 1e9 * (0.5 if causal else 1.0), 2)})
        del qkv
        torch.cuda.empty_cache()
    for name, S, B in (r for r in AT_THE_LIMIT if r[0] in families):
        hq, hkv, hd, causal, scale = FAMILIES[name]
        qkv = torch.randn(B, S, (hq + 2 * hkv) * hd, device="cuda")
        shape = (qkv, None, B, S, hq, hkv, hd, causal, scale)
        diff = float((attention_tiled(*shape)[0] - attention_float(*shape)[0]).abs().max())
        us, spread = alternate({"ts_attention_float_us": lambda: attention_float(*shape), "ts_attention_tiled_us": lambda: attention_tiled(*shape)}, args.rounds)
        emit({"pair": "tiled vs float", "family": name, "batch": B, "tokens": S, "heads": f"{hq}/{hkv} x {hd}", "causal": causal, "max_abs_diff": diff,
              **us, "spread_us": spread, "rounds": args.rounds, "gflop": round(4.0 * B * hq * S * S * hd / 1e9 * (0.5 if causal else 1.0), 2)})
        del qkv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
