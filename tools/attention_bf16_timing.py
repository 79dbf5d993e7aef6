#!/usr/bin/env python3
"""ts_attention_flash (the bf16 attention at any length, fused_forward.attention_bf16) against what the fused bf16 forwards ran at
the same shape before it: torch's scaled_dot_product_attention on transposed views of the stacked projection with the context
copied back to [B x S x hq hd] (grouped-query through enable_gqa, repeat_interleave where torch refuses it) - once as the
forwards run a batch WITH padding (the additive mask they build once per forward, [B x 1 x 1 x S], for the causal family
[B x 1 x S x S]; the fill itself is timed beside it, it is paid once per forward and not counted against torch) and once as they
run a batch without (no mask, is_causal for the causal family).  ts_attention_flash takes the int64 key mask, or none.

bf16, 256 sequences (64 from 1,024 tokens on), hipEvents around 30 calls; every shape and side warmed up; the sides alternate
inside every round and the figure is the median of the rounds (--rounds, at least 5), one process, one device.  One JSON line per
row (also appended to --out).  `routed_max_seq` is the routing rule fused_forward._BF16_TILED_ROUTED_MAX_SEQ (with padding) and _BF16_TILED_ROUTED_MAX_SEQ_NO_PADDING follow."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS = 30
FAMILIES = {"bert": (12, 12, 64, False, 0.125), "qwen3": (16, 8, 128, True, 128 ** -0.5), "gemma3": (3, 1, 256, False, 0.0625)}
LENGTHS = {"bert": (192, 256, 384, 512), "qwen3": (129, 192, 256, 384, 512, 1024, 2048), "gemma3": (32, 64, 128, 192, 256, 384, 512)}
ROW_KEYS = ("pair", "family", "head_dim", "batch", "tokens", "heads", "causal", "max_abs_diff", "ts_us", "before_us", "ts_nomask_us",
            "before_nomask_us", "mask_fill_us", "spread_us", "rounds")


def batch_of(S: int) -> int:
    return 64 if S >= 1024 else 256


def at_least_as_fast(row: dict, padding: bool = True) -> bool:
    """The new entry was at least as fast as what the forward did before: for a batch with padding (torch gets the additive mask),
    or for one without (no mask)."""
    return row["ts_us"] <= row["before_us"] if padding else row["ts_nomask_us"] <= row["before_nomask_us"]


def routed_max_seq(rows, head_dim: int, padding: bool = True) -> int:
    """The longest measured length of the head size at which the new entry was at least as fast there and at every shorter
    measured length; 0 when it loses at the shortest (or nothing was measured): the head size is not routed."""
    best = 0
    for row in sorted((r for r in rows if r["head_dim"] == head_dim), key=lambda r: r["tokens"]):
        if not at_least_as_fast(row, padding):
            break
        best = row["tokens"]
    return best


def read_rows(path: str) -> list:
    with open(path) as f:
        rows = [json.loads(line) for line in f if line.strip()]
    for row in rows:
        missing = [k for k in ROW_KEYS if k not in row]
        assert not missing, (missing, row)
    return rows


def main():
    import torch
    from theoremsearch_amd.fused_forward import attention_bf16
    F = torch.nn.functional

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--families", default="bert,qwen3,gemma3", help="comma-separated subset of the rows' families")
    ap.add_argument("--note", default="", help="copied into every row (which build of the library this is)")
    args = ap.parse_args()
    assert args.rounds >= 5

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / CALLS * 1e3

    def alternate(sides, rounds):
        for fn in sides.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        seen = {name: [] for name in sides}
        for _ in range(rounds):
            for name, fn in sides.items():
                seen[name].append(window(fn))
        return {name: round(statistics.median(v), 1) for name, v in seen.items()}, {name: round(max(v) - min(v), 1) for name, v in seen.items()}

    def torch_attention(qkv, B, S, hq, hkv, hd, causal, scale, mask):
        nq, nkv = hq * hd, hkv * hd
        q = qkv[..., :nq].view(B, S, hq, hd).transpose(1, 2)
        k = qkv[..., nq:nq + nkv].view(B, S, hkv, hd).transpose(1, 2)
        v = qkv[..., nq + nkv:].view(B, S, hkv, hd).transpose(1, 2)
        kw = dict(attn_mask=mask, is_causal=causal and mask is None, scale=scale)
        try:
            ctx = F.scaled_dot_product_attention(q, k, v, enable_gqa=hq != hkv, **kw)
        except (RuntimeError, TypeError):
            rep = hq // hkv
            ctx = F.scaled_dot_product_attention(q, k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1), **kw)
        return ctx.transpose(1, 2).reshape(B, S, nq)

    def fill_mask(am, B, S, causal):
        neg = torch.finfo(torch.bfloat16).min
        if not causal:
            return torch.zeros((B, 1, 1, S), dtype=torch.bfloat16, device="cuda").masked_fill_(~am[:, None, None, :].to(torch.bool), neg)
        keep = torch.ones((S, S), dtype=torch.bool, device="cuda").tril_()[None, None] & am[:, None, None, :].to(torch.bool)
        return torch.zeros((B, 1, S, S), dtype=torch.bfloat16, device="cuda").masked_fill_(~keep, neg)

    for name in args.families.split(","):
        hq, hkv, hd, causal, scale = FAMILIES[name]
        for S in LENGTHS[name]:
            B = batch_of(S)
            g = torch.Generator(device="cpu").manual_seed(1000 * hd + S)
            qkv = torch.randn(B, S, (hq + 2 * hkv) * hd, generator=g).to(torch.bfloat16).cuda()
            # right padding as a batch of texts has it: lengths between half the batch's length and all of it, the first one full
            lens = torch.randint(max(1, S // 2), S + 1, (B,), generator=g)
            lens[0] = S
            am = (torch.arange(S)[None, :] < lens[:, None]).to(torch.int64).cuda().contiguous()
            mask = fill_mask(am, B, S, causal)
            want = torch_attention(qkv, B, S, hq, hkv, hd, causal, scale, mask)
            got = attention_bf16(qkv, am, B, S, hq, hkv, hd, causal, scale)
            diff = float((got.float() - want.float()).abs().max())
            del want, got
            us, spread = alternate({
                "before_us": lambda: torch_attention(qkv, B, S, hq, hkv, hd, causal, scale, mask),
                "ts_us": lambda: attention_bf16(qkv, am, B, S, hq, hkv, hd, causal, scale),
                "before_nomask_us": lambda: torch_attention(qkv, B, S, hq, hkv, hd, causal, scale, None),
                "ts_nomask_us": lambda: attention_bf16(qkv, None, B, S, hq, hkv, hd, causal, scale),
                "mask_fill_us": lambda: fill_mask(am, B, S, causal)}, args.rounds)
            row = {"pair": "flash vs torch", "family": name, "head_dim": hd, "batch": B, "tokens": S, "heads": f"{hq}/{hkv} x {hd}", "causal": causal,
                   "max_abs_diff": diff, **us, "spread_us": spread, "rounds": args.rounds,
                   "gflop": round(4.0 * B * hq * S * S * hd / 1e9 * (0.5 if causal else 1.0), 2)}
            row["at_least_as_fast"] = {"padding": at_least_as_fast(row, True), "no_padding": at_least_as_fast(row, False)}
            if args.note:
                row["note"] = args.note
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del qkv, mask, am
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
