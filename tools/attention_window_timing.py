#!/usr/bin/env python3
"""The sliding-window attention entries (ts_attention_flash_window in bf16, ts_attention_tiled_window in fp32:
fused_forward.attention_bf16 / attention_tiled with window=) at Gemma3's shape - heads of 256, 3 query heads over 1 key / value head,
window 257 - against
  * the unwindowed parent entry at the same shape (the sanity gate: a windowed entry that is not clearly faster from 1,024 tokens on
    is not skipping chunks), and
  * what FusedGemma3Forward runs otherwise: torch's scaled_dot_product_attention with the additive mask of padding and window
    ([B x 1 x S x S]; without padding [1 x 1 x S x S]) on transposed views of the stacked projection, the context copied back to
    [B x S x hq hd].  The mask's fill is timed beside it: it is paid once per forward and not counted against torch.
258, 384, 512, 1,024 and 2,048 tokens, 256 sequences (64 from 1,024 tokens on), with right padding and without, bf16 and fp32.
hipEvents around CALLS calls; every shape and side warmed up; the sides alternate inside every round and the figure is the median of
the rounds (--rounds, at least 5), `spread_us` the largest minus the smallest round of each side; one process, one device.  One
JSON line per row (also appended to --out).  `routed_max_seq` is the rule fused_forward._WINDOW_ROUTED_MAX_SEQ_BF16 / _F32 follow."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HQ, HKV, HD, WINDOW, SCALE = 3, 1, 256, 257, 0.0625
LENGTHS = (258, 384, 512, 1024, 2048)
DTYPES = ("bf16", "fp32")
CHUNK = 32                                                  # keys per chunk at heads of 256 (attn_tiled_chunk)
ROW_KEYS = ("pair", "dtype", "head_dim", "batch", "tokens", "window", "heads", "max_abs_diff", "window_us", "parent_us", "torch_us",
            "window_nomask_us", "parent_nomask_us", "torch_nomask_us", "mask_fill_us", "spread_us", "rounds", "calls", "chunks_walked",
            "chunks_total")


def batch_of(S: int) -> int:
    return 64 if S >= 1024 else 256


def calls_of(S: int) -> int:
    return 10 if S >= 1024 else 30


def chunks_walked(S: int, W: int = WINDOW, C: int = CHUNK) -> tuple:
    """(chunks the workgroups of one (sequence, head) walk, chunks the parent's walk): the expected share of the parent's time."""
    walked = total = 0
    for q_first in range(0, S, 64):
        q_last = min(q_first + 63, S - 1)
        walked += min(S - 1, q_last + W - 1) // C - max(0, q_first - (W - 1)) // C + 1
        total += -(-S // C)
    return walked, total


def at_least_as_fast(row: dict) -> bool:
    """The windowed entry was at least as fast as torch's attention with the window mask and its layout copies, with padding and
    without (torch gets an additive mask either way and runs the same kernel: one table)."""
    return row["window_us"] <= row["torch_us"] and row["window_nomask_us"] <= row["torch_nomask_us"]


def routed_max_seq(rows, dtype: str, head_dim: int = HD) -> int:
    """The longest measured length of the type and head size at which the windowed entry was at least as fast there and at every
    shorter measured length; 0 when it loses at the shortest (or nothing was measured): not routed."""
    best = 0
    for row in sorted((r for r in rows if r["dtype"] == dtype and r["head_dim"] == head_dim), key=lambda r: r["tokens"]):
        if not at_least_as_fast(row):
            break
        best = row["tokens"]
    return best


def faster_than_parent(row: dict) -> bool:
    """The sanity gate: faster than the unwindowed parent entry by more than the spread between the alternating rounds."""
    sp = row["spread_us"]
    return (row["parent_us"] - row["window_us"] > max(sp["parent_us"], sp["window_us"]) and
            row["parent_nomask_us"] - row["window_nomask_us"] > max(sp["parent_nomask_us"], sp["window_nomask_us"]))


def read_rows(path: str) -> list:
    with open(path) as f:
        rows = [json.loads(line) for line in f if line.strip()]
    for row in rows:
        missing = [k for k in ROW_KEYS if k not in row]
        assert not missing, (missing, row)
    return rows


def main():
    import torch
    from theoremsearch_amd.fused_forward import attention_bf16, attention_tiled
    F = torch.nn.functional

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--dtypes", default=",".join(DTYPES))
    ap.add_argument("--lengths", default=",".join(str(s) for s in LENGTHS))
    ap.add_argument("--note", default="", help="copied into every row (which build of the library this is)")
    args = ap.parse_args()
    assert args.rounds >= 5

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls * 1e3

    def alternate(sides, rounds, calls):
        for fn in sides.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        seen = {name: [] for name in sides}
        for _ in range(rounds):
            for name, fn in sides.items():
                seen[name].append(timed(fn, calls))
        return {name: round(statistics.median(v), 1) for name, v in seen.items()}, {name: round(max(v) - min(v), 1) for name, v in seen.items()}

    def torch_attention(qkv, B, S, mask):
        nq, nkv = HQ * HD, HKV * HD
        q = qkv[..., :nq].view(B, S, HQ, HD).transpose(1, 2)
        k = qkv[..., nq:nq + nkv].view(B, S, HKV, HD).transpose(1, 2)
        v = qkv[..., nq + nkv:].view(B, S, HKV, HD).transpose(1, 2)
        try:
            ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=SCALE, enable_gqa=True)
        except (RuntimeError, TypeError):
            rep = HQ // HKV
            ctx = F.scaled_dot_product_attention(q, k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1), attn_mask=mask, scale=SCALE)
        return ctx.transpose(1, 2).reshape(B, S, nq)

    def fill_mask(am, S, dtype):
        """FusedGemma3Forward's additive mask of padding (am: [B x S] or None) and window."""
        pos = torch.arange(S, device="cuda")
        far = (pos[:, None] - pos[None, :]).abs() >= WINDOW
        hidden = far[None, None] if am is None else far[None, None] | ~am[:, None, None, :].to(torch.bool)
        return torch.zeros(hidden.shape, dtype=dtype, device="cuda").masked_fill_(hidden, torch.finfo(dtype).min)

    for dname in args.dtypes.split(","):
        dtype = torch.bfloat16 if dname == "bf16" else torch.float32
        if dname == "bf16":
            def ts(qkv, am, B, S, window):
                return attention_bf16(qkv, am, B, S, HQ, HKV, HD, False, SCALE, window=window)
        else:
            def ts(qkv, am, B, S, window):
                return attention_tiled(qkv, am, B, S, HQ, HKV, HD, False, SCALE, window=window)[0]
        for S in (int(s) for s in args.lengths.split(",")):
            B, calls = batch_of(S), calls_of(S)
            g = torch.Generator(device="cpu").manual_seed(1000 * HD + S)
            qkv = torch.randn(B, S, (HQ + 2 * HKV) * HD, generator=g).to(dtype).cuda()
            # right padding as a batch of texts has it: lengths between half the batch's length and all of it, the first one full
            lens = torch.randint(max(1, S // 2), S + 1, (B,), generator=g)
            lens[0] = S
            am = (torch.arange(S)[None, :] < lens[:, None]).to(torch.int64).cuda().contiguous()
            mask, mask_nopad = fill_mask(am, S, dtype), fill_mask(None, S, dtype)
            real = am.bool()
            diff = float((ts(qkv, am, B, S, WINDOW).float() - torch_attention(qkv, B, S, mask).float())[real].abs().max())
            us, spread = alternate({
                "torch_us": lambda: torch_attention(qkv, B, S, mask),
                "window_us": lambda: ts(qkv, am, B, S, WINDOW),
                "parent_us": lambda: ts(qkv, am, B, S, 0),
                "torch_nomask_us": lambda: torch_attention(qkv, B, S, mask_nopad),
                "window_nomask_us": lambda: ts(qkv, None, B, S, WINDOW),
                "parent_nomask_us": lambda: ts(qkv, None, B, S, 0),
                "mask_fill_us": lambda: fill_mask(am, S, dtype)}, args.rounds, calls)
            walked, total = chunks_walked(S)
            row = {"pair": "window vs parent vs torch", "dtype": dname, "head_dim": HD, "batch": B, "tokens": S, "window": WINDOW,
                   "heads": f"{HQ}/{HKV} x {HD}", "max_abs_diff": diff, **us, "spread_us": spread, "rounds": args.rounds, "calls": calls,
                   "chunks_walked": walked, "chunks_total": total}
            row["window_over_parent"] = {"padding": round(us["window_us"] / us["parent_us"], 3),
                                         "no_padding": round(us["window_nomask_us"] / us["parent_nomask_us"], 3), "chunks": round(walked / total, 3)}
            row["at_least_as_fast"] = at_least_as_fast(row)
            row["faster_than_parent"] = faster_than_parent(row)
            if args.note:
                row["note"] = args.note
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del qkv, mask, mask_nopad, am
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
