"""The k-chunked search's full pass (mfma_wide_kernel) beside the k-chunked rank pass's shallow counting launch
(rank_wide_kernel) at the same shape and batch, in ONE process: 1M rows, 256 queries, the two calls alternating seven times after
a warm-up of each; the figures are the bracketed kernel times of ts_index_profile_read (the full pass of a k = 10 search under
algo = mfma; the counting launch of a rank_many call with the query's rank-10 row as its one target), medians and all seven.

  python tools/rank_wide_pass_ab.py [--rows 1000000] [--out profiles/rank_wide_pass_ab.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("bf16", 2560), ("bf16", 4096), ("f32", 1536)]
BLOCK = 50_000
NQ = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_wide_pass_ab.json"))
    args = ap.parse_args()
    import torch

    import synthetic
    import theoremsearch_amd as ts
    out = {"rows": args.rows, "nq": NQ, "reps": args.reps, "shapes": []}
    for dtype, d in SHAPES:
        n, bf16 = args.rows, dtype == "bf16"
        ix = ts.TheoremIndex(n, d, dtype=dtype, metric="ip")
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1234 + d)
        for r0 in range(0, n, BLOCK):
            nb = min(BLOCK, n - r0)
            x = torch.randn((nb, d), generator=gen, device="cuda", dtype=torch.float32)
            x /= x.norm(dim=1, keepdim=True)
            torch.cuda.synchronize()
            ix.upload_device(x.data_ptr(), "f32", d, r0, nb)
            ix.synchronize()
        del x
        q = synthetic.synth_queries(0, NQ, d, bf16=bf16)
        qh = synthetic.bf16_bits_to_f32(q) if bf16 else q
        top = ix.search(qh, 256, algo="mfma")[1]
        one = [[int(top[i, 10])] for i in range(NQ)]
        ix.search(qh, 10, algo="mfma")
        ix.rank_many(qh, one)
        s_ms, r_ms = [], []
        ix.profile_enable(True)
        ix.profile_read()
        for _ in range(args.reps):
            ix.search(qh, 10, algo="mfma")
            p = ix.profile_read()
            s_ms.append(p["total_ms"] / max(1, p["launches"]))
            ix.rank_many(qh, one)
            p = ix.profile_read()
            r_ms.append(p["total_ms"] / max(1, p["launches"]))
        ix.profile_enable(False)
        ix.close()
        entry = {"dtype": dtype, "dim": d, "search_full_pass_ms": round(statistics.median(s_ms), 4),
                 "rank_count_pass_ms": round(statistics.median(r_ms), 4), "search_all": [round(x, 3) for x in s_ms],
                 "rank_all": [round(x, 3) for x in r_ms]}
        out["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
