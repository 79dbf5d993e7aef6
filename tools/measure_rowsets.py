"""Timing of the search behind a row set per query (ts_search_rowsets) against the way without it: one ts_search_rowset call
per distinct set, each over the whole corpus.

Workload: --rows (10M) x 768 bf16, unit rows drawn on the device; 256 bf16 queries resident on the device, k = 10; S distinct row
sets of density 0.5 for S in --sets (1, 2, 8, 64, 256), the queries dealt to the sets in contiguous runs of 256 / S, plus one
mix: 230 queries on 8 dense sets and 26 on 2 sets of density 0.05.  The sets are programs over one column of random codes
(row IN a random half of 65,536 codes), evaluated on the device.

Per S, in one process, after --warmup rounds: --reps rounds of (A) then (B), device events around each on the index's stream.
  (A) one ts_search_rowsets call (TS_ALGO_AUTO);
  (B) one ts_search_rowset call per set with that set's queries (TS_ALGO_AUTO) - paths this library has had all along.
Recorded: median / min / max ms of both, A's routing counters (pass_queries, scan_calls, fallback_queries, candidates), and that both
gave the same ids.

  python tools/measure_rowsets.py [--rows 10000000] [--out profiles/rowsets_<date>.json]
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, NQ, K, CODES = 768, 256, 10, 65536


def build_index(ts, torch, n, chunk=500_000):
    ix = ts.TheoremIndex(n, D, dtype="bf16", metric="ip")
    g = torch.Generator(device="cuda").manual_seed(11)
    stream = torch.cuda.current_stream().cuda_stream
    for r0 in range(0, n, chunk):
        rows = min(chunk, n - r0)
        x = torch.randn((rows, D), generator=g, device="cuda", dtype=torch.float32)
        x /= x.norm(dim=1, keepdim=True)
        ix.upload_device(x.data_ptr(), "f32", D, r0, rows, stream)
        torch.cuda.synchronize()
    return ix


def make_sets(ts, table, count, density, seed):
    from theoremsearch_amd.metadata import IN, Atom, code_set
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        codes = np.flatnonzero(rng.random(CODES) < density)
        out.append(table.eval([Atom(IN, 0, set=code_set(codes, CODES), set_bits=CODES)]))
    return out


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def measure(ts, torch, ix, q, rowsets, which, reps, warmup):
    """which: sorted by set, so that a set's queries are contiguous rows of q."""
    nq = q.shape[0]
    timer = ts.Timer(0)
    stream = ix.stream
    out = [(torch.empty((nq, K), dtype=torch.float32, device="cuda"), torch.empty((nq, K), dtype=torch.int64, device="cuda")) for _ in range(2)]
    runs = []                                   # (set, first query, queries)
    for i, w in enumerate(which.tolist()):
        if runs and runs[-1][0] == w:
            runs[-1][2] += 1
        else:
            runs.append([w, i, 1])
    row_bytes = D * 2

    def a():
        return ix.search_rowsets_device(q.data_ptr(), "bf16", nq, K, rowsets, which, out[0][0].data_ptr(), out[0][1].data_ptr(), stream)

    def b():
        for w, first, count in runs:
            ix.search_device(q.data_ptr() + first * row_bytes, "bf16", count, K, out[1][0].data_ptr() + first * K * 4,
                             out[1][1].data_ptr() + first * K * 8, stream, rowset=rowsets[w])

    for _ in range(warmup):
        a()
        b()
    ix.synchronize()
    ms_a, ms_b, stats = [], [], None
    for _ in range(reps):
        timer.start(stream)
        stats = a()
        timer.stop(stream)
        ix.synchronize()
        ms_a.append(timer.elapsed_ms())
        timer.start(stream)
        b()
        timer.stop(stream)
        ix.synchronize()
        ms_b.append(timer.elapsed_ms())
    same = bool(torch.equal(out[0][1], out[1][1]))
    return {"rowsets_call": spread(ms_a), "call_per_set": dict(spread(ms_b), calls=len(runs)), "same_ids": same,
            "speedup_median": round(statistics.median(ms_b) / statistics.median(ms_a), 3), "stats": stats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--sets", type=int, nargs="*", default=[1, 2, 8, 64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", f"rowsets_{datetime.date.today().isoformat()}.json"))
    args = ap.parse_args()
    import torch
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    if _ffi.device_count() == 0:
        sys.exit("measure_rowsets.py needs a GPU")
    n = args.rows
    ix = build_index(ts, torch, n)
    g = torch.Generator(device="cuda").manual_seed(12)
    q = torch.randn((NQ, D), generator=g, device="cuda", dtype=torch.float32)
    q = (q / q.norm(dim=1, keepdim=True)).to(torch.bfloat16).contiguous()
    torch.cuda.synchronize()
    table = ts.MetaTable.from_columns([np.random.default_rng(13).integers(0, CODES, n).astype(np.int32)])
    dense = make_sets(ts, table, max(args.sets + [8]), 0.5, 14)
    sparse = make_sets(ts, table, 2, 0.05, 15)
    doc = {"workload": {"rows": n, "d": D, "dtype": "bf16", "queries": NQ, "k": K, "set_density": 0.5, "reps": args.reps, "warmup": args.warmup,
                        "timing": "device events on the index's stream around the whole call(s), A and B alternating per round"},
           "cases": []}
    for s in args.sets:
        which = (np.arange(NQ) * s // NQ).astype(np.int32)
        r = measure(ts, torch, ix, q, dense[:s], which, args.reps, args.warmup)
        doc["cases"].append(dict(r, case=f"{s} dense sets", distinct_sets=s))
        print(json.dumps(doc["cases"][-1]), flush=True)
    which = np.sort(np.concatenate([np.arange(230) % 8, 8 + np.arange(26) % 2])).astype(np.int32)
    r = measure(ts, torch, ix, q, dense[:8] + sparse, which, args.reps, args.warmup)
    doc["cases"].append(dict(r, case="230 queries on 8 dense sets, 26 on 2 sets of density 0.05", distinct_sets=10))
    print(json.dumps(doc["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
