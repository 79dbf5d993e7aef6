"""Timing of the citation-weighted search with a weight and a row set per query (ts_search_biased_rowsets) against the way
without it: one ts_search_biased_rowset call per class (set, weight), each over the whole corpus.

Workload: --rows (1M) x 768 bf16, unit rows drawn on the device; 256 bf16 queries resident on the device, k = 10; a bias array
of the citation recipe's shape (20 % zeros, ln of 1..399, a dozen rows at ln 1e6..1e8) on the device; row sets of density 0.5
(programs over one column of random codes, evaluated on the device).  C classes for C in --classes (2, 4, 16, 64, 256): class
c has set c % S and weight WEIGHTS[c // S] with S = 2, 2, 4, 16, 64 sets; the queries are dealt to the classes in contiguous
runs of 256 / C.

Per C, in one process, after --warmup rounds of both: --reps rounds of (A) then (B), device events around each on the index's
stream.
  (A) one ts_search_biased_rowsets call (TS_ALGO_AUTO);
  (B) one ts_search_biased_rowset call per class with that class's queries (TS_ALGO_AUTO) - what a caller had before.
Recorded: median / min / max ms of both, A's routing counters, and that both gave the same ids.

--hist-sets (1, 16, 256): calls whose 256 pass queries name that many sets (two weights, so that nothing is delegated), for
the histogram stage's own time: run the tool under a kernel trace (rocprofv3 --kernel-trace --output-format csv -d DIR -- python
tools/measure_biased_rowsets.py --classes --hist-sets 1 16 256) and read bias_range_kernel + bias_hist_sets_kernel per call.

  python tools/measure_biased_rowsets.py [--rows 1000000] [--out profiles/biased_rowsets_timing.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, NQ, K, CODES = 768, 256, 10, 65536
WEIGHTS = (0.02, 0.05, 0.0, -0.02)
SETS_OF = {2: 2, 4: 2, 16: 4, 64: 16, 256: 64}


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


def recipe_bias(n):
    rng = np.random.default_rng(9)
    u, v = rng.random(n), rng.integers(1, 400, n)
    cites = np.where(u < 0.2, 0, v).astype(np.float64)
    cites[rng.choice(n, 12, replace=False)] = 10.0 ** rng.integers(6, 9, 12)
    return np.where(cites > 0, np.log(np.maximum(cites, 1.0)), 0.0).astype(np.float32)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def measure(ts, torch, ix, q, bias, rowsets, which, weights, reps, warmup):
    """which / weights: a class's queries are contiguous rows of q."""
    from theoremsearch_amd import _ffi
    lib = _ffi.load()
    nq = q.shape[0]
    timer = ts.Timer(0)
    stream = ix.stream
    out = [(torch.empty((nq, K), dtype=torch.float32, device="cuda"), torch.empty((nq, K), dtype=torch.int64, device="cuda")) for _ in range(2)]
    runs = []                                   # (set, weight, first query, queries)
    for i, (s, w) in enumerate(zip(which.tolist(), weights.tolist())):
        if runs and runs[-1][0] == s and runs[-1][1] == w:
            runs[-1][3] += 1
        else:
            runs.append([s, w, i, 1])
    row_bytes = D * 2

    def a():
        return ix.search_biased_rowsets_device(q.data_ptr(), "bf16", nq, K, bias.data_ptr(), weights, rowsets, which, out[0][0].data_ptr(), 0,
                                               out[0][1].data_ptr(), stream)

    def b():
        for s, w, first, count in runs:
            _ffi.check(lib.ts_search_biased_rowset(ix.handle, C.c_void_p(q.data_ptr() + first * row_bytes), _ffi.TS_BF16, 1, count, K,
                                                   C.c_void_p(bias.data_ptr()), 1, float(w), rowsets[s].handle,
                                                   C.c_void_p(out[1][0].data_ptr() + first * K * 4), None,
                                                   C.c_void_p(out[1][1].data_ptr() + first * K * 8), 1, C.c_void_p(stream), _ffi.TS_ALGO_AUTO, None))

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
    return {"biased_rowsets_call": spread(ms_a), "call_per_class": dict(spread(ms_b), calls=len(runs)), "same_ids": same,
            "speedup_median": round(statistics.median(ms_b) / statistics.median(ms_a), 3), "stats": stats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--classes", type=int, nargs="*", default=[2, 4, 16, 64, 256])
    ap.add_argument("--hist-sets", type=int, nargs="*", default=[])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "biased_rowsets_timing.json"))
    args = ap.parse_args()
    import torch
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    if _ffi.device_count() == 0:
        sys.exit("measure_biased_rowsets.py needs a GPU")
    n = args.rows
    ix = build_index(ts, torch, n)
    g = torch.Generator(device="cuda").manual_seed(12)
    q = torch.randn((NQ, D), generator=g, device="cuda", dtype=torch.float32)
    q = (q / q.norm(dim=1, keepdim=True)).to(torch.bfloat16).contiguous()
    bias = torch.from_numpy(recipe_bias(n)).cuda()
    torch.cuda.synchronize()
    table = ts.MetaTable.from_columns([np.random.default_rng(13).integers(0, CODES, n).astype(np.int32)])
    dense = make_sets(ts, table, max([SETS_OF[c] for c in args.classes] + args.hist_sets + [1]), 0.5, 14)
    doc = {"workload": {"rows": n, "d": D, "dtype": "bf16", "queries": NQ, "k": K, "set_density": 0.5, "weights": list(WEIGHTS),
                        "reps": args.reps, "warmup": args.warmup,
                        "timing": "device events on the index's stream around the whole call(s), A and B alternating per round"},
           "cases": []}
    for c in args.classes:
        s = SETS_OF[c]
        cls = np.arange(NQ) * c // NQ
        which = (cls % s).astype(np.int32)
        weights = np.asarray(WEIGHTS, dtype=np.float32)[cls // s]
        r = measure(ts, torch, ix, q, bias, dense[:s], which, weights, args.reps, args.warmup)
        doc["cases"].append(dict(r, case=f"{c} classes", classes=c, distinct_sets=s))
        print(json.dumps(doc["cases"][-1]), flush=True)
    for s in args.hist_sets:
        which = (np.arange(NQ) % s).astype(np.int32)
        weights = np.asarray(WEIGHTS[:2], dtype=np.float32)[(np.arange(NQ) // s) % 2] if s < NQ else np.asarray(WEIGHTS[:2], dtype=np.float32)[np.arange(NQ) % 2]
        out_s = torch.empty((NQ, K), dtype=torch.float32, device="cuda")
        out_i = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
        for _ in range(args.warmup + args.reps):
            st = ix.search_biased_rowsets_device(q.data_ptr(), "bf16", NQ, K, bias.data_ptr(), weights, dense[:s], which, out_s.data_ptr(), 0,
                                                 out_i.data_ptr(), ix.stream)
        print(json.dumps({"case": f"histograms of {s} sets", "calls": args.warmup + args.reps, "stats": st}), flush=True)
    if args.classes:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
