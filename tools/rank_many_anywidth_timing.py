"""Timing of ts_rank_many at widths between and beyond the four hand-laid ones (synthetic corpus of --rows rows, 256 queries).

Per shape (storage type, d) two legs, each the median of --reps synchronous calls after one warm-up call:
  one   one target per query (rank ~10)
  many  16 targets per query (ranks ~10 .. 235)
Each leg reports the wall time of the call and the bracketed kernel time of its dominant launches (profile_read: the counting
launches of the matrix pass, or the streaming passes of the ts_rank_of fallback, one per target column and 256 queries), with
the number of those launches.  Run it on two builds (--label) to compare the matrix pass with the fallback it replaces.

  python tools/rank_many_anywidth_timing.py [--rows 1000000] [--shapes bf16:192,bf16:1536,bf16:2048,f32:640] [--reps 5]
                                            [--label NAME] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import synthetic  # noqa: E402
import theoremsearch_amd as ts  # noqa: E402


def timed(ix, fn, reps):
    fn()
    ix.profile_enable(True)
    ix.profile_read()
    wall, kern, launches = [], [], 0
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        p = ix.profile_read()
        kern.append(p["total_ms"])
        launches = p["launches"]
    ix.profile_enable(False)
    return {"wall_ms": round(statistics.median(wall), 3), "kernel_ms": round(statistics.median(kern), 3), "launches": launches,
            "all_wall_ms": [round(x, 3) for x in wall]}


def shape_legs(dtype, d, n, nq, reps, threads):
    bf16 = dtype == "bf16"
    CH = synthetic.CHUNK_ROWS
    ix = ts.TheoremIndex(n, d, dtype=dtype, metric="ip")
    t0 = time.time()

    def make(c):
        a, b = c * CH, min(n, (c + 1) * CH)
        ix.upload(synthetic.synth_chunk(c, CH, d, bf16=bf16)[: b - a], a)

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(make, range((n + CH - 1) // CH)))
    print(f"corpus {n} x {d} {dtype} ready in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    q = synthetic.synth_queries(0, nq, d, bf16=bf16)
    top = ix.search(q, 256)[1]
    one = [[int(top[i, 10])] for i in range(nq)]
    many = [[int(top[i, 10 + 15 * j]) for j in range(16)] for i in range(nq)]
    legs = {"one": timed(ix, lambda: ix.rank_many(q, one), reps), "many": timed(ix, lambda: ix.rank_many(q, many), reps)}
    ranks = ix.rank_many(q, many)[0]
    hits = sum(int(ranks[i][j] == 10 + 15 * j) for i in range(nq) for j in range(16))
    ix.close()
    res = {"dtype": dtype, "d": d, "rows": n, "nq": nq, "corpus_gb": round(n * d * (2 if bf16 else 4) / 1e9, 3), "legs": legs,
           "ranks_equal_to_search_positions": hits, "of": 16 * nq}
    print(res, file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--shapes", default="bf16:192,bf16:1536,bf16:2048,f32:640")
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    shapes = [(s.split(":")[0], int(s.split(":")[1])) for s in args.shapes.split(",")]
    res = {"label": args.label, "shapes": [shape_legs(dt, d, args.rows, args.nq, args.reps, args.threads) for dt, d in shapes]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
