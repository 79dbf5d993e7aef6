"""Timing of ts_rank_many against ts_rank_of on configs[2]'s shape (10M x 768 bf16 synthetic corpus, 256 queries).

Legs, each the median wall time of --reps calls after one warm-up call (the calls are synchronous):
  topk          ts_search k = 10 (the matrix pass with the top-k epilogue: the yardstick of the counting pass)
  rank_of       ts_rank_of, one target per query (rank ~10)
  many_shallow  rank_many, one target per query at rank ~10
  many_deep     rank_many, one target per query at rank ~N/2 (every score passes the fast reject)
  many_16       rank_many, 16 targets per query at ranks ~10 .. 250
Each leg is reported in ms and as the fraction of 8 TB/s for the corpus bytes (15.36 GB at the default shape).

  python tools/rank_many_timing.py [--rows 10000000] [--dim 768] [--nq 256] [--reps 5] [--out FILE]
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


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n, d, nq = args.rows, args.dim, args.nq
    CH = synthetic.CHUNK_ROWS
    ix = ts.TheoremIndex(n, d, dtype="bf16", metric="ip")
    t0 = time.time()

    def make(c):
        a, b = c * CH, min(n, (c + 1) * CH)
        ix.upload(synthetic.synth_chunk(c, CH, d, bf16=True)[: b - a], a)

    with ThreadPoolExecutor(args.threads) as ex:
        list(ex.map(make, range((n + CH - 1) // CH)))
    print(f"corpus {n} x {d} bf16 ready in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    q = synthetic.synth_queries(0, nq, d, bf16=True)

    # targets: ranks ~10 from the top-k pass; ~N/2 from the candidates (64 random rows per query) nearest the middle
    top = ix.search(q, 256)[1]
    shallow = [[int(top[i, 10])] for i in range(nq)]
    many16 = [[int(top[i, 10 + 15 * j]) for j in range(16)] for i in range(nq)]
    rng = np.random.default_rng(3)
    cand = rng.integers(0, n, (nq, 64))
    cr = ix.rank_many(q, [list(map(int, r)) for r in cand])[0]
    deep = [[int(cand[i, np.argmin(np.abs(cr[i] - n // 2))])] for i in range(nq)]
    deep_rank = [int(cr[i][np.argmin(np.abs(cr[i] - n // 2))]) for i in range(nq)]

    bytes_corpus = n * d * 2
    legs = {}

    def leg(name, fn):
        med, all_ = timed(fn, args.reps)
        legs[name] = {"ms": round(med, 3), "frac_8TBs": round(bytes_corpus / (med * 1e-3) / 8e12, 4),
                      "all_ms": [round(x, 3) for x in all_]}
        print(name, legs[name], file=sys.stderr, flush=True)

    leg("topk", lambda: ix.search(q, 10))
    leg("rank_of", lambda: ix.rank_of(q, [t[0] for t in shallow]))
    leg("many_shallow", lambda: ix.rank_many(q, shallow))
    leg("many_deep", lambda: ix.rank_many(q, deep))
    leg("many_16", lambda: ix.rank_many(q, many16))

    # the two paths agree on the shallow targets (the same canonical order; scores from different arithmetic)
    r_of = ix.rank_of(q, [t[0] for t in shallow])[0]
    r_many = np.array([r[0] for r in ix.rank_many(q, shallow)[0]])
    res = {"rows": n, "dim": d, "nq": nq, "dtype": "bf16", "corpus_gb": round(bytes_corpus / 1e9, 3), "legs": legs,
           "ratios": {"rank_of_over_many_shallow": round(legs["rank_of"]["ms"] / legs["many_shallow"]["ms"], 2),
                      "many_shallow_over_topk": round(legs["many_shallow"]["ms"] / legs["topk"]["ms"], 2),
                      "many_deep_over_shallow": round(legs["many_deep"]["ms"] / legs["many_shallow"]["ms"], 2),
                      "many_16_over_shallow": round(legs["many_16"]["ms"] / legs["many_shallow"]["ms"], 2)},
           "deep_rank_median": int(np.median(deep_rank)),
           "shallow_rank_of_vs_many_max_diff": int(np.max(np.abs(r_of - r_many)))}
    ix.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
