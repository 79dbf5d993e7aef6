"""Timing of the metadata filter on the device (ts_meta_eval, kernels_meta.h) and of the search behind its row set.

1. The evaluator: --rows (10M) rows of columns shaped like tests/filters_common.make_sql_rows - the same value sets and NULL
   shares, generated straight into numpy columns - and the `open`, `years` and `everything` states of sql_filter_states().  Per
   state: the median over --reps calls, after --warmup calls, of the whole ts_meta_eval call between two device events on the
   stream it runs on (its set upload, the counter's memset, the kernel, the count's read-back), the host time of the call, the
   bytes the columns the program names hold, the mask it writes, and (bytes read + written) / time as a fraction of the HBM
   peak (8.0 TB/s, the specification's).
2. The host path it replaces: filters.sql_filter_mask for the same states over make_sql_rows(--host-rows) (200,000), timed once
   each with the host clock.  Reported as measured at that n, not extrapolated.
3. The search: --search-rows x 768 bf16, 256 queries resident on the device, k = 10, behind a mask that allows a fifth of the
   rows (citations in [0, 49]): through the row set (ts_search_rowset, AUTO: the matrix path) and with the same mask handed over
   as a bare device pointer (ts_search_filtered: the scan).  Median over --reps calls after one warm-up, device events on the
   index's stream.

  python tools/measure_filters.py [--rows 10000000] [--search-rows 1000000] [--out profiles/measure_filters.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12
CATS = ["math.AG", "math.NT", "math.PR"]
NAMES = ["Theorem", "Lemma", "Main Theorem", "Corollary", "proposition"]


def sql_columns(n, seed=9):
    """make_sql_rows's distributions as columns: (columns in the order of MetaTable.from_sql_rows, dictionaries)."""
    from filters_common import AUTHORS
    from theoremsearch_amd.metadata import NULL
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    kind = rng.integers(0, 10, n)
    source = np.where(kind == 0, NULL, np.where(kind < 7, 0, 1)).astype(np.int32)
    paper = i.astype(np.int32)                                   # a paper per row: the paper box is not timed here
    journal = (rng.random(n) >= 0.6).astype(np.int32)
    cat = rng.integers(0, 4, n).astype(np.int32)
    cat[cat == 3] = NULL
    name = rng.integers(0, 6, n).astype(np.int32)
    name[name == 5] = NULL
    year = np.where(i % 13 == 0, NULL, rng.integers(1995, 2026, n)).astype(np.int32)
    cit = np.where(i % 5 == 0, NULL, rng.integers(0, 200, n)).astype(np.int32)
    lens = np.where(i % 11 == 0, 0, rng.integers(1, 3, n))
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    first = rng.integers(0, 5, n)
    second = (first + rng.integers(1, 5, n)) % 5                 # two distinct authors
    codes = np.empty(int(offsets[-1]), dtype=np.int32)
    codes[offsets[:-1][lens >= 1]] = first[lens >= 1]
    codes[offsets[:-1][lens == 2] + 1] = second[lens == 2]
    cols = [source, paper, journal, cat, name, year, cit, (offsets, codes)]
    return cols, {"primary_category": CATS, "type_name": NAMES, "authors": AUTHORS}


def program_bytes(table, atoms):
    """bytes the columns a program names hold (each column once), and the mask the evaluation writes"""
    held = 0
    for c in sorted({a.col for a in atoms}):
        col = table.columns[c]
        held += col[0].nbytes + col[1].nbytes if isinstance(col, tuple) else col.nbytes
    return held, (table.n + 255) // 256 * 32


def median_ms(timer, stream, reps, warmup, call, sync):
    for _ in range(warmup):
        call()
    sync()
    ms, host = [], []
    for _ in range(reps):
        timer.start(stream)
        t0 = time.perf_counter()
        call()
        host.append((time.perf_counter() - t0) * 1e3)
        timer.stop(stream)
        sync()
        ms.append(timer.elapsed_ms())
    return statistics.median(ms), min(ms), statistics.median(host)


def measure_eval(ts, args, out):
    from filters_common import sql_filter_states
    from theoremsearch_amd import _ffi
    from theoremsearch_amd.metadata import _SQL
    cols, dicts = sql_columns(args.rows)
    table = ts.MetaTable.from_columns(cols, names=_SQL, dictionaries=dicts)
    timer = ts.Timer(0)
    states = sql_filter_states()
    for state in ("open", "years", "everything"):
        atoms = table.compile(states[state])
        held, written = program_bytes(table, atoms)
        sets = []

        def call():
            sets.append(table.eval(atoms))

        def sync():
            _ffi.check(_ffi.load().ts_device_synchronize(0))
            while len(sets) > 1:
                sets.pop(0).close()

        ms, ms_min, host_ms = median_ms(timer, 0, args.reps, args.warmup, call, sync)
        rs = sets.pop()
        line = {"what": "ts_meta_eval", "state": state, "rows": args.rows, "atoms": len(atoms), "groups": len({a.group for a in atoms}),
                "allowed": rs.allowed, "fraction_allowed": round(rs.allowed / args.rows, 4), "event_ms": round(ms, 4),
                "event_ms_min": round(ms_min, 4), "host_call_ms": round(host_ms, 4), "column_bytes": held, "mask_bytes": written,
                "hbm_fraction_of_8TBps": round((held + written) / (ms * 1e-3) / HBM_PEAK, 4), "reps": args.reps, "warmup": args.warmup}
        rs.close()
        out.append(line)
        print(json.dumps(line), flush=True)
    table.close()


def measure_host(args, out):
    from filters_common import make_sql_rows, sql_filter_states
    from theoremsearch_amd.filters import sql_filter_mask
    rows = make_sql_rows(args.host_rows)
    states = sql_filter_states()
    for state in ("open", "years", "everything"):
        t0 = time.perf_counter()
        mask = sql_filter_mask(rows, states[state])
        line = {"what": "filters.sql_filter_mask (host, per-row predicate)", "state": state, "rows": args.host_rows,
                "measured_at_rows": args.host_rows, "host_s": round(time.perf_counter() - t0, 4), "fraction_allowed": round(float(mask.mean()), 4)}
        out.append(line)
        print(json.dumps(line), flush=True)


def measure_search(ts, args, out):
    import torch

    import synthetic
    from concurrent.futures import ThreadPoolExecutor
    from theoremsearch_amd.metadata import RANGE, Atom
    n, d, nq, k = args.search_rows, 768, 256, 10
    ix = ts.TheoremIndex(n, d, dtype="bf16", metric="ip")
    CH = synthetic.CHUNK_ROWS

    def make(c):
        a, b = c * CH, min(n, (c + 1) * CH)
        ix.upload(synthetic.synth_chunk(c, CH, d, bf16=True)[: b - a], a)

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(make, range((n + CH - 1) // CH)))
    cols, _ = sql_columns(n)
    table = ts.MetaTable.from_columns(cols)
    rs = table.eval([Atom(RANGE, 6, 0, 49)])                     # citations in [0, 49]: a fifth of the rows
    q = synthetic.synth_queries(0, nq, d, bf16=True)
    qd = torch.from_numpy(q.view(np.int16)).cuda()
    out_s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    out_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    timer = ts.Timer(0)
    st = ix.stream
    answers = {}
    for label, kw in (("row set (ts_search_rowset, auto)", {"rowset": rs}), ("bare device mask (ts_search_filtered)", {"mask_ptr": rs.mask_ptr})):
        call = lambda: ix.search_device(qd.data_ptr(), "bf16", nq, k, out_s.data_ptr(), out_i.data_ptr(), st, **kw)
        ms, ms_min, _ = median_ms(timer, st, args.reps, 1, call, ix.synchronize)
        answers[label] = out_i.cpu().numpy().copy()
        qh = synthetic.bf16_bits_to_f32(q)
        used = ix.search(qh, k, mask=rs, return_stats=True)[2]["algo"] if "rowset" in kw else 1
        line = {"what": "filtered search, 256 queries, k = 10, bf16 d = 768", "mask": label, "rows": n, "fraction_allowed": round(rs.allowed / n, 4),
                "algo": {1: "scan", 2: "mfma"}[used], "event_ms": round(ms, 4), "event_ms_min": round(ms_min, 4), "reps": args.reps}
        out.append(line)
        print(json.dumps(line), flush=True)
    a, b = answers.values()
    print(json.dumps({"what": "the two answers name the same rows", "equal": bool(np.array_equal(a, b))}), flush=True)
    rs.close()
    table.close()
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--host-rows", type=int, default=200_000)
    ap.add_argument("--search-rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated: eval, host, search")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_filters.json"))
    args = ap.parse_args()
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    if _ffi.device_count() == 0:
        raise SystemExit("measure_filters.py needs a GPU: there is nothing to time without one")
    skip = set(args.skip.split(","))
    out = []
    if "eval" not in skip:
        measure_eval(ts, args, out)
    if "host" not in skip:
        measure_host(args, out)
    if "search" not in skip:
        measure_search(ts, args, out)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
