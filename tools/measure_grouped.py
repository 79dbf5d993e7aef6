"""Timing of the grouped search (ts_search_grouped) against the plain search it is built on.

Corpus: --rows (10M) x 768 bf16 synthetic rows (synthetic.py), inner product; queries resident on the device; k = 10.
Cases: 256 queries, and one query (the UI's call).  Group designs: code = row // 8, and every row its own group (all NULL).
Per case and design, the median (min .. max) over --reps timed calls after --warmup calls of
  - the grouped search (device queries, device outputs; the call waits for its result, so the host clock around it is the
    time a caller sees);
  - the plain search at the same k, and at depth `first` (ts_group_depth) - the same host clock around search_device +
    synchronize.  With --parent-tree DIR these two come from the package and library of that checkout (the parent commit's,
    built), measured in a child process of this tool before this process opens the device; else from this build, and the
    file says so;
  - the collapse launch alone on the [nq x first] lists of the plain search, between two device events.
And the share of queries that stage 1 certified, that entered stage 2 and stage 3 (ts_grouped_stats).

  python tools/measure_grouped.py [--rows 10000000] [--parent-tree /path/to/a/built/checkout/of/the/parent] [--out profiles/grouped_<date>.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

D, K = 768, 10
CASES = (256, 1)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def timed(call, reps, warmup):
    """host clock around `call` (which waits for its result)"""
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def build_index(ts, n):
    from concurrent.futures import ThreadPoolExecutor

    import synthetic
    ix = ts.TheoremIndex(n, D, dtype="bf16", metric="ip")
    ch = synthetic.CHUNK_ROWS

    def make(c):
        a, b = c * ch, min(n, (c + 1) * ch)
        ix.upload(synthetic.synth_chunk(c, ch, D, bf16=True)[: b - a], a)

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(make, range((n + ch - 1) // ch)))
    return ix


def measure_plain(ts, ix, qd, args, first, label):
    import torch
    lines = []
    for nq in CASES:
        for depth, what in ((K, "plain search at k"), (first, "plain search at depth first")):
            out_s = torch.empty((nq, depth), dtype=torch.float32, device="cuda")
            out_i = torch.empty((nq, depth), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()

            def call():
                ix.search_device(qd.data_ptr(), "bf16", nq, depth, out_s.data_ptr(), out_i.data_ptr(), 0)
                ix.synchronize()

            line = {"what": what, "library": label, "rows": args.rows, "queries": nq, "k": K, "depth": depth, **timed(call, args.reps, args.warmup),
                    "reps": args.reps, "warmup": args.warmup}
            lines.append(line)
            print(json.dumps(line), flush=True)
    return lines


def measure_grouped(ts, ix, qd, args, first):
    import torch
    from theoremsearch_amd import _ffi
    from theoremsearch_amd.metadata import NULL
    n = args.rows
    lines = []
    designs = {"code = row // 8": (np.arange(n) // 8).astype(np.int32), "every row its own group": np.full(n, NULL, dtype=np.int32)}
    timer = ts.Timer(0)
    for design, column in designs.items():
        with ts.MetaTable.from_columns([column]) as table:
            col_dev = torch.from_numpy(column).cuda()
            for nq in CASES:
                out_s = torch.empty((nq, K), dtype=torch.float32, device="cuda")
                out_i = torch.empty((nq, K), dtype=torch.int64, device="cuda")
                out_g = torch.empty((nq, K), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                stats = {}

                def call():
                    stats.update(ix.search_grouped_device(qd.data_ptr(), "bf16", nq, K, table, 0, out_s.data_ptr(), out_i.data_ptr(), out_g.data_ptr()))

                line = {"what": "grouped search", "design": design, "rows": n, "queries": nq, "k": K, "first": first, **timed(call, args.reps, args.warmup),
                        "path_of_stage_1": {1: "scan", 2: "mfma"}.get(stats["algo"]),
                        "share_certified_in_stage_1": round(1 - stats["deep_queries"] / nq, 4),
                        "share_entered_stage_2": round(stats["deep_queries"] / nq, 4),
                        "share_entered_stage_3": round(stats["excluded_queries"] / nq, 4), "exclusion_passes": stats["exclusion_passes"],
                        "reps": args.reps, "warmup": args.warmup}
                lines.append(line)
                print(json.dumps(line), flush=True)
                # the collapse launch alone, on the lists of the plain search at depth first
                list_s = torch.empty((nq, first), dtype=torch.float32, device="cuda")
                list_i = torch.empty((nq, first), dtype=torch.int64, device="cuda")
                found = torch.empty((nq,), dtype=torch.int32, device="cuda")
                complete = torch.empty((nq,), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                ix.search_device(qd.data_ptr(), "bf16", nq, first, list_s.data_ptr(), list_i.data_ptr(), 0)
                ix.synchronize()
                st = ix.stream
                ms = []
                for rep in range(args.warmup + args.reps):
                    timer.start(st)
                    _ffi.check(_ffi.load().ts_collapse_topk(0, C.c_void_p(list_s.data_ptr()), C.c_void_p(list_i.data_ptr()), nq, first, K,
                                                            C.c_void_p(col_dev.data_ptr()), n, 0, C.c_void_p(out_s.data_ptr()),
                                                            C.c_void_p(out_i.data_ptr()), C.c_void_p(out_g.data_ptr()),
                                                            C.c_void_p(found.data_ptr()), C.c_void_p(complete.data_ptr()), 1, C.c_void_p(st)))
                    timer.stop(st)
                    ix.synchronize()
                    if rep >= args.warmup:
                        ms.append(timer.elapsed_ms())
                line = {"what": "collapse launch alone (device events)", "design": design, "queries": nq, "k_in": first, "k_out": K, **spread(ms),
                        "lists_complete": int(complete.sum().item()), "reps": args.reps}
                lines.append(line)
                print(json.dumps(line), flush=True)
            del col_dev
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: the two plain numbers come from it")
    ap.add_argument("--plain-only", action="store_true", help="(the child process of --parent-tree) time the plain searches, print the lines")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package and library are measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", f"grouped_{datetime.date.today().isoformat()}.json"))
    args = ap.parse_args()
    lines = []
    sys.path.insert(0, os.path.abspath(args.tree))
    if args.parent_tree and not args.plain_only:
        # a fresh child process on the other checkout, run to its end before this process opens the device
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--tree", os.path.abspath(args.parent_tree),
                                "--rows", str(args.rows), "--reps", str(args.reps), "--warmup", str(args.warmup)],
                               capture_output=True, text=True)
        if child.returncode != 0:
            raise SystemExit("the parent library's run failed:\n" + child.stdout + child.stderr)
        lines += [json.loads(x) for x in child.stdout.splitlines() if x.startswith("{")]
        for x in lines:
            print(json.dumps(x), flush=True)
    import torch

    import synthetic
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    if _ffi.device_count() == 0:
        raise SystemExit("measure_grouped.py needs a GPU: there is nothing to time without one")
    ix = build_index(ts, args.rows)
    qd = torch.from_numpy(synthetic.synth_queries(0, max(CASES), D, bf16=True).view(np.int16)).cuda()
    torch.cuda.synchronize()
    # the measured package may be older than the grouped search (the child of --parent-tree): the rule is restated for it
    first = min(256, max(2 * K, K + 16))
    if args.plain_only:
        measure_plain(ts, ix, qd, args, first, "parent commit")
        return
    assert ts.group_depth(K)[0] == first
    if not args.parent_tree:
        lines += measure_plain(ts, ix, qd, args, first, "this build (no --parent-tree given)")
    lines += measure_grouped(ts, ix, qd, args, first)
    ix.close()
    with open(args.out, "w") as f:
        f.write(json.dumps(lines, indent=1) + "\n")


if __name__ == "__main__":
    main()
