"""Timing of ts_rank_many at the row widths the k-chunked rank pass serves (kernels_rank_wide.h: rows of more than 4,096 and at
most 16,384 bytes, d % 256 == 0) against a library built from the parent commit, where these widths take one streaming
ts_rank_of pass per target column.

Shapes (seeded random-normal unit rows made on the device, inner-product indexes, 256 queries resident on the device in the
storage type):
  1M x 2560 bf16, 1M x 4096 bf16, 1M x 1536 fp32
Per shape and library three legs:
  shallow  one target per query, the query's rank-10 row
  deep     one target per query at rank ~ N / 2 (the row of median score in a block of the corpus): every score of the pass
           takes the compare path
  many     16 targets per query, ranks 10, 25, .. 235
Each figure is the median over --reps calls, after one warm-up call, of the whole call between two device events on the
index's stream; `kernel_ms` is the bracketed time of ts_index_profile_read per call (the counting launches of the matrix pass,
or the streaming passes of the fallback) and `launches_per_call` their number; `rank_sum` is the sum of the returned ranks (the
two libraries may differ by a few places in all: near-ties, added in different orders).

Every (shape, library) pair runs in a process of its own (TS_LIB selects the library); the libraries alternate, --rounds times,
and the figures of a pair are the medians over its rounds.  Where profiles/wide_timing.json holds the k-chunked search's full
pass at the shape (256 queries, k = 10), its bracketed time is copied beside the counting kernel's.

  python tools/rank_many_wide_timing.py [--parent-lib FILE] [--rows 1000000] [--reps 5] [--rounds 2]
                                        [--out profiles/rank_many_wide_timing.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("bf16", 2560), ("bf16", 4096), ("f32", 1536)]
LEGS = ("shallow", "deep", "many")
BLOCK = 50_000          # rows made and uploaded at a time
NQ = 256


def child(args):
    import numpy as np
    import torch

    import synthetic
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    dtype, d = SHAPES[args.shape]
    n = args.rows
    bf16 = dtype == "bf16"
    ix = ts.TheoremIndex(n, d, dtype=dtype, metric="ip")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234 + d)
    first = None
    for r0 in range(0, n, BLOCK):
        nb = min(BLOCK, n - r0)
        x = torch.randn((nb, d), generator=gen, device="cuda", dtype=torch.float32)
        x /= x.norm(dim=1, keepdim=True)
        torch.cuda.synchronize()
        ix.upload_device(x.data_ptr(), "f32", d, r0, nb)
        ix.synchronize()
        if first is None:
            first = x.clone()
    del x
    q = synthetic.synth_queries(0, NQ, d, bf16=bf16)
    qh = synthetic.bf16_bits_to_f32(q) if bf16 else q
    qd = torch.from_numpy(q.view(np.int16) if bf16 else q).cuda()
    # the targets: positions of the search's top 256, and per query the row of median score in the first block
    top = ix.search(qh, 256)[1]
    med = (torch.from_numpy(np.ascontiguousarray(qh)).cuda() @ first.T).argsort(dim=1)[:, first.shape[0] // 2].cpu().numpy()
    del first
    torch.cuda.synchronize()
    lists = {"shallow": [[int(top[i, 10])] for i in range(NQ)], "deep": [[int(med[i])] for i in range(NQ)],
             "many": [[int(top[i, 10 + 15 * j]) for j in range(16)] for i in range(NQ)]}
    timer = ts.Timer(0)
    st = ix.stream
    lib, h = ix._lib, ix._h
    legs = {}
    for name in LEGS:
        t = lists[name]
        off = np.zeros(NQ + 1, dtype=np.int64)
        np.cumsum([len(x) for x in t], out=off[1:])
        rows = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int64) for x in t]))
        ranks = np.empty(rows.shape[0], dtype=np.int64)
        scores = np.empty(rows.shape[0], dtype=np.float32)

        def call():
            _ffi.check(lib.ts_rank_many(h, C.c_void_p(qd.data_ptr()), _ffi.np_dtype_code(q), 1, NQ, _ffi.as_ptr(off), _ffi.as_ptr(rows),
                                        _ffi.as_ptr(ranks), _ffi.as_ptr(scores), None))
        call()
        ix.synchronize()
        ix.profile_enable(True)
        ix.profile_read()
        ms = []
        for _ in range(args.reps):
            timer.start(st)
            call()
            timer.stop(st)
            ix.synchronize()
            ms.append(timer.elapsed_ms())
        prof = ix.profile_read()
        ix.profile_enable(False)
        legs[name] = {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "kernel_ms": round(prof["total_ms"] / args.reps, 4),
                      "launches_per_call": prof["launches"] / args.reps, "median_rank": float(np.median(ranks)),
                      "rank_sum": int(ranks.sum())}
    ix.close()
    print("RESULT " + json.dumps({"dtype": dtype, "dim": d, "rows": n, "legs": legs}), flush=True)


def run_child(args, shape, lib, is_parent):
    env = dict(os.environ)
    if lib:
        env["TS_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shape", str(shape), "--rows", str(args.rows), "--reps", str(args.reps)]
    t0 = time.time()
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if p.returncode != 0:
        raise SystemExit(f"child failed ({p.returncode}): shape {shape}, lib {lib or 'this build'}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
    print(f"shape {SHAPES[shape]} {'parent' if is_parent else 'new'}: {time.time() - t0:.0f}s", file=sys.stderr, flush=True)
    return json.loads(line[7:])


def merge(rounds):
    """Median over rounds of every timing of every leg."""
    out = {}
    for name in rounds[0]["legs"]:
        ls = [r["legs"][name] for r in rounds]
        out[name] = {key: (statistics.median(x[key] for x in ls) if key in ("ms", "min_ms", "kernel_ms") else ls[-1][key]) for key in ls[0]}
        out[name]["ms_rounds"] = [x["ms"] for x in ls]
    return out


def search_full_pass_ms(dtype, d):
    """The k-chunked search's bracketed full pass at this shape (256 queries, k = 10), where profiles/wide_timing.json has it."""
    try:
        with open(os.path.join(ROOT, "profiles", "wide_timing.json")) as f:
            for s in json.load(f)["shapes"]:
                if s["dtype"] == dtype and s["dim"] == d:
                    return s["new"]["k10_nq256_mfma"]["pass_ms"]
    except (OSError, KeyError, ValueError):
        pass
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="libtsearch.so built from the parent commit")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_many_wide_timing.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {"rows": args.rows, "nq": NQ, "reps": args.reps, "rounds": args.rounds, "shapes": []}
    for shape in [int(x) for x in args.shapes.split(",")]:
        new, par = [], []
        for _ in range(args.rounds):
            new.append(run_child(args, shape, "", False))
            if args.parent_lib:
                par.append(run_child(args, shape, os.path.abspath(args.parent_lib), True))
        entry = {"dtype": SHAPES[shape][0], "dim": SHAPES[shape][1], "new": merge(new)}
        if par:
            entry["parent"] = merge(par)
            entry["parent_over_new"] = {name: round(entry["parent"][name]["ms"] / entry["new"][name]["ms"], 2) for name in LEGS}
            # the streaming passes add a score in another order than the matrix chain: targets in a near-tie may rank a place apart
            entry["rank_sum_new_minus_parent"] = {name: entry["new"][name]["rank_sum"] - entry["parent"][name]["rank_sum"] for name in LEGS}
        entry["search_full_pass_ms"] = search_full_pass_ms(*SHAPES[shape])
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        with open(args.out, "w") as f:          # after every shape: a later failure keeps what was measured
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
