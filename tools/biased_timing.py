"""Timing of the batched citation-weighted search (ts_search_biased_ex: the biased general-width matrix pass, kernels_mfma_anyd.h
with the bias term in its epilogue) against a library built from the parent commit, whose only biased search is
ts_search_biased - the scan, four queries per pass.

Shapes (seeded synthetic corpora, inner-product indexes, queries and bias resident on the device, queries in the storage type):
  1M x 768 bf16, 1M x 1024 bf16, 1M x 768 fp32, 1M x 1536 bf16
Bias: the citation recipe of the tests (no bonus for a fifth of the rows, ln(1..399), twelve rows at ln(1e6..1e8)), w = 0.02.
Per shape and library: k = 10, batches of 5, 8, 16, 64 and 256 queries; this build through algo = scan, mfma and auto, the
parent through ts_search_biased.  Each figure is the median over --reps calls, after one warm-up call, of the whole call
between two device events on the index's stream; `pass_ms` is the bracketed kernel time of ts_index_profile_read per call.
On 1M x 1536 bf16 the plain search (algo = mfma, the general-width pass without the term) is timed at 256 queries too.

Every (shape, library) pair runs in a process of its own (TS_LIB selects the library); the libraries alternate, --rounds
times, and the figures of a pair are the medians over its rounds.

--rerun-share: instead of timing, the share of queries the biased matrix search sends to the exact re-run, on --rerun-rows x 768
bf16, 256 queries, k = 10 and k = 100, under the tests' recipe (w = 0.02) and under power-law citation counts (w = 0.05).

  python tools/biased_timing.py [--parent-lib FILE] [--rows 1000000] [--reps 7] [--rounds 2] [--out profiles/biased_timing.json]
  python tools/biased_timing.py --rerun-share [--rerun-rows 1000000,10000000]
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

SHAPES = [("bf16", 768), ("bf16", 1024), ("f32", 768), ("bf16", 1536)]
BATCHES = (5, 8, 16, 64, 256)
W = 0.02


def recipe_bias(n, kind="test"):
    import numpy as np
    rng = np.random.default_rng(9)
    if kind == "powerlaw":            # citation counts with a power-law tail: most rows 1 (no bonus), a few in the thousands
        return np.log(rng.zipf(2.0, n).astype(np.float64)).astype(np.float32)
    u, v = rng.random(n), rng.integers(1, 400, n)
    cites = np.where(u < 0.2, 0, v).astype(np.float64)
    cites[rng.choice(n, 12, replace=False)] = 10.0 ** rng.integers(6, 9, 12)
    return np.where(cites > 0, np.log(np.maximum(cites, 1.0)), 0.0).astype(np.float32)


def build_index(ts, n, d, dtype):
    from concurrent.futures import ThreadPoolExecutor

    import synthetic
    CH = synthetic.CHUNK_ROWS
    ix = ts.TheoremIndex(n, d, dtype=dtype, metric="ip")

    def make(c):
        a, b = c * CH, min(n, (c + 1) * CH)
        ix.upload(synthetic.synth_chunk(c, CH, d, bf16=dtype == "bf16")[: b - a], a)

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(make, range((n + CH - 1) // CH)))
    return ix


def child(args):
    import numpy as np
    import torch

    import synthetic
    from theoremsearch_amd import _ffi
    if args.is_parent:
        _ffi._SIGNATURES.pop("ts_search_biased_ex", None)        # the parent's library does not export it
    import theoremsearch_amd as ts
    lib = _ffi.load()
    dtype, d = SHAPES[args.shape]
    n = args.rows
    bf16 = dtype == "bf16"
    ix = build_index(ts, n, d, dtype)
    q = synthetic.synth_queries(0, 256, d, bf16=bf16)
    qd = torch.from_numpy(q.view(np.int16) if bf16 else q).cuda()
    bd = torch.from_numpy(recipe_bias(n)).cuda()
    out_s = torch.empty((256, 10), dtype=torch.float32, device="cuda")
    out_m = torch.empty((256, 10), dtype=torch.float32, device="cuda")
    out_i = torch.empty((256, 10), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    timer = ts.Timer(0)
    st = ix.stream
    qcode = _ffi.TS_BF16 if bf16 else _ffi.TS_F32
    legs = {}

    def biased(nq, algo):
        if algo == "parent":
            _ffi.check(lib.ts_search_biased(ix.handle, C.c_void_p(qd.data_ptr()), qcode, 1, nq, 10, C.c_void_p(bd.data_ptr()), 1, W, None, 0,
                                            C.c_void_p(out_s.data_ptr()), C.c_void_p(out_m.data_ptr()), C.c_void_p(out_i.data_ptr()), 1,
                                            C.c_void_p(st)))
        elif algo == "plain":
            ix.search_device(qd.data_ptr(), dtype, nq, 10, out_s.data_ptr(), out_i.data_ptr(), st, algo="mfma")
        else:
            ix.search_biased_device(qd.data_ptr(), dtype, nq, 10, bd.data_ptr(), W, out_s.data_ptr(), out_m.data_ptr(), out_i.data_ptr(), st,
                                    algo=algo)

    def leg(nq, algo):
        biased(nq, algo)
        ix.synchronize()
        ix.profile_enable(True)
        ix.profile_read()
        ms = []
        for _ in range(args.reps):
            timer.start(st)
            biased(nq, algo)
            timer.stop(st)
            ix.synchronize()
            ms.append(timer.elapsed_ms())
        prof = ix.profile_read()
        ix.profile_enable(False)
        legs[f"nq{nq}_{algo}"] = {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                                  "pass_ms": round(prof["total_ms"] / args.reps, 4), "launches_per_call": prof["launches"] / args.reps}
        if algo in ("mfma", "auto"):      # which path was taken, and the re-runs: a host call with statistics
            qh = synthetic.bf16_bits_to_f32(q[:nq]) if bf16 else q[:nq]
            used = ix.search_biased(qh, 10, bd.cpu().numpy(), W, algo=algo, return_stats=True)[3]
            legs[f"nq{nq}_{algo}"].update({"algo": used["algo"], "fallback_queries": used["fallback_queries"],
                                           "candidates_per_query": round(used["candidates"] / nq, 1)})

    for nq in BATCHES:
        for algo in (("parent",) if args.is_parent else ("scan", "mfma", "auto")):
            leg(nq, algo)
    if not args.is_parent and (dtype, d) == ("bf16", 1536):
        leg(256, "plain")
    ix.close()
    print("RESULT " + json.dumps({"dtype": dtype, "dim": d, "rows": n, "legs": legs}), flush=True)


def rerun_child(args):
    import synthetic
    import theoremsearch_amd as ts
    n, d = args.rows, 768
    ix = build_index(ts, n, d, "bf16")
    qh = synthetic.bf16_bits_to_f32(synthetic.synth_queries(0, 256, d, bf16=True))
    out = {}
    for kind, w in (("test", 0.02), ("powerlaw", 0.05)):
        bias = recipe_bias(n, kind)
        for k in (10, 100):
            st = ix.search_biased(qh, k, bias, w, algo="mfma", return_stats=True)[3]
            out[f"{kind}_w{w}_k{k}"] = {"rerun_queries": st["fallback_queries"], "of": 256, "candidates_per_query": round(st["candidates"] / 256, 1),
                                        "algo": st["algo"], "levels": st["levels"]}
    ix.close()
    print("RESULT " + json.dumps({"dtype": "bf16", "dim": d, "rows": n, "cases": out}), flush=True)


def run_child(args, extra, lib, label):
    env = dict(os.environ)
    if lib:
        env["TS_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps)] + extra
    t0 = time.time()
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if p.returncode != 0:
        raise SystemExit(f"child failed ({p.returncode}): {label}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
    print(f"{label}: {time.time() - t0:.0f}s", file=sys.stderr, flush=True)
    return json.loads(line[7:])


def merge(rounds):
    """Median over rounds of every figure of every leg."""
    out = {}
    for name in rounds[0]["legs"]:
        ls = [r["legs"][name] for r in rounds]
        out[name] = {key: (statistics.median(x[key] for x in ls) if key in ("ms", "min_ms", "pass_ms") else ls[-1][key]) for key in ls[0]}
        out[name]["ms_rounds"] = [x["ms"] for x in ls]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="libtsearch.so built from the parent commit")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--shapes", default="0,1,2,3")
    ap.add_argument("--child-timeout", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "biased_timing.json"))
    ap.add_argument("--rerun-share", action="store_true")
    ap.add_argument("--rerun-rows", default="1000000,10000000")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rerun-child", action="store_true")
    ap.add_argument("--is-parent", action="store_true")
    ap.add_argument("--shape", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.rerun_child:
        return rerun_child(args)
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)

    def save():
        with open(args.out, "w") as f:          # after every shape: a later failure keeps what was measured
            f.write(json.dumps(res, indent=1) + "\n")

    if args.rerun_share:
        res["rerun_share"] = []
        for rows in [int(x) for x in args.rerun_rows.split(",")]:
            r = run_child(args, ["--rerun-child", "--rows", str(rows)], "", f"re-run share, {rows} rows")
            res["rerun_share"].append(r)
            print(json.dumps(r), flush=True)
            save()
        return
    res.update({"rows": args.rows, "reps": args.reps, "rounds": args.rounds, "k": 10, "weight": W, "shapes": []})
    for shape in [int(x) for x in args.shapes.split(",")]:
        new, par = [], []
        for _ in range(args.rounds):
            new.append(run_child(args, ["--child", "--shape", str(shape), "--rows", str(args.rows)], "", f"shape {SHAPES[shape]} new"))
            if args.parent_lib:
                par.append(run_child(args, ["--child", "--is-parent", "--shape", str(shape), "--rows", str(args.rows)],
                                     os.path.abspath(args.parent_lib), f"shape {SHAPES[shape]} parent"))
        entry = {"dtype": SHAPES[shape][0], "dim": SHAPES[shape][1], "new": merge(new)}
        if par:
            entry["parent"] = merge(par)
            entry["parent_over_new_auto"] = {str(nq): round(entry["parent"][f"nq{nq}_parent"]["ms"] / entry["new"][f"nq{nq}_auto"]["ms"], 2)
                                             for nq in BATCHES}
        entry["scan_over_mfma"] = {str(nq): round(entry["new"][f"nq{nq}_scan"]["ms"] / entry["new"][f"nq{nq}_mfma"]["ms"], 3) for nq in BATCHES}
        if "nq256_plain" in entry["new"]:
            entry["biased_over_plain_pass"] = round(entry["new"]["nq256_mfma"]["pass_ms"] / entry["new"]["nq256_plain"]["pass_ms"], 3)
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        save()


if __name__ == "__main__":
    main()
