"""Timing of the batched search at the row widths the k-chunked matrix kernel serves (kernels_mfma_wide.h: rows of more than
4,096 and at most 16,384 bytes, d % 256 == 0) against the streaming scan, and against a library built from the parent commit
(where algo = auto is the scan at these widths and algo = mfma is refused).

Shapes (seeded random-normal unit rows made on the device, inner-product indexes, queries resident on the device in the
storage type):
  1M x 2560 bf16, 1M x 4096 bf16, 1M x 1536 fp32
Per shape and library: k = 10, batches of 5, 8, 16, 64 and 256 queries through algo = scan, mfma (this build only) and auto;
k = 100 (the scan serves one query per pass there) at 2, 4 and 8 queries.  This build also runs the 256-query pass in the plain
two-barrier form (TS_MFMA_WIDE_SERIAL = 1): the A/B partner of the one-barrier form.  Each figure is the median over --reps
calls, after one warm-up call, of the whole call between two device events on the index's stream; `pass_ms` is the bracketed
kernel time of ts_index_profile_read per call (the full pass of the matrix path / the sum of a call's scan passes), `tb_s` the
corpus bytes over it.

Every (shape, library) pair runs in a process of its own (TS_LIB selects the library); the libraries alternate, --rounds
times, and the figures of a pair are the medians over its rounds.

  python tools/wide_timing.py [--parent-lib FILE] [--rows 1000000] [--reps 7] [--rounds 2] [--out profiles/wide_timing.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("bf16", 2560), ("bf16", 4096), ("f32", 1536)]
BATCHES = (5, 8, 16, 64, 256)
BATCHES_K100 = (2, 4, 8)
BLOCK = 50_000          # rows made and uploaded at a time


def child(args):
    import numpy as np
    import torch

    import synthetic
    import theoremsearch_amd as ts
    dtype, d = SHAPES[args.shape]
    n = args.rows
    bf16 = dtype == "bf16"
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
    q = synthetic.synth_queries(0, 256, d, bf16=bf16)
    qd = torch.from_numpy(q.view(np.int16) if bf16 else q).cuda()
    out_s = torch.empty((256, 100), dtype=torch.float32, device="cuda")
    out_i = torch.empty((256, 100), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    timer = ts.Timer(0)
    st = ix.stream
    algos = ("scan", "auto") if args.is_parent else ("scan", "mfma", "auto")
    corpus_tb = n * d * (2 if bf16 else 4) / 1e12
    legs = {}

    def leg(k, nq, algo, name=None):
        def call():
            ix.search_device(qd.data_ptr(), dtype, nq, k, out_s.data_ptr(), out_i.data_ptr(), st, algo=algo)
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
        # which path AUTO took: a host call with statistics
        qh = synthetic.bf16_bits_to_f32(q[:nq]) if bf16 else q[:nq]
        used = ix.search(qh, k, algo=algo, return_stats=True)[2]
        pass_ms = prof["total_ms"] / args.reps
        launches = prof["launches"] / args.reps
        legs[name or f"k{k}_nq{nq}_{algo}"] = {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "pass_ms": round(pass_ms, 4),
                                               "launches_per_call": launches, "tb_s": round(corpus_tb * launches / (pass_ms * 1e-3), 3) if pass_ms > 0 else 0.0,
                                               "algo": used["algo"], "fallback_queries": used["fallback_queries"]}

    for nq in BATCHES:
        for algo in algos:
            leg(10, nq, algo)
    for nq in BATCHES_K100:
        for algo in algos:
            leg(100, nq, algo)
    if not args.is_parent:
        ix.set_option("TS_MFMA_WIDE_SERIAL", 1)
        leg(10, 256, "mfma", "k10_nq256_mfma_serial")
        ix.set_option("TS_MFMA_WIDE_SERIAL", None)
    ix.close()
    print("RESULT " + json.dumps({"dtype": dtype, "dim": d, "rows": n, "legs": legs}), flush=True)


def run_child(args, shape, lib, is_parent):
    env = dict(os.environ)
    if lib:
        env["TS_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shape", str(shape), "--rows", str(args.rows), "--reps", str(args.reps)]
    if is_parent:
        cmd.append("--is-parent")
    t0 = time.time()
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if p.returncode != 0:
        raise SystemExit(f"child failed ({p.returncode}): shape {shape}, lib {lib or 'this build'}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
    print(f"shape {SHAPES[shape]} {'parent' if is_parent else 'new'}: {time.time() - t0:.0f}s", file=sys.stderr, flush=True)
    return json.loads(line[7:])


def merge(rounds):
    """Median over rounds of every figure of every leg."""
    out = {}
    for name in rounds[0]["legs"]:
        ls = [r["legs"][name] for r in rounds]
        out[name] = {key: (statistics.median(x[key] for x in ls) if key in ("ms", "min_ms", "pass_ms", "tb_s") else ls[-1][key]) for key in ls[0]}
        out[name]["ms_rounds"] = [x["ms"] for x in ls]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="libtsearch.so built from the parent commit")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_timing.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--is-parent", action="store_true")
    ap.add_argument("--shape", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {"rows": args.rows, "reps": args.reps, "rounds": args.rounds, "k": 10, "shapes": []}
    for shape in [int(x) for x in args.shapes.split(",")]:
        new, par = [], []
        for _ in range(args.rounds):
            new.append(run_child(args, shape, "", False))
            if args.parent_lib:
                par.append(run_child(args, shape, os.path.abspath(args.parent_lib), True))
        entry = {"dtype": SHAPES[shape][0], "dim": SHAPES[shape][1], "new": merge(new)}
        if par:
            entry["parent"] = merge(par)
            entry["parent_auto_over_new_auto"] = {
                f"k{k}_nq{nq}": round(entry["parent"][f"k{k}_nq{nq}_auto"]["ms"] / entry["new"][f"k{k}_nq{nq}_auto"]["ms"], 2)
                for k, bs in ((10, BATCHES), (100, BATCHES_K100)) for nq in bs}
        entry["scan_over_mfma"] = {f"k{k}_nq{nq}": round(entry["new"][f"k{k}_nq{nq}_scan"]["ms"] / entry["new"][f"k{k}_nq{nq}_mfma"]["ms"], 3)
                                   for k, bs in ((10, BATCHES), (100, BATCHES_K100)) for nq in bs}
        entry["serial_over_one_barrier_pass"] = round(entry["new"]["k10_nq256_mfma_serial"]["pass_ms"] / entry["new"]["k10_nq256_mfma"]["pass_ms"], 3)
        res["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        with open(args.out, "w") as f:          # after every shape: a later failure keeps what was measured
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
