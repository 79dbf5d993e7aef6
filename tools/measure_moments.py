#!/usr/bin/env python3
"""Times the corpus-moments pass (TheoremIndex.moments: ts_index_moments) on one GPU and sets each time beside two yardsticks
taken in the same run, on the same device:

* one corpus read at the stream rate the device delivers: leg 1 ("stream only") of tools/microbench/mfma_stream_ceiling.hip
  (build/libts_ceiling.so, built by __graft_entry__.build()) over a resident 768-wide bf16 corpus gives bytes per second; a
  shape's yardstick is its own bytes over that rate;
* torch's own ``X.T @ X`` over the same rows in the index's storage type (bf16 inputs, fp32 accumulation inside the GEMM;
  fp32 without TF32), over as many rows as ``--torch-rows`` allows, scaled per row.

Shapes: 10M x 768 bf16, 1M x 1024 bf16, 1M x 1024 fp32 (``--rows-scale`` shrinks them for a rehearsal).  Per shape: 3 warm-up
calls, then ``--calls`` (at least 20) timed calls; median, minimum, maximum and the quartiles.  Two times per call: the whole
call on the host clock (it ends in a stream synchronise and includes the copy of the d x d doubles to the host), and the Gram
kernel alone from the index's event bracket (ts_index_profile_*).  The rows are attached torch tensors (no host copy of 15 GB).
One JSON document: ``--out`` (default profiles/moments_<date>.json).  No GPU: it fails, it does not fall back."""
import argparse
import ctypes as C
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(10_000_000, 768, "bf16"), (1_000_000, 1024, "bf16"), (1_000_000, 1024, "f32")]


def spread(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4),
            "q1_ms": round(float(q1), 4), "q3_ms": round(float(q3), 4), "calls": int(a.size)}


def flops_and_bytes(n, d, elem):
    """what the pass computes and reads: the panel pairs on or above the diagonal as whole 128 x 128 tiles (a diagonal pair
    leaves out one 64 x 64 quadrant), two panels staged per pair (one on the diagonal), by every row"""
    panels = (d + 127) // 128
    width = [min(128, d - 128 * p) for p in range(panels)]
    macs = cols = 0
    for i in range(panels):
        for j in range(i, panels):
            macs += width[i] * width[j] - (64 * 64 if i == j else 0)
            cols += width[j] if i == j else width[i] + width[j]
    return 2.0 * n * macs, float(n) * cols * elem, float(n) * d * elem


def random_rows(torch, n, d, tdt):
    cap = (n + 255) // 256 * 256
    x = torch.zeros((cap, d), dtype=tdt, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    step = 1 << 20
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        x[r0:r1] = (torch.randn((r1 - r0, d), generator=g, device="cuda") * 0.05).to(tdt)
    return x, cap


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows-scale", type=float, default=1.0)
    ap.add_argument("--torch-rows", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", f"moments_{datetime.date.today():%Y%m%d}.json"))
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20 timed calls")
    import torch
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    if _ffi.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("measure_moments needs a GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    info = _ffi.device_info(0)
    doc = {"device": info["name"], "compute_units": info["compute_units"], "date": f"{datetime.date.today():%Y-%m-%d}",
           "how": f"{args.warmup} warm-up + {args.calls} timed calls per shape; call = host clock around ts_index_moments (ends in a "
                  "stream synchronise, includes the d x d double copy); gram_kernel = the index's event bracket around the pair kernel",
           "shapes": []}

    stream_gbs = None
    cl = C.CDLL(os.path.join(ROOT, "tools", "microbench", "build", "libts_ceiling.so"))
    cl.ts_ceiling_run.restype = C.c_int
    cl.ts_ceiling_run.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p]

    for n, d, dtype in SHAPES:
        n = max(256 * 64, int(n * args.rows_scale))
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        elem = 2 if dtype == "bf16" else 4
        x, cap = random_rows(torch, n, d, tdt)
        torch.cuda.synchronize()
        if stream_gbs is None:
            assert d == 768 and dtype == "bf16", "the stream yardstick runs on the first shape: 768-wide bf16"
            q = (torch.randn((256, 768), device="cuda") * 0.05).to(torch.bfloat16)
            ms4 = (C.c_double * 4)()
            rows_c = n // 32 * 32
            if cl.ts_ceiling_run(0, C.c_void_p(x.data_ptr()), rows_c, C.c_void_p(q.data_ptr()), 3, 5, ms4, None) != 0:
                sys.exit("the stream-rate leg failed")
            stream_gbs = rows_c * 768 * 2 / (ms4[1] * 1e-3) / 1e9
            doc["stream"] = {"rows": rows_c, "stream_only_ms": round(ms4[1], 4), "gb_per_s": round(stream_gbs, 1),
                             "how": "leg 1 of tools/microbench/mfma_stream_ceiling.hip, 3 rounds x 5 launches, this run, this corpus"}
        with ts.TheoremIndex(n, d, dtype=dtype, metric="ip") as ix:
            ix.attach_device(x.data_ptr(), cap, keep_alive=x)
            for _ in range(args.warmup):
                ix.moments()
            ix.profile_enable(True)
            ix.profile_read()
            call_ms, kern_ms = [], []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                cnt, s, g = ix.moments()
                call_ms.append((time.perf_counter() - t0) * 1e3)
                p = ix.profile_read()
                kern_ms.append(p["total_ms"] / max(1, p["launches"]))
            ix.profile_enable(False)
            sums_ms = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                ix.moments(gram=None)
                sums_ms.append((time.perf_counter() - t0) * 1e3)
            assert cnt == n
        # torch's GEMM over the same rows, scaled per row
        tn = min(n, args.torch_rows)
        xt = x[:tn]
        for _ in range(args.warmup):
            gt = xt.T @ xt
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch_ms = []
        for _ in range(args.calls):
            e0.record()
            gt = xt.T @ xt
            e1.record()
            e1.synchronize()
            torch_ms.append(e0.elapsed_time(e1) * n / tn)
        # the two agree (torch rounds its result to the storage type)
        ref = gt.float().cpu().numpy().astype(np.float64)
        if tn == n:
            rel = float(np.abs(g - ref).max() / np.abs(ref).max())
        else:
            rel = None
        fl, staged, corpus = flops_and_bytes(n, d, elem)
        call, kern, tor, sm = spread(call_ms), spread(kern_ms), spread(torch_ms), spread(sums_ms)
        read_ms = corpus / (stream_gbs * 1e9) * 1e3
        doc["shapes"].append({
            "rows": n, "d": d, "dtype": dtype, "call": call, "gram_kernel": kern, "sums_only_call": sm,
            "torch_xtx_scaled": dict(tor, rows_timed=tn), "one_corpus_read_ms": round(read_ms, 4),
            "flops": fl, "staged_bytes": staged, "corpus_bytes": corpus,
            "gram_kernel_tflops": round(fl / (kern["median_ms"] * 1e-3) / 1e12, 1),
            "gram_kernel_staged_gb_per_s": round(staged / (kern["median_ms"] * 1e-3) / 1e9, 1),
            "kernel_over_one_read": round(kern["median_ms"] / read_ms, 3), "call_over_one_read": round(call["median_ms"] / read_ms, 3),
            "kernel_over_torch": round(kern["median_ms"] / tor["median_ms"], 3), "call_over_torch": round(call["median_ms"] / tor["median_ms"], 3),
            "max_rel_diff_vs_torch": rel})
        print(json.dumps(doc["shapes"][-1]), flush=True)
        del x, xt, gt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
