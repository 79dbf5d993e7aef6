#!/usr/bin/env python3
"""A/B of the attention entry points of two builds of the library (the same C ABI): same bytes, same time.

    TS_LIB=.../libtsearch.so python tools/attention_ab.py --dump FILE.npz     # one process per library, needs a GPU
    python tools/attention_ab.py --compare A.npz B.npz                        # no GPU; exit 1 on any differing byte, key or shape
    TS_LIB=.../libtsearch.so python tools/attention_ab.py --time FILE.json    # one process per library and run, needs a GPU
    python tools/attention_ab.py --judge P1.json P2.json P3.json N1.json N2.json N3.json

--dump runs ts_attention_short, ts_attention_gqa, ts_attention_float and ts_attention_tiled on every case of `cases()` - seeded
N(0, 1.5^2) inputs from a CPU generator, as the tests use - and writes every output's raw bytes: bf16 as uint16, fp32 as uint32.
The cases reach every instantiation of the six attention kernels (every tile count T = 1 .. 8 of the bf16 kernels, R = 1, 2, 4,
both causal values, the three fp32 head sizes) next to every tile, query-block and chunk edge, under no mask, a padded tail and
a sequence without a single key.  One archive is about 860 MB (1,968 calls, 2,700 arrays, uncompressed: random outputs do not
compress): write it to a temporary directory, never into the repository tree, and keep only --compare's report.

--time reports, per row of `time_rows()` (the workload's shapes), the median over ROUNDS windows of CALLS calls between two
device events, after a warm-up.  --judge takes three runs of the parent and three of the new build, made alternately in one
job: a row passes when the new build's median is no slower than the parent's median plus the parent's own spread (max - min of
its three runs) - the noise the parent shows against itself.  Exit 1 when a row fails.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32_MAX_SEQ = {64: 512, 128: 256, 256: 128}          # attn_f32_max_seq (encoder_plan.h)
TILED_CHUNK = {64: 128, 128: 64, 256: 32}            # attn_tiled_chunk
MASKS = ("none", "tail", "keyless")
BF16_LENGTHS = tuple(s for t in range(1, 9) for s in (16 * t - 15, 16 * t - 1, 16 * t))
GQA_HEADS = ((2, 2), (4, 2), (4, 1))                 # (query heads, key / value heads): R = 1, 2, 4 of attention_gqa_rows_kernel
F32_HEADS = ((6, 2, 64), (4, 4, 128), (3, 1, 256))
CALLS, ROUNDS, WARMUP = 30, 7, 10


def gqa_rows_r(hq, hkv):
    """attn_gqa_plan's choice: the largest of 4, 2, 1 that divides the query heads per key / value head."""
    per = hq // hkv
    return 4 if per % 4 == 0 else 2 if per % 2 == 0 else 1


def f32_lengths(hd):
    c = TILED_CHUNK[hd]
    return sorted({1, 15, 16, 17, 63, 64, 65, c - 1, c, c + 1, 2 * c + 1, 4 * c + 17})


def cases():
    """Every call of the dump, in order: dicts of entry, B, S, hq, hkv, hd, causal, mask and (fp32) bias, want_out."""
    out = []
    for S in BF16_LENGTHS:
        for mask in MASKS:
            out.append(dict(entry="ts_attention_short", B=3, S=S, hq=3, hkv=3, hd=64, causal=0, mask=mask))
            for hq, hkv in GQA_HEADS:
                for causal in (0, 1):
                    out.append(dict(entry="ts_attention_gqa", B=3, S=S, hq=hq, hkv=hkv, hd=128, causal=causal, mask=mask))
    for hq, hkv, hd in F32_HEADS:
        for S in f32_lengths(hd):
            for mask in MASKS:
                for causal in (0, 1):
                    for bias in (0, 1):
                        for want_out in (1, 0):
                            for entry in ("ts_attention_float", "ts_attention_tiled"):
                                if entry == "ts_attention_float" and S > F32_MAX_SEQ[hd]:
                                    continue
                                out.append(dict(entry=entry, B=2, S=S, hq=hq, hkv=hkv, hd=hd, causal=causal, mask=mask, bias=bias,
                                                want_out=want_out))
    return out


def case_key(c):
    return "/".join("%s=%s" % (k, c[k]) for k in ("entry", "S", "hq", "hkv", "hd", "causal", "mask", "bias", "want_out") if k in c)


def key_mask(kind, B, S):
    """none -> None; tail: sequence b keeps its first max(1, S - 3 b - 1) keys; keyless: tail with sequence 1 all zeros."""
    import torch
    if kind == "none":
        return None
    keep = torch.tensor([max(1, S - 3 * b - 1) for b in range(B)])
    m = (torch.arange(S)[None, :] < keep[:, None]).to(torch.int64)
    if kind == "keyless":
        m[1] = 0
    return m


def time_rows():
    """The workload's shapes: (name, entry, B, S, hq, hkv, hd, causal)."""
    rows = []
    for S in (32, 128):
        rows.append(("bert bf16 256x%d" % S, "ts_attention_short", 256, S, 12, 12, 64, 0))
        rows.append(("qwen3 bf16 256x%d" % S, "ts_attention_gqa", 256, S, 16, 8, 128, 1))
    for hq, hkv, hd, causal in ((12, 12, 64, 0), (16, 8, 128, 1), (3, 1, 256, 0)):
        rows.append(("float fp32 head %d 256x128" % hd, "ts_attention_float", 256, 128, hq, hkv, hd, causal))
    for hq, hkv, hd, causal, lengths in ((12, 12, 64, 0, (384, 512)), (16, 8, 128, 1, (384, 512)), (3, 1, 256, 0, (192,))):
        for S in lengths:
            rows.append(("tiled fp32 head %d 256x%d" % (hd, S), "ts_attention_tiled", 256, S, hq, hkv, hd, causal))
    return rows


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
def _call(lib, c, qkv, mask, bias, out, pieces):
    import ctypes as C
    import torch

    def P(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if c["entry"] == "ts_attention_short":
        return lib.ts_attention_short(0, P(qkv), P(mask), c["B"], c["S"], c["hq"], c["hd"], P(out), st)
    if c["entry"] == "ts_attention_gqa":
        return lib.ts_attention_gqa(0, P(qkv), P(mask), c["B"], c["S"], c["hq"], c["hkv"], c["hd"], c["causal"], P(out), st)
    return getattr(lib, c["entry"])(0, P(qkv), P(bias), P(mask), c["B"], c["S"], c["hq"], c["hkv"], c["hd"], c["causal"], c["hd"] ** -0.5,
                                    P(out), P(pieces), st)


def _inputs(c, g):
    import torch
    fp32 = c["entry"] in ("ts_attention_float", "ts_attention_tiled")
    width = (c["hq"] + 2 * c["hkv"]) * c["hd"]
    qkv = torch.randn(c["B"], c["S"], width, generator=g, device=g.device) * 1.5
    bias = torch.randn(width, generator=g, device=g.device).cuda() if c.get("bias") else None
    return (qkv if fp32 else qkv.to(torch.bfloat16)).cuda(), bias, fp32


def _outputs(c, fp32):
    import torch
    B, S, d = c["B"], c["S"], c["hq"] * c["hd"]
    if not fp32:
        return torch.zeros((B, S, d), dtype=torch.bfloat16, device="cuda"), None
    out = torch.zeros((B, S, d), dtype=torch.float32, device="cuda") if c.get("want_out", 1) else None
    return out, torch.zeros((B * S, 3 * d), dtype=torch.bfloat16, device="cuda")


def dump(path):
    import torch
    from theoremsearch_amd import _ffi
    lib = _ffi.load()
    g = torch.Generator(device="cpu").manual_seed(52000)
    arrays = {}
    for c in cases():
        qkv, bias, fp32 = _inputs(c, g)
        mask = key_mask(c["mask"], c["B"], c["S"])
        mask = None if mask is None else mask.cuda()
        out, pieces = _outputs(c, fp32)
        _ffi.check(_call(lib, c, qkv, mask, bias, out, pieces))
        torch.cuda.synchronize()
        if out is not None:
            arrays[case_key(c) + "/out"] = out.view(torch.int32 if fp32 else torch.int16).cpu().numpy().view(np.uint32 if fp32 else np.uint16)
        if pieces is not None:
            arrays[case_key(c) + "/pieces"] = pieces.view(torch.int16).cpu().numpy().view(np.uint16)
    np.savez(path, **arrays)
    print("attention_ab: %d calls, %d arrays, %.1f MB from %s -> %s" % (len(cases()), len(arrays), sum(a.nbytes for a in arrays.values()) / 1e6,
                                                                         _ffi.lib_path(), path))


def time_entries(path):
    import torch
    from theoremsearch_amd import _ffi
    lib = _ffi.load()
    g = torch.Generator(device="cuda").manual_seed(53000)         # (timing inputs: up to 2 GB a row, made where they are used)
    rows = {}
    for name, entry, B, S, hq, hkv, hd, causal in time_rows():
        c = dict(entry=entry, B=B, S=S, hq=hq, hkv=hkv, hd=hd, causal=causal, want_out=1)
        qkv, bias, fp32 = _inputs(c, g)
        out, pieces = _outputs(c, fp32)
        for _ in range(WARMUP):
            _ffi.check(_call(lib, c, qkv, None, bias, out, pieces))
        torch.cuda.synchronize()
        windows = []
        for _ in range(ROUNDS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(CALLS):
                _call(lib, c, qkv, None, bias, out, pieces)
            t1.record()
            t1.synchronize()
            windows.append(t0.elapsed_time(t1) * 1000.0 / CALLS)
        rows[name] = {"us_per_call": statistics.median(windows), "min": min(windows), "max": max(windows)}
    with open(path, "w") as f:
        json.dump({"lib": _ffi.lib_path(), "calls": CALLS, "rounds": ROUNDS, "rows": rows}, f, indent=1)
    print("attention_ab: %d rows from %s -> %s" % (len(rows), _ffi.lib_path(), path))


# ---- the CPU side ------------------------------------------------------------------------------------------------------------------
def compare(path_a, path_b, out=sys.stdout):
    """-> the number of keys that are missing on a side, differ in shape or dtype, or differ in any byte."""
    a, b = np.load(path_a), np.load(path_b)
    bad = 0
    for k in sorted(set(a.files) ^ set(b.files)):
        print("%s: only in %s" % (k, path_a if k in a.files else path_b), file=out)
        bad += 1
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype:
            print("%s: %s %s against %s %s" % (k, x.dtype, x.shape, y.dtype, y.shape), file=out)
            bad += 1
        elif x.tobytes() != y.tobytes():
            print("%s: %d of %d elements differ" % (k, int((x != y).sum()), x.size), file=out)
            bad += 1
    print("attention_ab: %d arrays in %s, %d in %s: %d differ" % (len(a.files), path_a, len(b.files), path_b, bad), file=out)
    return bad


def judge(parent_paths, new_paths, out=sys.stdout):
    """-> the number of rows where the new median is slower than the parent's median + the parent's spread."""
    def load(paths):
        return [json.load(open(p))["rows"] for p in paths]
    parent, new = load(parent_paths), load(new_paths)
    bad = 0
    print("%-32s %10s %10s %10s %10s  %s" % ("row (us per call)", "parent", "spread", "new", "allowed", ""), file=out)
    for name in parent[0]:
        p = [r[name]["us_per_call"] for r in parent]
        n = [r[name]["us_per_call"] for r in new]
        pm, spread, nm = statistics.median(p), max(p) - min(p), statistics.median(n)
        ok = nm <= pm + spread
        bad += 0 if ok else 1
        print("%-32s %10.2f %10.2f %10.2f %10.2f  %s" % (name, pm, spread, nm, pm + spread, "pass" if ok else "FAIL"), file=out)
    print("attention_ab: %d rows, %d slower than the parent's median + spread" % (len(parent[0]), bad), file=out)
    return bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", metavar="FILE")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--time", metavar="FILE")
    ap.add_argument("--judge", nargs="+", metavar="JSON", help="the parent's three --time files, then the new build's three")
    args = ap.parse_args()
    if args.dump:
        dump(args.dump)
    elif args.time:
        time_entries(args.time)
    elif args.compare:
        sys.exit(1 if compare(*args.compare) else 0)
    elif args.judge:
        if len(args.judge) != 6:
            ap.error("--judge takes six files: three runs of the parent (its spread is their max - min), then three of the new build")
        sys.exit(1 if judge(args.judge[:3], args.judge[3:]) else 0)
    else:
        ap.error("one of --dump, --compare, --time, --judge")
