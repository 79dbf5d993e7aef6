#!/usr/bin/env python3
"""Compare two directories of device assembly listings (`make devasm`) per function symbol.

    python tools/devasm_diff.py DIR_A DIR_B

The gate of a change that must leave the device code as it is: build the listings of the parent commit and of the new
tree (with the Makefile's flags, and again with DEVASM_DEFS=-DTS_DIAG) and expect 0 differences.  Per unit (a `.s` file
of the same name on both sides) and per function symbol it compares
  * the instruction lines, with the function-local labels (.LBB<fn>_<n>, .Ltmp<n>, .Lfunc_*<n>) renumbered in order of first
    appearance and the per-build `__hip_cuid_*` symbol ignored, and
  * the values of the `.amdhsa_*` kernel descriptor.
It prints the units, functions and descriptors compared, every difference with its unit and symbol, and the symbols (or
units) present on one side only.  Exit status 0 = the same symbols on both sides and no difference.

    python tools/devasm_diff.py --summary DIR_A DIR_B

The gate of a change that may move a kernel's instructions but not what it costs: for every kernel whose instructions or
descriptor differ it prints a table of both sides - scratch and LDS bytes, .amdhsa_next_free_vgpr and the waves per SIMD it
allows, and the counts of v_mfma*, ds_read*, ds_write*, global_load*, global_store*, buffer_* and s_barrier lines - and whether
the static gate holds: scratch, LDS and every count unchanged, waves per SIMD not below side A's.  Exit status 0 = the same
symbols on both sides and no moved kernel fails it.
"""
import difflib
import re
import sys
from pathlib import Path

_LABEL = re.compile(r"\.L[A-Za-z_$]+[0-9]+(?:_[0-9]+)?")
_FUNC = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
_KD = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")


def _norm(line):
    line = line.split(";", 1)[0].split("//", 1)[0].strip()
    return re.sub(r"\s+", " ", line)


def parse(text):
    """-> (functions: {symbol: [normalised instruction lines]}, descriptors: {symbol: {field: value}})"""
    funcs, descs = {}, {}
    cur, kd, labels = None, None, {}
    for raw in text.splitlines():
        m = _FUNC.match(raw)
        if m:
            cur, labels = m.group(1), {}
            funcs[cur] = []
            continue
        m = _KD.match(raw)
        if m:
            kd = descs.setdefault(m.group(1), {})
            continue
        line = _norm(raw)
        if not line or "__hip_cuid_" in line:
            continue
        if kd is not None:
            if line == ".end_amdhsa_kernel":
                kd = None
            elif line.startswith(".amdhsa_"):
                field, _, value = line.partition(" ")
                kd[field] = value.strip()
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if line.startswith(".") and not line.endswith(":"):
            continue                                   # directives (.p2align, .cfi, .size ...) are not instructions
        if line == cur + ":":
            continue
        funcs[cur].append(_LABEL.sub(lambda k: labels.setdefault(k.group(0), ".L%d" % len(labels)), line))
    return funcs, descs


_STATIC_FIELDS = (".amdhsa_private_segment_fixed_size", ".amdhsa_group_segment_fixed_size")
_COUNTED = (("v_mfma", ("v_mfma",)), ("ds_read", ("ds_read", "ds_load")), ("ds_write", ("ds_write", "ds_store")),
            ("global_load", ("global_load",)), ("global_store", ("global_store",)), ("buffer", ("buffer_",)), ("s_barrier", ("s_barrier",)))


def waves_per_simd(next_free_vgpr):
    """gfx90a and later: 512 unified registers per lane of a SIMD, allocated in blocks of 8, at most 8 waves."""
    return min(8, 512 // max(8, -(-int(next_free_vgpr) // 8) * 8))


def static_row(lines, desc):
    """The figures a moved kernel must keep: scratch and LDS bytes, registers and the waves per SIMD they allow, and how many
    matrix, LDS, global, buffer and barrier instructions it holds."""
    row = {f[len(".amdhsa_"):]: desc.get(f) for f in _STATIC_FIELDS}
    row["next_free_vgpr"] = desc.get(".amdhsa_next_free_vgpr")
    row["waves_per_simd"] = waves_per_simd(row["next_free_vgpr"]) if row["next_free_vgpr"] is not None else None
    for name, prefixes in _COUNTED:
        row[name] = sum(1 for ln in lines if ln.startswith(prefixes))
    row["lines"] = len(lines)
    return row


def static_verdict(a, b):
    """'' when b keeps a's scratch, LDS and instruction counts and allows no fewer waves per SIMD, else what it broke."""
    bad = [k for k in a if k not in ("next_free_vgpr", "waves_per_simd", "lines") and a[k] != b[k]]
    if a["waves_per_simd"] is not None and b["waves_per_simd"] is not None and b["waves_per_simd"] < a["waves_per_simd"]:
        bad.append("waves_per_simd")
    return ", ".join(bad)


def compare_dirs(dir_a, dir_b, out=sys.stdout, summary=False):
    """Prints the report; returns the number of differences (one-sided units and symbols count).  summary: instead of the
    first differing lines, one static table row pair (static_row) per differing kernel and whether it holds (static_verdict)."""
    a_units = {p.name: p for p in sorted(Path(dir_a).glob("*.s"))}
    b_units = {p.name: p for p in sorted(Path(dir_b).glob("*.s"))}
    ndiff = nfunc = ndesc = nunits = nmoved = 0
    for name in sorted(set(a_units) ^ set(b_units)):
        print("unit %s: only in %s" % (name, dir_a if name in a_units else dir_b), file=out)
        ndiff += 1
    for name in sorted(set(a_units) & set(b_units)):
        nunits += 1
        fa, da = parse(a_units[name].read_text())
        fb, db = parse(b_units[name].read_text())
        for kind, xa, xb in (("function", fa, fb), ("descriptor", da, db)):
            for sym in sorted(set(xa) ^ set(xb)):
                print("%s: %s %s: only in %s" % (name, kind, sym, dir_a if sym in xa else dir_b), file=out)
                ndiff += 1
        if summary:
            nfunc += len(set(fa) & set(fb))
            ndesc += len(set(da) & set(db))
            for sym in sorted(set(fa) & set(fb) & set(da) & set(db)):
                if fa[sym] == fb[sym] and da[sym] == db[sym]:
                    continue
                nmoved += 1
                ra, rb = static_row(fa[sym], da[sym]), static_row(fb[sym], db[sym])
                bad = static_verdict(ra, rb)
                ndiff += 1 if bad else 0
                print("%s: %s: %s" % (name, sym, "STATIC GATE FAILS: " + bad if bad else "moved, static gate holds"), file=out)
                print("    %-28s %10s %10s" % ("", "a", "b"), file=out)
                for k in ra:
                    print("    %-28s %10s %10s%s" % (k, ra[k], rb[k], "" if ra[k] == rb[k] else "   *"), file=out)
            continue
        for sym in sorted(set(fa) & set(fb)):
            nfunc += 1
            if fa[sym] != fb[sym]:
                ndiff += 1
                print("%s: function %s: instructions differ (%d / %d lines)" % (name, sym, len(fa[sym]), len(fb[sym])), file=out)
                for d in list(difflib.unified_diff(fa[sym], fb[sym], "a", "b", n=0, lineterm=""))[2:22]:
                    print("    " + d, file=out)
        for sym in sorted(set(da) & set(db)):
            ndesc += 1
            for field in sorted(set(da[sym]) | set(db[sym])):
                if da[sym].get(field) != db[sym].get(field):
                    ndiff += 1
                    print("%s: descriptor %s: %s %s -> %s" % (name, sym, field, da[sym].get(field), db[sym].get(field)), file=out)
    if summary:
        print("devasm_diff: %d units, %d functions, %d descriptors compared: %d kernels moved, %d one-sided or failing the static gate"
              % (nunits, nfunc, ndesc, nmoved, ndiff), file=out)
    else:
        print("devasm_diff: %d units, %d functions, %d descriptors compared: %d differences" % (nunits, nfunc, ndesc, ndiff), file=out)
    return ndiff


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--summary"]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(1 if compare_dirs(args[0], args[1], summary="--summary" in sys.argv[1:]) else 0)
