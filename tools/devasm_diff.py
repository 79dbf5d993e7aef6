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


def compare_dirs(dir_a, dir_b, out=sys.stdout):
    """Prints the report; returns the number of differences (one-sided units and symbols count)."""
    a_units = {p.name: p for p in sorted(Path(dir_a).glob("*.s"))}
    b_units = {p.name: p for p in sorted(Path(dir_b).glob("*.s"))}
    ndiff = nfunc = ndesc = nunits = 0
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
    print("devasm_diff: %d units, %d functions, %d descriptors compared: %d differences" % (nunits, nfunc, ndesc, ndiff), file=out)
    return ndiff


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(1 if compare_dirs(sys.argv[1], sys.argv[2]) else 0)
