"""What the ISA tests share: the device assembly of a translation unit of theoremsearch_amd/csrc, compiled for gfx950 by the
Makefile's own `asm` target (its CXXFLAGS, so the listing is the library's code) at most once per pytest process, and the
walks over a kernel's listing.  No GPU needed: hipcc cross-compiles."""
import atexit
import collections
import functools
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "theoremsearch_amd", "csrc")

sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import audit_ring  # noqa: F401  (the tests call audit_ring.main / audit_ring.audit)
finally:
    sys.path.pop(0)

DeviceAsm = collections.namedtuple("DeviceAsm", "path text usage")


def hipcc_or_skip():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    return hipcc


@functools.lru_cache(maxsize=None)
def _asm_dir():
    tmp = tempfile.mkdtemp(prefix="tsearch_asm_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)      # tens of MB of intermediates per unit
    return tmp


@functools.lru_cache(maxsize=None)
def device_asm(unit):
    """(path, text, usage) of `unit`.hip: its gfx950 assembly file, that file's text, and the compiler's
    -Rpass-analysis=kernel-resource-usage report."""
    hipcc = hipcc_or_skip()
    r = subprocess.run(["make", "-C", CSRC, "asm", "HIPCC=" + hipcc, "ASM_UNITS=" + unit, "ASM_DIR=" + _asm_dir()],
                       capture_output=True, text=True, timeout=850)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    path = os.path.join(_asm_dir(), unit + "-hip-amdgcn-amd-amdhsa-gfx950.s")
    return DeviceAsm(path, open(path).read(), open(os.path.join(_asm_dir(), unit + ".resource_usage.txt")).read())


def kernel_body(text, d, nb, variant):
    """Instructions and labels of mfma16_topk_kernel<d, nb, variant> (the other template arguments at their defaults), without
    comments and directives."""
    m = re.search(r"^_ZN2ts18mfma16_topk_kernelILi%dELi%dELi%dELb0ELb0ELb0ELb0EEEvNS_8MfmaArgsE:[^\n]*\n(.*?)\n\.Lfunc_end" % (d, nb, variant),
                  text, re.S | re.M)
    assert m, "no mfma16_topk_kernel<%d, %d, %d>" % (d, nb, variant)
    out = []
    for line in m.group(1).split("\n"):
        s = line.split(";")[0].strip()
        if s and not (s.startswith(".") and not s.endswith(":")):
            out.append(s)
    return out


def _successors(ins):
    labels = {l[:-1]: i for i, l in enumerate(ins) if l.endswith(":")}
    succ = []
    for i, l in enumerate(ins):
        op = l.split()[0]
        assert not op.startswith(("s_setpc", "s_swappc", "s_call")), l      # no indirect control flow to follow
        if op == "s_endpgm":
            succ.append([])
        elif op == "s_branch":
            succ.append([labels[l.split()[1]]])
        elif op.startswith("s_cbranch"):
            succ.append([labels[l.split()[1]]] + ([i + 1] if i + 1 < len(ins) else []))
        else:
            succ.append([i + 1] if i + 1 < len(ins) else [])
    return succ


def _closure(start, edges):
    seen, todo = set(start), list(start)
    while todo:
        for j in edges[todo.pop()]:
            if j not in seen:
                seen.add(j)
                todo.append(j)
    return seen


def tile_loop(ins):
    """Indices of the instructions between the first barrier and the last one in execution order: reachable from the first
    s_barrier of the listing, and with a path to some s_barrier."""
    succ = _successors(ins)
    pred = [[] for _ in ins]
    for i, ss in enumerate(succ):
        for j in ss:
            pred[j].append(i)
    bars = [i for i, l in enumerate(ins) if l.startswith("s_barrier")]
    assert len(bars) >= 2, bars
    return sorted(_closure([bars[0]], succ) & _closure(bars, pred))
