"""The fp32 screen's unit (launch_screen8_f32.hip; kernels_screen8_f32.h) in the compiled gfx950 ISA: the exact rescore exists
for both widths and multiplies with v_mfma_f32_16x16x4_f32 - the fp32 pass's instruction - and nothing else: W / 4 of them per
chunk in one chain; no kernel of the unit uses scratch or spills, and VGPRs + AGPRs stay within the 512 registers a lane of a
256-thread workgroup can have; the row streams through counted waits (never a drain inside the chain) and no compiler-made
vector instruction writes an MFMA operand right in front of its MFMA (the MFMAs are asm text: hipcc pads no hazard for them).
The unit holds no tile kernel of its own: the screen launched for an fp32 index is mfma16_topk_kernel<384 / 512, NB, 8 / 14> of
launch_screen8.hip / launch_screen8_wide.hip, the very symbols tests/test_screen8_isa_cpu.py and its neighbours check."""
import os
import re

import pytest

from isa_common import CSRC, audit_ring, device_asm

MFMA = "v_mfma_f32_16x16x4_f32"
UNIT = "launch_screen8_f32"


def functions(text):
    """{symbol: [(line number, line)]} of every function of the listing."""
    out, cur = {}, None
    for no, ln in enumerate(text.splitlines(), 1):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is not None:
            cur.append((no, ln))
            if ln.startswith(".Lfunc_end"):
                cur = None
    return out


def instructions(lines):
    out = []
    for _, ln in lines:
        s = ln.split(";")[0].strip()
        if s and not s.endswith(":") and not s.startswith("."):
            out.append(s)
    return out


def usage_by_function(usage):
    """{symbol: {field: int}} of the -Rpass-analysis=kernel-resource-usage report."""
    out, cur = {}, None
    for ln in usage.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: [^ ]+\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


@pytest.mark.timeout(900)
def test_f32_screen_unit_isa():
    asm, text, usage = device_asm(UNIT)
    fns = functions(text)
    # the three kernels of the unit, at both widths - and no tile kernel, no other matrix instruction
    for w in (768, 1024):
        for name in ("quantize_tiles_f32_kernelILi%dE" % w, "quantize_queries_f32_kernelILi%dE" % w, "screen_rescore_f32_kernelILi%dE" % w):
            assert [f for f in fns if re.match(r"_ZN2ts\d+%s" % name, f)], name
    assert not [f for f in fns if "mfma16_topk_kernel" in f], "the tile kernel lives in launch_screen8.hip / launch_screen8_wide.hip"
    opcodes = set(re.findall(r"^\s*(v_mfma\w+|v_smfma\w+)", text, re.M))
    assert opcodes == {MFMA}, opcodes
    code = "\n".join(l.split("//")[0] for l in open(os.path.join(CSRC, UNIT + ".hip")).read().splitlines())
    assert "screen_tile_pass(" in code and "mfma16_topk_kernel" not in code, "the screen is launched through the units that hold it"
    # registers: per kernel, no scratch, no spill, VGPRs + AGPRs within the 512 of a lane at 256 threads per workgroup
    use = usage_by_function(usage)
    assert len(use) == 6, sorted(use)
    for f, u in use.items():
        assert u["ScratchSize"] == 0 and u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0, (f, u)
        assert u["VGPRs"] + u["AGPRs"] <= 512, (f, u)
        print(f, "VGPRs", u["VGPRs"], "AGPRs", u["AGPRs"], "occupancy", u.get("Occupancy"))
    for w in (768, 1024):
        (f,) = [f for f in fns if "screen_rescore_f32_kernelILi%dE" % w in f]
        ins = instructions(fns[f])
        mm = [i for i, l in enumerate(ins) if l.startswith(MFMA)]
        # one chain of W / 4 MFMAs: the first from a zero accumulator, every other one adds to the accumulator it writes
        assert len(mm) == w // 4, (w, len(mm))
        acc = ins[mm[0]].split()[1].rstrip(",")
        assert ins[mm[0]].endswith(", 0"), ins[mm[0]]
        for i in mm[1:]:
            ops = [o.strip() for o in ins[i].split(None, 1)[1].split(",")]
            assert ops[0] == acc and ops[3] == acc, ins[i]
            assert ops[2].startswith("a"), ins[i]                      # the query comes from the accumulator file
        # the row streams: loads of later chunks sit among the MFMAs, and inside the chain the waits are counted, never a drain
        chain = ins[mm[0]:mm[-1] + 1]
        assert sum(l.startswith("global_load_dwordx4") for l in chain) == w // 16 - 16, w
        assert not [l for l in chain if l.startswith(("flat_", "scratch_", "buffer_"))]
        waits = [l for l in chain[:chain.index([l for l in chain if l.startswith("global_load_dwordx4")][-1])] if l.startswith("s_waitcnt") and "vmcnt" in l]
        assert waits and "s_waitcnt vmcnt(0)" not in waits, waits[:4]
        # no compiler-made vector instruction writes an MFMA operand right in front of it (tools/audit_ring.py, second check)
        bad = audit_ring.audit(f, fns[f])
        assert not bad, bad[:5]
