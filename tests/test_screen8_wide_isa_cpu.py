"""The d = 1024 int8 screen's unit (launch_screen8_wide.hip) in the compiled gfx950 ISA, as tests/test_screen8_isa_cpu.py and
its neighbours check the d = 768 unit: no register of the fragment ring is read while its load is in flight and no operand is
written right in front of its MFMA (tools/audit_ring.py); the product kernels mfma16_topk_kernel<512, 1 .. 4, 8> (unmasked)
and <512, 1 .. 4, 14> (row mask) are there and issue the i8 MFMA; no kernel of the unit spills or uses scratch; and the tile
loop of the unmasked kernels never drains the DMA ring: the steady units wait for a counted vmcnt behind an immediate, and the
only s_waitcnt vmcnt(0) between the first barrier and the last are the returning atomics of the full-list path (rare, exact)
and the last rung of the general units' wait ladder (the end of a workgroup's tile range, nothing left in flight)."""
import re

import pytest

from isa_common import audit_ring, device_asm, kernel_body, tile_loop

MFMA = "v_mfma_i32_16x16x64_i8"
UNITS = 2                # units (barriers) per tile of 1,024-byte rows
UNIT_STEPS = 8           # k-steps per unit: 2 NB MFMAs each


def check_no_drain(ins, nb):
    loop = tile_loop(ins)
    assert sum(ins[i].startswith(MFMA) for i in loop) >= 2 * UNITS * UNIT_STEPS * 2 * nb       # steady and general tiles
    # the steady units: a counted wait with an immediate in front of the barrier, then straight-line code to the unit's last MFMA
    steady = 0
    for b in loop:
        if not ins[b].startswith("s_barrier"):
            continue
        waits = [l for l in ins[max(0, b - 3):b] if re.match(r"s_waitcnt vmcnt\(\d+\)$", l)]
        if not waits or waits[-1] == "s_waitcnt vmcnt(0)":
            continue
        seg, mm = [], 0
        for l in ins[b + 1:]:
            if l.startswith("s_barrier"):
                break
            seg.append(l)
            mm += l.startswith(MFMA)
            if mm == UNIT_STEPS * 2 * nb:
                break
        if mm != UNIT_STEPS * 2 * nb or [l for l in seg if l.startswith(("s_cbranch", "s_branch"))]:
            continue
        steady += 1
        assert not [l for l in seg if l.startswith("s_waitcnt") and "vmcnt" in l], [l for l in seg if "vmcnt" in l]
    assert steady >= UNITS - 1, steady          # (the unit that opens a steady tile is entered through the loop's branch)
    # every drain of the vector-memory queue inside the loop: behind a returning atomic of the full-list path, or the ladder's end
    ladder = []
    for i in loop:
        if ins[i].startswith("s_waitcnt") and "vmcnt(0)" in ins[i]:
            if not any(p.startswith("global_atomic_add") for p in ins[max(0, i - 4):i]):
                ladder.append(i)
    for i in ladder:
        assert ins[i - 1].startswith("s_cbranch"), ins[i - 6:i + 2]          # a rung of the counted-wait ladder
    assert len(ladder) <= UNITS, [ins[i - 3:i + 1] for i in ladder]
    return steady, len(ladder)


@pytest.mark.timeout(900)
def test_wide_screen_unit_isa():
    asm, text, usage = device_asm("launch_screen8_wide")
    assert audit_ring.main(asm) == 0
    for variant in (8, 14):
        found = re.findall(r"^_ZN2ts18mfma16_topk_kernelILi512ELi(\d)ELi%dELb0ELb0ELb0ELb0EEEvNS_8MfmaArgsE:" % variant, text, re.M)
        assert sorted(found) == ["1", "2", "3", "4"], (variant, found)
    assert MFMA in text
    # the quantisers and both forms of the exact rescore live in this unit too
    for name in ("quantize_tiles_kernelILi1024E", "quantize_queries_kernelILi1024E", "screen_rescore_kernelILi1024ELb0E",
                 "screen_rescore_kernelILi1024ELb1E"):
        assert re.search(r"^_ZN2ts\d+%s\w*:" % name, text, re.M), name
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", usage)]
    assert scratch and max(scratch) == 0, scratch
    spills = [int(x) for x in re.findall(r"[SV]GPRs Spill: (\d+)", usage)]
    assert spills and max(spills) == 0, spills
    for nb in (1, 2, 3, 4):
        steady, ladder = check_no_drain(kernel_body(text, 512, nb, 8), nb)
        print("NB = %d: %d steady units without a vmcnt wait behind their barrier, %d ladder ends" % (nb, steady, ladder))
