"""The int8 screen's unit (launch_screen8.hip), checked in the compiled gfx950 ISA as tests/test_isa_audit_cpu.py checks the
bf16 units: no register of the fragment ring is read while its load is in flight, no operand is written right in front of its
MFMA (tools/audit_ring.py), the i8 MFMA is what the screen issues, and no kernel of the unit spills or uses scratch."""
import re

import pytest

from isa_common import audit_ring, device_asm


@pytest.mark.timeout(900)
def test_screen_unit_isa():
    asm, text, usage = device_asm("launch_screen8")
    assert audit_ring.main(asm) == 0
    screen = re.findall(r"^_ZN2ts18mfma16_topk_kernelILi384ELi(\d)ELi8ELb0ELb0ELb0ELb0EEEvNS_8MfmaArgsE:", text, re.M)
    assert sorted(screen) == ["1", "2", "3", "4"], screen
    assert "v_mfma_i32_16x16x64_i8" in text
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", usage)]
    assert scratch and max(scratch) == 0, scratch
