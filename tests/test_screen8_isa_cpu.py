"""The int8 screen's unit (launch_screen8.hip), checked in the compiled gfx950 ISA as tests/test_isa_audit_cpu.py checks the
bf16 units: no register of the fragment ring is read while its load is in flight, no operand is written right in front of its
MFMA (tools/audit_ring.py), the i8 MFMA is what the screen issues, and no kernel of the unit spills or uses scratch."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "theoremsearch_amd", "csrc")


@pytest.mark.timeout(900)
def test_screen_unit_isa():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-fvisibility=hidden",
                            "-save-temps=obj", "-c", "-o", os.path.join(tmp, "launch_screen8.o"), os.path.join(CSRC, "launch_screen8.hip"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=850, cwd=tmp)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = os.path.join(tmp, "launch_screen8-hip-amdgcn-amd-amdhsa-gfx950.s")
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        try:
            import audit_ring
            assert audit_ring.main(asm) == 0
        finally:
            sys.path.pop(0)
        text = open(asm).read()
        screen = re.findall(r"^_ZN2ts18mfma16_topk_kernelILi384ELi(\d)ELi8ELb0ELb0ELb0ELb0EEEvNS_8MfmaArgsE:", text, re.M)
        assert sorted(screen) == ["1", "2", "3", "4"], screen
        assert "v_mfma_i32_16x16x64_i8" in text
        scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
        assert scratch and max(scratch) == 0, scratch
