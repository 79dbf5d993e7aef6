"""The int8 screen's admitted-pair path in the compiled gfx950 ISA (launch_screen8.hip, NB = 4, the unmasked product kernel):
a wave that stages (row, query) pairs waits for nothing.  Its list is wave-private, the fill count is a scalar register that
lives through the tile loop, an entry's place is that count plus the lane's rank in the mask of passing lanes
(mfma8_append_block in kernels_mfma16.h).  So inside the tile loop - every instruction that can be reached from the first
barrier and can still reach a barrier, the append blocks included wherever hipcc has placed them - there is no LDS atomic, no
load of a kernel argument (the tile-scalar s_load_dwordx4 is the only scalar load) and no vector load from global memory.  The
row mask is read by the masked form of the kernel only (VARIANT 14): one scalar load of the tile's mask word, no vector load
either, so the DMA ring's vmcnt queue sees nothing of the path but the overflow case's atomics."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "theoremsearch_amd", "csrc")
NB = 4


def _kernel(text, nb, variant):
    m = re.search(r"^_ZN2ts18mfma16_topk_kernelILi384ELi%dELi%dELb0ELb0ELb0ELb0EEEvNS_8MfmaArgsE:[^\n]*\n(.*?)\n\.Lfunc_end" % (nb, variant),
                  text, re.S | re.M)
    assert m, "no NB = %d screen kernel of variant %d" % (nb, variant)
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


def _compile(tmp):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "-fvisibility=hidden",
                        "-save-temps=obj", "-c", "-o", os.path.join(tmp, "launch_screen8.o"), os.path.join(CSRC, "launch_screen8.hip")],
                       capture_output=True, text=True, timeout=850, cwd=tmp)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(tmp, "launch_screen8-hip-amdgcn-amd-amdhsa-gfx950.s")).read()


@pytest.mark.timeout(900)
def test_screen_append_path():
    with tempfile.TemporaryDirectory() as tmp:
        text = _compile(tmp)
    ins = _kernel(text, NB, 8)
    loop = [ins[i] for i in tile_loop(ins)]
    ops = [l.split()[0] for l in loop]
    # the loop was found: the tiles' MFMAs and the append blocks (a ranked ds_write_b64 per accumulator value) are in it
    assert sum(o == "v_mfma_i32_16x16x64_i8" for o in ops) >= 24 * NB
    writes = [l for l in loop if l.startswith("ds_write_b64")]
    assert len(writes) >= 8 * NB, writes
    assert sum(o.startswith("v_mbcnt_hi") for o in ops) >= 8 * NB and sum(o.startswith("s_bcnt1_i32_b64") for o in ops) >= 8 * NB
    print("append blocks: %d ds_write_b64, %d v_mbcnt_hi, %d s_bcnt1" % (len(writes), sum(o.startswith("v_mbcnt_hi") for o in ops),
                                                                         sum(o.startswith("s_bcnt1_i32_b64") for o in ops)))
    # no LDS atomic anywhere in the kernel: the fill count is a scalar register
    assert not [l for l in ins if l.startswith(("ds_add", "ds_inc", "ds_cmpst", "ds_wrxchg"))]
    # scalar loads of the loop: the tile scalars, one 16-byte load each - no kernel argument is re-read on the append path
    sl = [l for l in loop if l.startswith(("s_load", "s_buffer_load"))]
    assert sl and all(l.startswith("s_load_dwordx4 ") for l in sl), sl
    # vector loads from global memory: only the LDS-DMA stream (the unmasked kernel never touches the row mask)
    gl = [l for l in loop if re.match(r"(global|flat|buffer|scratch)_load", l) and not l.startswith("global_load_lds_")]
    assert not gl, gl
    # ... and the masked form of the kernel is the one that reads it: a scalar load of one mask word per tile with a passing
    # lane, in front of the same ranked write
    masked = _kernel(text, NB, 14)
    mloop = [masked[i] for i in tile_loop(masked)]
    msl = [l for l in mloop if l.startswith("s_load") and not l.startswith("s_load_dwordx4 ")]
    assert msl and all(l.startswith("s_load_dword ") for l in msl), msl
    assert not [l for l in mloop if re.match(r"(global|flat|buffer|scratch)_load", l) and not l.startswith("global_load_lds_")]
    assert [l for l in mloop if l.startswith("ds_write_b64")]
    assert not [l for l in masked if l.startswith(("ds_add", "ds_inc"))]
