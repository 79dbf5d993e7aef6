"""The int8 screen's admitted-pair path in the compiled gfx950 ISA (launch_screen8.hip, NB = 4, the unmasked product kernel):
a wave that stages (row, query) pairs waits for nothing.  Its list is wave-private, the fill count is a scalar register that
lives through the tile loop, an entry's place is that count plus the lane's rank in the mask of passing lanes
(mfma8_append_block in kernels_screen8_tile.h).  So inside the tile loop - every instruction that can be reached from the first
barrier and can still reach a barrier, the append blocks included wherever hipcc has placed them - there is no LDS atomic, no
load of a kernel argument (the tile-scalar s_load_dwordx4 is the only scalar load) and no vector load from global memory.  The
row mask is read by the masked form of the kernel only (VARIANT 14): one scalar load of the tile's mask word, no vector load
either, so the DMA ring's vmcnt queue sees nothing of the path but the overflow case's atomics."""
import re

import pytest

from isa_common import device_asm, kernel_body, tile_loop

NB = 4


@pytest.mark.timeout(900)
def test_screen_append_path():
    text = device_asm("launch_screen8").text
    ins = kernel_body(text, 384, NB, 8)
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
    masked = kernel_body(text, 384, NB, 14)
    mloop = [masked[i] for i in tile_loop(masked)]
    msl = [l for l in mloop if l.startswith("s_load") and not l.startswith("s_load_dwordx4 ")]
    assert msl and all(l.startswith("s_load_dword ") for l in msl), msl
    assert not [l for l in mloop if re.match(r"(global|flat|buffer|scratch)_load", l) and not l.startswith("global_load_lds_")]
    assert [l for l in mloop if l.startswith("ds_write_b64")]
    assert not [l for l in masked if l.startswith(("ds_add", "ds_inc"))]
