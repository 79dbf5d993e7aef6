"""The int8 screen's tile tail in the compiled gfx950 ISA (launch_screen8.hip, NB = 4): the tile thresholds are computed among
the tile's MFMAs (screen_thr_piece in kernels_screen8_tile.h, TS16_THR8 in kernels_mfma16.h), so between the last i8 MFMA of a steady tile and the load of
the scalars two tiles ahead there is only the ring's drain, the block test and a little scalar bookkeeping."""
import re

import pytest

from isa_common import device_asm, kernel_body

NB = 4
MFMA = "v_mfma_i32_16x16x64_i8"
# VALU of the tail beyond the 5 NB block-test instructions: the hand-over to the general units (a v_lshl_add_u64 and two
# v_mov_b32, on the path once per launch) and room for one copy that hipcc may place there
BOOKKEEPING = 4


def _tail_path(ins, start):
    """The straight path from `start` to the next scalar load: conditional branches fall through (the hand-over block, once per
    launch, is on it; the append path, taken when a lane passes, is not), unconditional ones are followed.  None: a barrier
    comes first."""
    labels = {l[:-1]: i for i, l in enumerate(ins) if l.endswith(":")}
    path, i = [], start
    while i < len(ins) and len(path) < 400:
        l = ins[i]
        if l.startswith("s_barrier"):
            return None
        if l.startswith("s_load_dword"):
            return path, i
        if l.startswith("s_branch "):
            i = labels[l.split()[1]] + 1
            continue
        if not l.endswith(":"):
            path.append(l)
        i += 1
    return None


def _steady_tiles(ins):
    """(barrier, last MFMA, tail path, scalar load) of every tile of 96 MFMAs whose tail reaches a scalar load before any barrier."""
    tiles = []
    for b, line in enumerate(ins):
        if not line.startswith("s_barrier"):
            continue
        mm = []
        for i in range(b + 1, len(ins)):
            if ins[i].startswith("s_barrier"):
                break
            if ins[i].startswith(MFMA):
                mm.append(i)
                if len(mm) == 24 * NB:
                    break
        if len(mm) != 24 * NB:
            continue
        t = _tail_path(ins, mm[-1] + 1)
        if t:
            tiles.append((b, mm[-1]) + t)
    return tiles


@pytest.mark.timeout(900)
def test_screen_tile_tail():
    ins = kernel_body(device_asm("launch_screen8").text, 384, NB, 8)
    tiles = _steady_tiles(ins)
    assert tiles, "no steady tile of %d MFMAs followed by the tile-scalar load" % (24 * NB)
    for b, last, tail, load in tiles:
        body = ins[b + 1:last]
        print("tail:\n  " + "\n  ".join(tail))
        # the thresholds are computed among the MFMAs: 3 FMAs, the clamp, floor and convert per query block
        assert sum(l.startswith("v_cvt_i32_f32") for l in body) == NB, body
        assert sum(l.startswith("v_floor_f32") for l in body) == NB
        assert sum(l.startswith("v_fma_f32") for l in body) == 3 * NB
        # ... and none of it is left behind the last MFMA
        bad = [l for l in tail if re.match(r"v_(floor|med3|fma|fmac|mul|sub|add)_f32|v_cvt_\w*i32_f32", l)]
        assert not bad, bad
        valu = [l for l in tail if l.startswith("v_")]
        assert len(valu) <= 5 * NB + BOOKKEEPING, valu
        assert sum(l.startswith(("v_max3_i32", "v_max_i32", "v_cmp_ge_i32")) for l in tail) == 5 * NB
        # lgkmcnt(0): none among the MFMAs; in the tail only the drain (and hipcc's wait for the scalars, which landed a tile
        # earlier), both ahead of the block test
        assert not [l for l in body if "lgkmcnt(0)" in l]
        first_test = next(i for i, l in enumerate(tail) if l.startswith("v_max3_i32"))
        assert not [l for l in tail[first_test:] if "lgkmcnt" in l], tail[first_test:]
        assert "lgkmcnt(0)" in tail[0], tail[:3]
        # the load of the scalars two tiles ahead stays in flight into the next tile: no wait behind it before the loop branch
        for l in ins[load + 1:]:
            if l.startswith(("s_cbranch", "s_branch")):
                break
            assert "lgkmcnt" not in l, ins[load:load + 12]
