"""The late-test screen in the compiled gfx950 ISA (launch_screen8_late.hip: mfma16_topk_kernel<384, 4, 15>): the block tests
of tile t - 1 are two-instruction pieces behind MFMAs of tile t (TS16_LATE in kernels_mfma16.h, late_test_a / b / c in
kernels_screen8_tile.h), so between a tile's last i8 MFMA and the load of the scalars two tiles ahead there is the ring's drain,
the OR of four lane masks and scalar bookkeeping - no test instruction, no LDS atomic.  Reads hand-placed code only."""
import re

import pytest

from isa_common import audit_ring, device_asm, kernel_body

UNIT = "launch_screen8_late"
NB = 4
VARIANT = 15
MFMA = "v_mfma_i32_16x16x64_i8"
TEST_OPS = ("v_max3_i32", "v_max_i32", "v_cmp_ge_i32")
LDS_ATOMICS = ("ds_add", "ds_sub", "ds_inc", "ds_dec", "ds_min", "ds_max", "ds_and", "ds_or", "ds_xor", "ds_cmpst", "ds_wrxchg")


def _tail_path(ins, start):
    """The straight path from `start` to the next scalar load: conditional branches fall through (the hand-over to the general
    units, once per launch, is on it; the pair path is not), unconditional ones are followed.  None: a barrier comes first."""
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


def _tiles(ins):
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


@pytest.fixture(scope="module")
def asm():
    return device_asm(UNIT)


@pytest.mark.timeout(900)
def test_ring_audit_and_registers(asm):
    assert audit_ring.main(asm.path) == 0
    blocks = re.split(r"Function Name: ", asm.usage)
    mine = [b for b in blocks if b.startswith("_ZN2ts18mfma16_topk_kernelILi384ELi%dELi%dE" % (NB, VARIANT))]
    assert len(mine) == 1, [b[:80] for b in blocks]
    for what, want in (("ScratchSize [bytes/lane]", 0), ("VGPRs Spill", 0), ("SGPRs Spill", 0), ("Occupancy [waves/SIMD]", 1)):
        m = re.search(re.escape(what) + r": (\d+)", mine[0])
        assert m and int(m.group(1)) == want, (what, m and m.group(1))


@pytest.mark.timeout(900)
def test_late_tile_shape(asm):
    ins = kernel_body(asm.text, 384, NB, VARIANT)
    assert any(l.startswith(MFMA) for l in ins)
    tiles = _tiles(ins)
    # a trip of the loop is two tiles, one per accumulator set (steady and general form of each)
    assert len(tiles) >= 2 and len(tiles) % 2 == 0, len(tiles)
    steady_tiles = 0
    for b, last, tail, load in tiles:
        body = ins[b + 1:last]
        print("tail:\n  " + "\n  ".join(tail))
        # the previous tile's block tests stand among this tile's MFMAs: 5 NB instructions
        assert sum(l.startswith("v_max3_i32") for l in body) == 3 * NB
        assert sum(l.startswith("v_max_i32") for l in body) == NB
        assert sum(l.startswith("v_cmp_ge_i32") for l in body) == NB
        # ... in a steady tile (no branch among its MFMAs: the general units branch around their DMA pieces, and hipcc puts copies
        # where those paths meet) each piece of at most two instructions in the gap behind an MFMA (scalar instructions of
        # hipcc's may stand there too: they do not take the vector issue)
        steady = not any(l.startswith("s_cbranch") for l in body)
        steady_tiles += steady
        for i, l in enumerate(body):
            if steady and l.startswith(TEST_OPS):
                j, mine = i - 1, 1
                while body[j].startswith(TEST_OPS) or body[j].startswith("s_"):
                    mine += body[j].startswith(TEST_OPS)
                    j -= 1
                assert body[j].startswith(MFMA) and mine <= 2, body[max(0, i - 4):i + 1]
        # ... and so do this tile's thresholds: 3 FMAs, the clamp, floor and convert per query block
        assert sum(l.startswith("v_cvt_i32_f32") for l in body) == NB
        assert sum(l.startswith("v_floor_f32") for l in body) == NB
        assert sum(l.startswith("v_fma_f32") for l in body) == 3 * NB
        # behind the last MFMA: no test instruction, no LDS atomic
        assert not [l for l in tail if l.startswith(("v_max3_i32", "v_cmp_ge_i32"))], tail
        assert not [l for l in tail if l.startswith(LDS_ATOMICS)], tail
        # lgkmcnt(0): none among the MFMAs; the tail begins with the ring's drain
        assert not [l for l in body if "lgkmcnt(0)" in l]
        # (general units: behind the bookkeeping of the unit they issued)
        assert "lgkmcnt(0)" in tail[0] if steady else any("lgkmcnt(0)" in l for l in tail), tail[:3]
        # the load of the scalars two tiles ahead stays in flight into the next tile: no wait behind it before the loop branch
        for l in ins[load + 1:]:
            if l.startswith(("s_cbranch", "s_branch")):
                break
            assert "lgkmcnt" not in l, ins[load:load + 12]
    assert steady_tiles == 2, steady_tiles         # the steady trip: one tile per accumulator set
