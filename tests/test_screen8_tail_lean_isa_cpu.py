"""What stands between a steady tile's last MFMA and the next tile's barrier in the late-test screen (launch_screen8_late.hip:
mfma16_topk_kernel<384, 4, 15>), read off the compiled gfx950 ISA.  One wave per SIMD has nothing to overlap that stretch with,
so it holds what must stand there and nothing else: the ring's drain, the test of the masks' union with the rare-path branch,
the load of the scalars two tiles ahead, the loop's branch and the next tile's vmcnt wait.  The union of the four lane masks, the
ring offsets, the stream's tile base and the scalars' address are made among the MFMAs (TS16_LATE, kernels_mfma16.h); the steady
tiles run in a loop of their own, so no copy stands where two forms of the tile would meet."""
import pytest

from isa_common import device_asm, kernel_body

UNIT = "launch_screen8_late"
NB = 4
VARIANT = 15
MFMA = "v_mfma_i32_16x16x64_i8"
MAX_INSTRUCTIONS = 16
MAX_BRANCHES = 3
COPIES = ("s_mov_b32", "s_mov_b64", "v_mov_b64")


def steady_tiles(ins):
    """(barrier, last MFMA) of every tile of 96 MFMAs without a branch among them (the general units branch around their DMA
    pieces)."""
    out = []
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
        if len(mm) == 24 * NB and not any(l.startswith("s_cbranch") for l in ins[b + 1:mm[-1]]):
            out.append((b, mm[-1]))
    return out


def path_to_barrier(ins, start):
    """The instructions from `start` to the next s_barrier (not included), and that barrier's index: conditional branches fall
    through, except a backward one (the loop's back edge), which is taken; unconditional ones are followed."""
    labels = {l[:-1]: i for i, l in enumerate(ins) if l.endswith(":")}
    path, i = [], start
    while len(path) < 200:
        l = ins[i]
        if l.startswith("s_barrier"):
            return path, i
        if l.endswith(":"):
            i += 1
            continue
        path.append(l)
        assert not l.startswith("s_endpgm"), path
        if l.startswith("s_branch "):
            i = labels[l.split()[1]]
        elif l.startswith("s_cbranch") and labels[l.split()[1]] < i:
            i = labels[l.split()[1]]
        else:
            i += 1
    raise AssertionError("no barrier behind the tile: " + repr(path[:40]))


@pytest.fixture(scope="module")
def asm():
    return device_asm(UNIT)


@pytest.mark.timeout(900)
def test_steady_tail_is_lean(asm):
    ins = kernel_body(asm.text, 384, NB, VARIANT)
    tiles = steady_tiles(ins)
    assert len(tiles) == 2, tiles                  # one steady trip: a tile per accumulator set
    barriers = {b for b, _ in tiles}
    reached = set()
    for b, last in tiles:
        path, nxt = path_to_barrier(ins, last + 1)
        reached.add(nxt)
        branches = [l for l in path if l.startswith(("s_cbranch", "s_branch"))]
        print("tile at %d: %d instructions, %d branch instructions\n  %s" % (b, len(path), len(branches), "\n  ".join(path)))
        assert len(path) <= MAX_INSTRUCTIONS, path
        assert len(branches) <= MAX_BRANCHES, branches
        assert not [l for l in path if l.startswith(COPIES)], path
        assert not [l for l in path if l.startswith("s_or_b64")], path          # the masks' union stands among the MFMAs
        assert path[0].startswith("s_waitcnt") and "lgkmcnt(0)" in path[0], path[:2]       # the ring's drain comes first
        loads = [i for i, l in enumerate(path) if l.startswith("s_load_dword")]
        assert len(loads) == 1, path                # the scalars two tiles ahead ...
        assert not [l for l in path[loads[0] + 1:] if "lgkmcnt" in l], path                # ... still in flight at the barrier
        assert sum("vmcnt" in l for l in path) == 1 and "vmcnt" in path[-1], path          # the stream's counted wait, then the barrier
    # the two tiles follow each other: the even one runs into the odd one, the odd one's back edge into the even one
    assert reached == barriers, (reached, barriers)


@pytest.mark.timeout(900)
def test_union_of_the_masks_among_the_mfmas(asm):
    ins = kernel_body(asm.text, 384, NB, VARIANT)
    for b, last in steady_tiles(ins):
        body = ins[b + 1:last]
        ors = [i for i, l in enumerate(body) if l.startswith("s_or_b64") and "exec" not in l]
        cmps = [i for i, l in enumerate(body) if l.startswith("v_cmp_ge_i32")]
        assert len(ors) == NB - 1 and len(cmps) == NB, (ors, cmps)
        assert ors[0] > cmps[-1], (ors, cmps)       # behind the last block test ...
        for i in ors:                                # ... each one in a gap behind an MFMA (scalar neighbours allowed)
            j = i - 1
            while body[j].startswith("s_"):
                j -= 1
            assert body[j].startswith(MFMA), body[max(0, i - 4):i + 1]
