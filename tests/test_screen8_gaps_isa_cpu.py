"""The MFMA gaps of a steady tile of the late-test screen (launch_screen8_late.hip: mfma16_topk_kernel<384, 4, 15>), read off the
compiled gfx950 ISA.  A gap is what stands behind one MFMA and in front of the next.  One wave per SIMD hides fillers only where
they are few per gap, and a wait state in front of a filler hides nowhere, so between the barrier and the last MFMA of a steady
tile:
  * no s_nop - hipcc pads an asm statement that reads a register written by an earlier asm statement when only asm statements
    lie between the two; the pieces are placed so that no such pair exists (TS16_STEP / TS16_THR8 / TS16_LATE, kernels_mfma16.h),
    and m0 is written a gap ahead of its LDS-DMA piece;
  * a gap without a DMA piece holds at most three instructions, at most two of them vector instructions (VALU, ds_read);
  * a gap with a DMA piece holds the piece and at most two scalar instructions;
  * nothing between a write of m0 and its piece writes m0 again, and an MFMA stands between them."""
import pytest

from isa_common import device_asm, kernel_body

UNIT = "launch_screen8_late"
NB = 4
VARIANT = 15
MFMA = "v_mfma_i32_16x16x64_i8"
DMA = "global_load_lds_dwordx4"
MAX_PER_GAP = 3
MAX_VECTOR_PER_GAP = 2
MAX_SCALAR_BESIDE_DMA = 2
COUNTS = (("v_fma_f32", 3 * NB), ("v_floor_f32", NB), ("v_cvt_i32_f32", NB), ("v_max3_i32", 3 * NB), ("v_max_i32", NB),
          ("v_cmp_ge_i32", NB), ("ds_read_b128", 24), (DMA, 6))


def steady_tiles(ins):
    """(barrier, MFMA indices) of every tile of 96 MFMAs without a branch among them."""
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
            out.append((b, mm))
    return out


def gaps(ins, b, mm):
    """The head (barrier .. first MFMA) as gap -1, then gap g = the instructions between MFMA g and MFMA g + 1."""
    table = [(-1, [l for l in ins[b + 1:mm[0]] if not l.endswith(":")])]
    for g in range(len(mm) - 1):
        table.append((g, [l for l in ins[mm[g] + 1:mm[g + 1]] if not l.endswith(":")]))
    return table


def is_vector(l):
    return l.startswith(("v_", "ds_"))


def writes_m0(l):
    ops = l.split(None, 1)
    return len(ops) == 2 and ops[0].startswith("s_") and ops[1].split(",")[0].strip() == "m0"


def show(table):
    return "\n".join("  gap %3d (%d): %s" % (g, len(body), " | ".join(body)) for g, body in table)


@pytest.fixture(scope="module")
def asm():
    return device_asm(UNIT)


@pytest.fixture(scope="module")
def tables(asm):
    ins = kernel_body(asm.text, 384, NB, VARIANT)
    tiles = steady_tiles(ins)
    assert len(tiles) == 2, [b for b, _ in tiles]      # one steady trip: a tile per accumulator set
    out = [gaps(ins, b, mm) for b, mm in tiles]
    for t in out:
        print("steady tile:\n" + show(t))
    return out


@pytest.mark.timeout(900)
def test_no_wait_state_among_the_mfmas(tables):
    for table in tables:
        pads = [(g, l) for g, body in table for l in body if l.startswith("s_nop")]
        assert not pads, "%r\n%s" % (pads, show(table))


@pytest.mark.timeout(900)
def test_gap_budget(tables):
    for table in tables:
        for g, body in table:
            if any(l.startswith(DMA) for l in body):
                rest = [l for l in body if not l.startswith(DMA)]
                assert sum(l.startswith(DMA) for l in body) == 1, (g, body)
                assert not [l for l in rest if is_vector(l)] and len(rest) <= MAX_SCALAR_BESIDE_DMA, "gap %d: %r\n%s" % (g, body, show(table))
            else:
                assert len(body) <= MAX_PER_GAP and sum(is_vector(l) for l in body) <= MAX_VECTOR_PER_GAP, "gap %d: %r\n%s" % (g, body, show(table))


@pytest.mark.timeout(900)
def test_m0_is_written_a_gap_ahead_of_its_piece(tables):
    for table in tables:
        flat = [(g, l) for g, body in table for l in body]
        pieces = [i for i, (_, l) in enumerate(flat) if l.startswith(DMA)]
        assert len(pieces) == 6, show(table)
        prev = -1
        for i in pieces:
            w = [j for j in range(prev + 1, i) if writes_m0(flat[j][1])]
            # one write of m0 per piece, nothing else touches m0 before the piece, and an MFMA stands between the two
            assert len(w) == 1, "piece in gap %d: m0 written by %r\n%s" % (flat[i][0], [flat[j] for j in w], show(table))
            assert flat[w[0]][0] < flat[i][0], "piece in gap %d: m0 written in the same gap\n%s" % (flat[i][0], show(table))
            prev = i


@pytest.mark.timeout(900)
def test_instruction_counts(tables):
    for table in tables:
        body = [l for _, b in table for l in b]
        for op, want in COUNTS:
            assert sum(l.startswith(op) for l in body) == want, "%s\n%s" % (op, show(table))
