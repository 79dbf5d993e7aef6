"""The late-test screen with its pieces spread over the k-steps (mfma16_topk_kernel<384, 4, 15>, TS16_THR8 / TS16_LATE in
kernels_mfma16.h): the four threshold pieces of a query block stand in four k-steps, the four blocks side by side in each of them,
and the block tests of the previous tile run two blocks abreast through two temporaries.  What can go wrong is a threshold or a
temporary of one block read by another, or a value read before its last piece ran - so the four query blocks of every wave
(block b = queries 64 b .. 64 b + 63) get thresholds that differ by orders of magnitude.  Three query sets:
  * "scaled": query q times 4^(q // 64), exact in bf16 - the score thresholds of the blocks are factors of 4 apart.  The screen's
    INTEGER thresholds are not: a query's int8 image and its threshold in units of that image do not change with its length, so
    this set alone lets a block's test run against another block's threshold unnoticed (tried: it does);
  * "spiked up" / "spiked down": one coordinate of every query of block b raised to 2^b (2^(3 - b)) times the query's largest
    one.  The image's scale grows with the spike and the integer threshold shrinks by about that factor (less the growth of the
    query's norm): neighbouring blocks a factor of two apart, blocks 0 and 3 most of an order of magnitude, while the image of
    the most spiked block still has +-16 to spend on the other coordinates and the screen stays selective (at 27 times the
    largest coordinate it admitted nearly everything and two such blocks could not be told apart).  With a larger block's
    threshold the rows just above a query's own threshold are lost and the ids differ; with a smaller one more pairs are
    admitted and the rescore drops them, which no answer shows - hence both orders.

Planted rows are scaled copies of one query (0.9 of the unit vector, less a little where one tile gets several: far above
anything a random row scores), one per tile and a few per query (two per tile sent a spiked query of the unscreened search to
the exact re-run), for every (block, tile parity), in steady tiles, in the last steady tile and in the tiles behind the
hand-over to the general units, of workgroups of 8 tiles (a steady trip and a left-over steady tile) and of 9 (two trips): 512 tiles on 60 workgroups, the smallest
row count the matrix path takes.  The knob on, TS_MFMA_SCREEN_LATE=0 and TS_MFMA_SCREEN=0 must give identical ids and score bits
and the same counters; the unscreened search must send no query to the exact re-run (asserted: the comparison would be between
two re-runs)."""
import functools

import numpy as np
import pytest

from test_screen8_late_gpu import D, N_WHOLE, NQ, assert_same, base, bounds, run

pytestmark = pytest.mark.gpu

GRID = 60                 # 512 tiles: workgroups of 8 and 9 tiles
AHEAD = 5                 # units in flight behind a steady tile (test_screen8_tail_lean_gpu.py)
K = 10
SCALES = (0.9, 0.85, 0.8)


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


QUERY_SETS = ("scaled", "spiked up", "spiked down")


@functools.lru_cache(maxsize=None)
def queries(kind):
    """The query set `kind` (module docstring), from the unit queries every case shares."""
    q = base(N_WHOLE)[1]
    block = np.arange(NQ) // 64
    if kind == "scaled":
        out = q * (4.0 ** block)[:, None].astype(np.float32)
    else:
        out = q.copy()
        power = block if kind == "spiked up" else 3 - block
        at = 3 * np.arange(NQ)                           # a coordinate of its own for every query's spike
        out[np.arange(NQ), at] = np.abs(q).max(axis=1) * (2.0 ** power)
    out = out.astype(np.float32)
    out.setflags(write=False)
    return out


def workgroup_of(length, nth=0):
    """The nth workgroup with `length` tiles: (first tile, tiles of its steady loop)."""
    b = bounds(N_WHOLE, GRID)
    w = [w for w in range(GRID) if b[w + 1] - b[w] == length][nth]
    return b[w], max(0, length - AHEAD) & ~1


class Planter:
    def __init__(self, kind):
        self.q = queries(kind)
        self.unit = self.q / np.linalg.norm(self.q, axis=1, keepdims=True)
        self.c = base(N_WHOLE)[0].copy()
        self.rows = {}                          # query -> planted rows
        self.used = set()

    def plant(self, tile, query, count, slot):
        """`count` scaled copies of `query` in `tile`, at rows that differ with `slot` (all four row quarters, both row blocks)."""
        for i in range(count):
            row = 32 * tile + (11 * slot + 13 * i + 5 * (query // 64)) % 32
            while row in self.used:
                row = 32 * tile + (row + 1) % 32
            self.used.add(row)
            have = len(self.rows.setdefault(query, []))
            assert have < K - 2, (query, have)  # the k-th best of every query stays a random row
            self.c[row] = (SCALES[i % len(SCALES)] - 0.01 * (have // len(SCALES))) * self.unit[query]
            self.rows[query].append(row)


def check(out, planter, what):
    st = {name: o[2] for name, o in out.items()}
    # precondition: the unscreened search answers every query from its candidates
    assert st["bf16"]["fallback_queries"] == 0, (what, st["bf16"])
    assert_same(out, what)                      # ids, score bits, candidates, fallback_queries
    assert st["late"]["screened"] == 1 and st["tail"]["screened"] == 1 and st["bf16"]["screened"] == 0, (what, st)
    ids = out["late"][1]
    for query, rows in planter.rows.items():
        assert np.isin(rows, ids[query]).all(), (what, query, rows, ids[query].tolist())
        assert np.array_equal(np.sort(ids[query][:len(rows)]), np.sort(rows)), (what, query)     # nothing random ranks above them


@pytest.mark.parametrize("kind", QUERY_SETS)
@pytest.mark.parametrize("length", [8, 9])
def test_one_block_per_tile(ts, length, kind):
    """For every block and tile parity its own tiles: a steady tile, the last steady tile or the one in front of it, and a tile
    behind the hand-over - each in a workgroup of its own parity's choosing, so no other block passes in the same tile."""
    p = Planter(kind)
    for b in range(4):
        for par in range(2):
            t0, steady = workgroup_of(length, 2 * b + par)
            assert steady >= 2
            query = 64 * b + 16 * ((b + par) % 4) + (5 * b + 3 * par) % 16      # every wave, varied lanes
            p.plant(t0 + par, query, 1, slot=2 * b + par)                        # a steady tile of parity par
            p.plant(t0 + steady - 2 + par, query, 1, slot=2 * b + par + 3)       # ... the last steady trip
            p.plant(t0 + steady + par, query, 1, slot=2 * b + par + 5)           # ... behind the hand-over
    out = run(ts, p.c, p.q, GRID, k=K)[0]
    check(out, p, ("one block per tile", length, kind))


@pytest.mark.parametrize("kind", QUERY_SETS)
@pytest.mark.parametrize("length", [8, 9])
def test_four_blocks_abreast(ts, length, kind):
    """All four blocks of every wave pass in the same tile, in consecutive tiles from the first steady tile to the second tile
    behind the hand-over: both temporaries and all four masks in use in every tile, for both accumulator sets."""
    p = Planter(kind)
    t0, steady = workgroup_of(length, 1)
    for t in range(steady + 2):
        for b in range(4):
            for wave in range(4):
                if (wave + t) % 2 == 0:
                    continue                        # two waves per tile, the other two in the next
                p.plant(t0 + t, 64 * b + 16 * wave + (3 * t + b) % 16, 1, slot=t + 4 * b + wave)
    out = run(ts, p.c, p.q, GRID, k=K)[0]
    check(out, p, ("four blocks abreast", length, kind))


@pytest.mark.parametrize("kind", QUERY_SETS)
def test_two_searches_one_handle(ts, kind):
    p = Planter(kind)
    for length in (8, 9):
        t0, steady = workgroup_of(length, 3)
        for t in range(steady + 1):
            for b in range(4):
                p.plant(t0 + t, 64 * b + 16 * ((b + t) % 4) + (7 * t + b) % 16, 1, slot=t + 3 * b)
    first, second = run(ts, p.c, p.q, GRID, k=K, searches=2)
    check(first, p, ("first search", kind))
    check(second, p, ("second search", kind))
    for name in first:
        assert np.array_equal(first[name][1], second[name][1]), name
        assert np.array_equal(first[name][0].view(np.uint32), second[name][0].view(np.uint32)), name
