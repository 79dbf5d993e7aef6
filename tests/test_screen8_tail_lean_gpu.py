"""The late-test screen's tile loop in two parts (mfma16_topk_kernel<384, 4, 15>, kernels_mfma16.h): the steady trips - two
tiles, one per accumulator set - run in a loop of their own, one hand-over follows, and the general units run the rest, a
left-over odd steady tile among them.  A tile is steady while five more units are still to be issued behind it, so a workgroup of
nt tiles has nt - 5 steady tiles and 2 * ((nt - 5) // 2) of them in the steady loop: 5 tiles -> none, 6 -> one left-over and no
trip, 7 -> one trip, 8 -> a trip and a left-over, 9 -> two trips.  The tile scalars live in two register sets by tile parity, each
loaded two tiles ahead; the steady loop reads them through a running pointer without the clamp to the workgroup's last tile.

On one index, the knob on, TS_MFMA_SCREEN_LATE=0 (the kernel that tests each tile at its own end) and TS_MFMA_SCREEN=0 (the bf16
pass) must give identical ids, identical score bits and the same counters.  Every comparison is exact."""
import numpy as np
import pytest

from test_screen8_append_gpu import plant
from test_screen8_late_gpu import N_PAD, N_WHOLE, assert_same, base, bounds, run

pytestmark = pytest.mark.gpu

N_EVEN = 17_280           # 540 tiles: 108 workgroups of 5, 90 of 6, 60 of 9
AHEAD = 5                 # units in flight behind a steady tile (the ring's slots - 1; one unit per tile at d = 768)


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


def steady_loop_tiles(nt):
    """Tiles of a workgroup of nt that its steady loop runs."""
    return max(0, nt - AHEAD) & ~1


def lengths(n, grid):
    b = bounds(n, grid)
    return sorted({b[w + 1] - b[w] for w in range(grid)})


def hand_over_tiles(n, grid, wgs, where):
    """Per workgroup of `wgs` with a steady trip: the last tile of its steady loop (where = -1) or the first tile behind the
    hand-over (where = 0)."""
    b = bounds(n, grid)
    out = []
    for w in wgs:
        ts_ = steady_loop_tiles(b[w + 1] - b[w])
        if ts_ > 0:
            out.append(b[w] + ts_ + where)
    return out


# grid -> tiles per workgroup.  540 tiles: 108 -> 5, 90 -> 6, 60 -> 9; 512 tiles: 102 -> 5 / 6, 85 -> 6 / 7, 60 -> 8 / 9;
# 626 tiles (the last one with padding rows): 125 -> 5 / 6, 104 -> 6 / 7, 70 -> 8 / 9
LENGTH_CASES = [(N_EVEN, 108, [5]), (N_EVEN, 90, [6]), (N_EVEN, 60, [9]), (N_WHOLE, 102, [5, 6]), (N_WHOLE, 85, [6, 7]),
                (N_WHOLE, 60, [8, 9]), (N_PAD, 125, [5, 6]), (N_PAD, 104, [6, 7]), (N_PAD, 70, [8, 9])]


@pytest.mark.parametrize("n,grid,want", LENGTH_CASES)
def test_workgroup_lengths_around_the_steady_loop(ts, n, grid, want):
    """No steady tile, a left-over steady tile without a trip, one trip, a trip and a left-over, two trips - with a dense tile
    (512 passing pairs) as the first and as the last tile of three workgroups."""
    assert lengths(n, grid) == want
    c, q = base(n)
    b = bounds(n, grid)
    tiles = sorted({t for w in (0, grid // 2, grid - 1) for t in (b[w], b[w + 1] - 1) if 32 * t + 32 <= n})
    out = run(ts, plant(c, q, tiles), q, grid, k=100)[0]
    assert_same(out, ("lengths", n, grid, want))
    ids = out["late"][1]
    assert (ids >= 0).all() and (ids < n).all()
    assert np.isin(ids[0] // 32, np.asarray(tiles)).sum() >= 4


@pytest.mark.parametrize("where", [-1, 0])
@pytest.mark.parametrize("n,grid", [(N_WHOLE, 85), (N_WHOLE, 60), (N_EVEN, 60), (N_PAD, 70)])
def test_dense_tile_across_the_hand_over(ts, n, grid, where):
    """512 passing pairs in the last tile of the steady loop (staged by the first general tile, from the other accumulator set,
    across the hand-over) and in the first tile behind it (tested among that tile's successor's MFMAs)."""
    c, q = base(n)
    tiles = hand_over_tiles(n, grid, [1, grid // 2, grid - 2, grid - 1], where)
    assert len(tiles) >= 2, tiles
    out = run(ts, plant(c, q, tiles), q, grid, k=100)[0]
    assert_same(out, ("hand-over", n, grid, where, tiles))
    assert np.isin(out["late"][1][0] // 32, np.asarray(tiles)).sum() >= 4      # query 0: rows 0 .. 3 of a planted tile


@pytest.mark.parametrize("n,grid", [(N_WHOLE, 60), (N_WHOLE, 102), (N_PAD, 70)])
def test_non_finite_in_the_last_two_tiles(ts, n, grid):
    """A NaN tile and an Inf tile as the last two tiles of the last workgroup: their scalars are the last two entries of the
    array, read two tiles ahead; every pair of both tiles is admitted."""
    c, q = base(n)
    c = c.copy()
    ntiles = (n + 31) // 32
    c[32 * (ntiles - 2) + 5, 17] = np.nan
    c[min(n - 1, 32 * (ntiles - 1) + 2), 3] = np.inf
    out = run(ts, c, q, grid)[0]
    assert_same(out, ("non-finite tail", n, grid))


def test_two_searches_one_handle(ts):
    c, q = base(N_PAD)
    tiles = hand_over_tiles(N_PAD, 70, [0, 35, 69], -1) + hand_over_tiles(N_PAD, 70, [1, 36, 68], 0)
    first, second = run(ts, plant(c, q, tiles), q, 70, k=100, searches=2)
    assert_same(first, "first search")
    assert_same(second, "second search")
    assert np.array_equal(first["late"][1], second["late"][1])
    assert np.array_equal(first["late"][0].view(np.uint32), second["late"][0].view(np.uint32))
