"""The late-test form of the int8 screen (TS_MFMA_SCREEN_LATE; mfma16_topk_kernel<384, 4, 15>, launch_screen8_late.hip): tile
t - 1 is tested among the MFMAs of tile t and its admitted pairs are staged one tile late, the last tile's behind the loop.  On
one index, the knob on, the knob off (the kernel that tests each tile at its own end) and TS_MFMA_SCREEN=0 (the bf16 pass) must
give identical ids, identical score bits and the same counters.

Small corpora (512 and 626 tiles) and TS_MFMA_GRID put every workgroup length on the path: 0, 1, 2, 3 tiles and an odd and an
even larger number (the loop runs two tiles per trip, one per accumulator set).  Dense tiles (the recipe of
test_screen8_append_gpu.py: 512 passing pairs in a tile) stand in a workgroup's first, second-to-last and last tile - staged by
the next tile's tail from the other accumulator set, and by the block behind the loop."""
import functools

import numpy as np
import pytest

from synthetic import bf16_bits
from test_screen8_append_gpu import plant, planted_rows, unit

pytestmark = pytest.mark.gpu

D = 768
NQ = 256
N_WHOLE = 16_384          # 512 whole tiles
N_PAD = 20_011            # 625 whole tiles + one of 11 rows and 21 padding rows
FORMS = (("late", {"TS_MFMA_SCREEN_LATE": 1}), ("tail", {"TS_MFMA_SCREEN_LATE": 0}), ("bf16", {"TS_MFMA_SCREEN": 0}))


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


@functools.lru_cache(maxsize=4)
def base(n, seed=31):
    rng = np.random.default_rng(seed)
    c = unit(rng.standard_normal((n, D), dtype=np.float32))
    q = unit(rng.standard_normal((NQ, D), dtype=np.float32))
    c.setflags(write=False)
    q.setflags(write=False)
    return c, q


def bounds(n, grid):
    """First tile of every workgroup (equal shares: what the kernel computes without a feedback table) and the end."""
    ntiles = (n + 31) // 32
    return [ntiles * w // grid for w in range(grid + 1)]


def edge_tiles(n, grid, wgs):
    """First, second-to-last and last tile of the workgroups `wgs` (those they have)."""
    b = bounds(n, grid)
    out = set()
    for w in wgs:
        t0, t1 = b[w], b[w + 1]
        out.update(t for t in (t0, t1 - 2, t1 - 1) if t0 <= t < t1)
    return sorted(out)


def search_forms(ix, q, k, mask=None, forms=FORMS):
    out = {}
    for name, opts in forms:
        for o, v in opts.items():
            ix.set_option(o, v)
        s, i, st = ix.search(q, k, algo="mfma", return_stats=True, mask=mask)
        out[name] = (np.asarray(s).copy(), np.asarray(i).copy(), st)
        for o in opts:
            ix.set_option(o, None)
    return out


def assert_same(out, what):
    s0, i0, st0 = out["tail"]
    for name, (s, i, st) in out.items():
        print(what, name, "fallback_queries", st["fallback_queries"], "candidates", st["candidates"], "screened", st["screened"])
    for name, (s, i, st) in out.items():
        bad = np.argwhere(i != i0)
        assert bad.size == 0, (what, name, bad[:5].tolist())
        assert np.array_equal(s.view(np.uint32), s0.view(np.uint32)), (what, name)
        # the rescore keeps the pairs whose exact score reaches the threshold - the bf16 pass's candidates, whichever screen ran
        assert st["candidates"] == st0["candidates"], (what, name)
        assert st["fallback_queries"] == st0["fallback_queries"], (what, name)


def run(ts, c, q, grid, k=10, mask=None, searches=1, forms=FORMS):
    ix = ts.TheoremIndex(c.shape[0], D, dtype="bf16", metric="ip")
    try:
        ix.upload(bf16_bits(c), 0)
        if grid is not None:
            ix.set_option("TS_MFMA_GRID", grid)
        qb = bf16_bits(q)
        return [search_forms(ix, qb, k, mask=mask, forms=forms) for _ in range(searches)]
    finally:
        ix.close()


# grid -> tiles per workgroup: 512 tiles: 1024 -> 0 / 1, 512 -> 1, 256 -> 2, 171 -> 2 / 3, 73 -> 7 / 8, 64 -> 8;
# 626 tiles: 209 -> 2 / 3, 64 -> 9 / 10, 7 -> 89 / 90
@pytest.mark.parametrize("n,grid", [(N_WHOLE, 1024), (N_WHOLE, 512), (N_WHOLE, 256), (N_WHOLE, 171), (N_WHOLE, 73), (N_WHOLE, 64),
                                    (N_PAD, 209), (N_PAD, 64), (N_PAD, 7)])
@pytest.mark.parametrize("nq", [256, 193])
def test_dense_tiles_at_workgroup_edges(ts, n, grid, nq):
    """Dense tiles in the first, second-to-last and last tile of three workgroups (the corpus's last one among them: with
    N_PAD its last tile holds padding rows, so the checked form of the pair path is reached from inside the loop - the tile
    before - and from behind it)."""
    c, q = base(n)
    tiles = edge_tiles(n, grid, [1, grid // 2, grid - 1])
    b = bounds(n, grid)
    lens = sorted({b[w + 1] - b[w] for w in range(grid)})
    c = plant(c, q, [t for t in tiles if 32 * t + 32 <= n])
    if n % 32:
        c[n - n % 32:] = planted_rows(q, n % 32, 99)
    out = run(ts, c, q[:nq], grid, k=100)[0]                   # k = 100: room for all planted rows of a query (at most 40)
    assert_same(out, ("edges", n, grid, nq, "tiles per workgroup", lens))
    ids = out["late"][1]
    assert (ids >= 0).all() and (ids < n).all()
    assert np.isin(ids[0] // 32, np.asarray(tiles + [n // 32])).sum() >= 4      # query 0: rows 0 .. 3 of a planted tile
    if n % 32:
        assert np.isin(n - n % 32 + np.arange(4), ids[0]).all()                # ... and of the corpus's last tile


def test_wave_list_overflows(ts):
    """Six dense tiles inside one workgroup of eight: 768 pairs per wave against a list of 384 - the slow exact way, taken from
    the late path; the last two of them are the workgroup's last tiles."""
    c, q = base(N_WHOLE)
    tiles = list(range(8 * 5 + 2, 8 * 5 + 8))
    out = run(ts, plant(c, q, tiles), q, 64, k=100)[0]
    assert_same(out, "wave list overflow")
    assert np.isin(out["late"][1][0] // 32, np.asarray(tiles)).sum() >= 20


def test_query_list_overflows(ts):
    """More rows pass one query's threshold than its candidate list holds (8,192): the query is answered by the exact re-run."""
    c, q = base(N_WHOLE)
    rng = np.random.default_rng(3)
    c = c.copy()
    # copies of query 5 + noise in the tiles the threshold sample (every fourth tile) does not see
    rows = np.flatnonzero((np.arange(N_WHOLE) // 32) % 4 != 0)[:9_600]
    c[rows] = unit(q[5] + 0.02 * rng.standard_normal((rows.size, D), dtype=np.float32))
    out = run(ts, c, q, 64)[0]
    assert_same(out, "query list overflow")
    assert out["late"][2]["fallback_queries"] >= 1
    assert np.isin(out["late"][1][5], rows).all()


@pytest.mark.parametrize("grid", [64, 171])
def test_nan_tile_first_and_last(ts, grid):
    """A non-finite value makes its tile's threshold INT_MIN: every pair of the tile is admitted (1,024 per wave, past the
    list) - as a workgroup's first tile and as its last."""
    c, q = base(N_WHOLE)
    b = bounds(N_WHOLE, grid)
    c = c.copy()
    w = grid // 3
    c[32 * b[w] + 5, 17] = np.nan
    c[32 * (b[w + 2] - 1) + 30, 700] = np.inf
    c[32 * (b[grid] - 1) + 2, 3] = -np.inf
    out = run(ts, c, q, grid)[0]
    assert_same(out, ("nan tile", grid))


def test_two_searches_one_handle(ts):
    c, q = base(N_PAD)
    c = plant(c, q, edge_tiles(N_PAD, 64, [0, 63])[:-1])
    first, second = run(ts, c, q, 64, searches=2)
    assert_same(first, "first search")
    assert_same(second, "second search")
    assert np.array_equal(first["late"][1], second["late"][1])


def test_masked_and_small_batches_keep_their_kernels(ts):
    """A masked search and a batch of 64 queries have no late form: with the knob on they run the kernels they ran before."""
    c, q = base(N_PAD)
    c = plant(c, q, edge_tiles(N_PAD, 64, [3, 63])[:-1])
    mask = np.random.default_rng(9).random(N_PAD) < 0.5
    out = run(ts, c, q, 64, mask=mask)[0]
    assert_same(out, "masked")
    assert mask[out["late"][1].ravel()].all()
    out = run(ts, c, q[:64], 64)[0]
    assert_same(out, "64 queries")
