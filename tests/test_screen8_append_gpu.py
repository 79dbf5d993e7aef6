"""The int8 screen's admitted-pair path (mfma8_append_block in kernels_screen8_tile.h: a wave-private LDS list filled at a
wave-uniform count + the lane's rank among the passing lanes, an exact slow path when the list is full, a checked form for the
corpus's last tile and for masked searches) under load it never sees on Gaussian rows: tiles in which hundreds of (row, query)
pairs pass at once.  Every case compares TS_MFMA_SCREEN=1 with TS_MFMA_SCREEN=0 on one index: identical ids, identical score bits.

A planted tile: its rows come in groups of four (rows 4 a .. 4 a + 3, a = 0 .. 7) built from the sum of 16 queries, one of every
block of 16 queries - query 16 blk + (2 a + blk) % 16 of block blk - plus a little noise that keeps the four apart.  A row
scores ~0.3 against its 16 queries (the threshold of the pass sits near 0.16), so in that tile
  * a lane (query, row quarter) holds four passing values, all in one row block;
  * every query block has passing lanes in all four row quarters (several lanes of one compare mask), and
  * every wave has passing lanes in all four of its query blocks:
512 pairs per tile, 128 per wave."""
import functools

import numpy as np
import pytest

from synthetic import bf16_bits

pytestmark = pytest.mark.gpu

D = 768
NQ = 256
STAGE_CAP = 384       # entries of a wave's list (kScreenStageCap)


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


def unit(x):
    x = x.astype(np.float32)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


@functools.lru_cache(maxsize=2)
def base(n, seed=21):
    rng = np.random.default_rng(seed)
    return unit(rng.standard_normal((n, D), dtype=np.float32)), unit(rng.standard_normal((NQ, D), dtype=np.float32))


def planted_rows(q, rows, seed):
    """`rows` planted rows, as they would fill tiles from a tile's first row on (row i of the result = row i % 32 of its tile)."""
    rng = np.random.default_rng(seed)
    out = np.empty((rows, D), dtype=np.float32)
    for i in range(rows):
        a = (i % 32) // 4
        members = [16 * blk + (2 * a + blk) % 16 for blk in range(16)]
        out[i] = q[members].sum(axis=0) + 0.02 * rng.standard_normal(D, dtype=np.float32)
    return unit(out)


def plant(c, q, tiles, seed=5):
    c = c.copy()
    for j, t in enumerate(tiles):
        c[32 * t:32 * t + 32] = planted_rows(q, 32, seed + j)
    return c


def both(ix, q, k, mask=None):
    out = {}
    for on in (0, 1):
        ix.set_option("TS_MFMA_SCREEN", on)
        s, i, st = ix.search(q, k, algo="mfma", return_stats=True, mask=mask)
        out[on] = (np.asarray(s).copy(), np.asarray(i).copy(), st)
    ix.set_option("TS_MFMA_SCREEN", None)
    return out


def assert_same(out, what):
    (s0, i0, st0), (s1, i1, st1) = out[0], out[1]
    print(what, "fallback_queries unscreened / screened:", st0["fallback_queries"], st1["fallback_queries"],
          "candidates per query:", st0["candidates"] / max(1, i0.shape[0]), st1["candidates"] / max(1, i1.shape[0]))
    bad = np.argwhere(i0 != i1)
    assert bad.size == 0, (what, bad[:5].tolist())
    assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), what


def planted_found(out, tiles, q_member):
    """The planted rows are what the search returns for a query they were built from."""
    ids = out[1][1][q_member]
    return np.isin(ids // 32, np.asarray(tiles)).sum()


def run(ts, c, q, k=10, mask=None):
    ix = ts.TheoremIndex(c.shape[0], D, dtype="bf16", metric="ip")
    try:
        ix.upload(bf16_bits(c), 0)
        return both(ix, bf16_bits(q), k, mask=mask)
    finally:
        ix.close()


def test_one_dense_tile(ts):
    """(a) one tile with 512 passing pairs: several values of a lane, several lanes of a mask, all four blocks of every wave."""
    c, q = base(200_000)
    tiles = [1234]
    out = run(ts, plant(c, q, tiles), q)
    assert_same(out, "one dense tile")
    assert planted_found(out, tiles, 0) >= 4          # query 0 = block 0, a = 0: rows 0 .. 3 of the tile


def test_wave_list_overflows(ts):
    """(b) twelve dense tiles in a row: wherever the workgroups' tile ranges are cut (equal shares or the feedback table, ~24
    tiles each here), some workgroup holds at least six of them = 768 pairs per wave against a list of 384."""
    c, q = base(200_000)
    tiles = list(range(3000, 3012))
    assert 128 * (len(tiles) // 2) > STAGE_CAP
    out = run(ts, plant(c, q, tiles), q)
    assert_same(out, "overflow")
    assert planted_found(out, tiles, 0) == 10
    # a second search on the same data moves the tile ranges (feedback partition): still exact
    out = run(ts, plant(c, q, tiles), q, k=100)
    assert_same(out, "overflow, k = 100")


def test_mask_and_last_tile(ts):
    """(c) n not a multiple of 32 with planted rows in the last tile next to the padding rows, dense tiles elsewhere, and a row
    mask that removes half of the planted rows (and half of everything else)."""
    n = 32 * 6000 + 13
    c, q = base(n)
    tiles = list(range(2000, 2012)) + [4000]
    c = plant(c, q, tiles)
    c[32 * 6000:] = planted_rows(q, 13, 99)                     # the real rows of the last tile
    out = run(ts, c, q, k=100)                                  # k = 100: room for all 56 planted rows of a query
    assert_same(out, "last tile, no mask")
    assert (out[1][1] < n).all() and (out[1][1] >= 0).all()
    assert np.isin(32 * 6000 + np.arange(4), out[1][1][0]).all()        # query 0: rows 0 .. 3 of the last tile
    rng = np.random.default_rng(8)
    mask = rng.random(n) < 0.5
    planted = np.concatenate([np.arange(32 * t, 32 * t + 32) for t in tiles] + [np.arange(32 * 6000, n)])
    mask[planted] = (np.arange(planted.size) % 2) == 0
    out = run(ts, c, q, k=100, mask=mask)
    assert_same(out, "last tile, mask")
    assert mask[out[1][1].ravel()].all()
    assert np.isin(32 * 6000 + np.array([0, 2]), out[1][1][0]).all()    # ... of which the mask keeps rows 0 and 2
    assert not np.isin(32 * 6000 + np.array([1, 3]), out[1][1][0]).any()
    # masks that keep everything / only the planted rows of the last tile
    out = run(ts, c, q, mask=np.ones(n, dtype=bool))
    assert_same(out, "all-true mask")
    few = np.zeros(n, dtype=bool)
    few[32 * 6000:] = True
    few[::7] = True
    out = run(ts, c, q, mask=few)
    assert_same(out, "sparse mask")


@pytest.mark.parametrize("nq", [250, 100, 33])
def test_padding_queries(ts, nq):
    """(d) a batch that does not fill its query blocks: the padding queries' lanes see the dense tiles and, in a tile with a
    non-finite value, a threshold that admits everything - none of it may reach an answer.  (Seen through the answers: the
    lists themselves are internal.)"""
    c, q = base(200_000)
    tiles = list(range(5000, 5008))
    c = plant(c, q, tiles)
    c[32 * 5003 + 7, 11] = np.nan
    c[32 * 777 + 3, 5] = np.inf
    c[32 * 778 + 3, 5] = -np.inf
    out = run(ts, c, q[:nq])
    assert_same(out, ("padding queries", nq))
    assert out[1][1].shape[0] == nq
    assert planted_found(out, tiles, 0) >= 4
