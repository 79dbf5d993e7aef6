"""The opt-in int8 screen of the d = 1024 bf16 full pass (TS_MFMA_SCREEN_WIDE; kernels_screen8.h, launch_screen8_wide.hip)
returns exactly what the unscreened pass returns: on one index, the option on and off must give identical ids and identical
score bits - whichever arithmetic form the unscreened pass takes (one chain of 32 k-steps, or the paired pass's two half-chains
added: batch size, TS_MFMA_PAIR and TS_MFMA_GRID select it) - on Gaussian rows, adversarial rows (coarse scales, rounding
errors aligned with a query, rows on the threshold, duplicates, zero / NaN / Inf rows), masks, n not a multiple of 32, views,
and rows written after the image was made.  With the option on the ids also equal the fp64 truth where that pins them."""
import concurrent.futures
import functools

import numpy as np
import pytest

from oracle import oracle
from synthetic import bf16_bits, bf16_bits_to_f32

pytestmark = pytest.mark.gpu

D = 1024
KNOB = "TS_MFMA_SCREEN_WIDE"


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


def unit(x):
    x = x.astype(np.float32)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


@functools.lru_cache(maxsize=1)
def gaussian(n=400_003, nq=256, seed=21):
    rng = np.random.default_rng(seed)
    return bf16_bits(unit(rng.standard_normal((n, D), dtype=np.float32))), bf16_bits(unit(rng.standard_normal((nq, D), dtype=np.float32)))


def adversarial(n=200_017, nq=256, seed=22, huge_every=640):
    """Gaussian rows with: one huge element per row (a coarse tile scale), rows whose rounding error points along a query,
    rows on a query's threshold (copies of its best rows, across tiles), duplicates, zero rows, NaN and +-Inf rows."""
    rng = np.random.default_rng(seed)
    c = unit(rng.standard_normal((n, D), dtype=np.float32))
    q = unit(rng.standard_normal((nq, D), dtype=np.float32))
    huge = rng.choice(n, n // huge_every, replace=False)
    c[huge, rng.integers(0, D, huge.size)] = 40.0
    # e_x || q: rows built as a coarse grid value plus a small multiple of a query
    al = rng.choice(n, n // 20, replace=False)
    base = np.round(rng.standard_normal((al.size, D)) * 4) / 4
    c[al] = unit(base + 0.05 * q[rng.integers(0, nq, al.size)])
    # the best rows of some queries, copied many times (ties on and around the threshold) and across tiles
    s = c[:20000] @ q[:8].T
    top = np.argsort(-s, axis=0)[:12].ravel()
    dst = rng.choice(np.setdiff1d(np.arange(n), np.concatenate([huge, al])), top.size * 6, replace=False)
    c[dst] = np.repeat(c[top], 6, axis=0)
    z = rng.choice(n, 100, replace=False)
    c[z] = 0.0
    c[z[:10], 5] = np.nan
    c[z[10:20], 7] = np.inf
    c[z[20:30], 9] = -np.inf
    return bf16_bits(c), bf16_bits(q)


def make(ts, c, chunk=None):
    ix = ts.TheoremIndex(c.shape[0], D, dtype="bf16", metric="ip")
    if chunk is None:
        ix.upload(c, 0)
    else:
        starts = list(range(0, c.shape[0], chunk))
        np.random.default_rng(5).shuffle(starts)
        with concurrent.futures.ThreadPoolExecutor(16) as pool:
            list(pool.map(lambda a: ix.upload(c[a:a + chunk], a), starts))
    return ix


def both(ix, q, k, mask=None, matrix_path=True):
    """The search with the option off (0) and on (1); asserts that the stats say which pass ran.  matrix_path=False: a search
    the library serves with the streaming scan whatever the option says (it is asked for with algo="auto")."""
    out = {}
    try:
        for on in (0, 1):
            ix.set_option(KNOB, on)
            s, i, st = ix.search(q, k, algo="mfma" if matrix_path else "auto", return_stats=True, mask=mask)
            out[on] = (np.asarray(s).copy(), np.asarray(i).copy(), st)
            if matrix_path:
                assert st["algo"] == 2 and st["levels"] >= 2, st
                assert st["screened"] == on, (on, st)
            else:
                assert st["algo"] == 1 and st["screened"] == 0, (on, st)
    finally:
        ix.set_option(KNOB, None)
    return out


def assert_same(out, what):
    (s0, i0, st0), (s1, i1, st1) = out[0], out[1]
    print(what, "fallback_queries off / on:", st0["fallback_queries"], st1["fallback_queries"],
          "candidates off / on:", st0["candidates"], st1["candidates"])
    bad = np.argwhere(i0 != i1)
    assert bad.size == 0, (what, bad[:5].tolist())
    assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), what


@pytest.fixture(scope="module")
def gauss_index(ts):
    c, q = gaussian()
    ix = make(ts, c)
    yield ix, q
    ix.close()


def test_knob_and_stats(ts, gauss_index):
    """The option exists, is off by default, and `screened` tells which full pass ran."""
    ix, q = gauss_index
    s, i, st = ix.search(q, 10, algo="mfma", return_stats=True)
    assert st["levels"] >= 2 and st["screened"] == 0, st
    ix.set_option(KNOB, 1)
    try:
        s, i, st = ix.search(q, 10, algo="mfma", return_stats=True)
        assert st["levels"] >= 2 and st["screened"] == 1, st
        ix.set_option("TS_MFMA_SCREEN", 0)          # the screen's main switch covers the wide one
        try:
            s, i, st = ix.search(q, 10, algo="mfma", return_stats=True)
            assert st["screened"] == 0, st
        finally:
            ix.set_option("TS_MFMA_SCREEN", None)
    finally:
        ix.set_option(KNOB, None)
    s, i, st = ix.search(q, 10, algo="mfma", return_stats=True)
    assert st["screened"] == 0, st


@pytest.mark.parametrize("nq,k", [(1, 10), (17, 1), (64, 100), (150, 10), (192, 100), (193, 1), (193, 256), (200, 10), (256, 10),
                                  (256, 100), (256, 256)])
def test_gaussian(ts, gauss_index, nq, k):
    ix, q = gauss_index
    assert_same(both(ix, q[:nq], k), ("gaussian", nq, k))


@pytest.mark.parametrize("nq", [193, 256])
@pytest.mark.parametrize("opt", [("TS_MFMA_PAIR", 0), ("TS_MFMA_PAIR", 1), ("TS_MFMA_PAIR", None), ("TS_MFMA_GRID", 48),
                                 ("TS_MFMA_GRID", 200)])
def test_gaussian_pass_forms(ts, gauss_index, nq, opt):
    """193 .. 256 queries: the unscreened pass is the paired k-split form (default), the paired plain form (TS_MFMA_PAIR=1), or
    two unpaired launches (TS_MFMA_PAIR=0; a grid that is not a multiple of 16) - the rescore follows each.  (A grid of 48
    workgroups is three groups of 16: pairs again, on a small grid; 200 is the grid without pairs.)"""
    ix, q = gauss_index
    name, v = opt
    ix.set_option(name, v)
    try:
        for k in (10, 100):
            assert_same(both(ix, q[:nq], k), ("forms", name, v, nq, k))
    finally:
        ix.set_option(name, None)


def test_gaussian_masks_and_view(ts, gauss_index):
    """Row masks through the masked form of the screen (VARIANT 14).  The matrix path serves host masks that keep at least a
    tenth of the rows (search.hip; sparser ones leave the threshold sample too few rows and take the scan, as before this
    option existed): the 50 % mask and a 12 % one drive the screen; the 5 % mask must still give the same answers with the
    option on and off, and `screened` must say that no screen ran."""
    ix, q = gauss_index
    n = gaussian()[0].shape[0]
    assert n % 32 != 0
    rng = np.random.default_rng(3)
    for share in (0.5, 0.12, 0.05):
        mask = rng.random(n) < share
        for nq in (256, 64):
            assert_same(both(ix, q[:nq], 10, mask=mask, matrix_path=share >= 0.1), ("mask", share, nq))
    ix.set_option(KNOB, 1)
    try:
        v = ix.view()                       # a view reads rows it does not own: never screened, the same answers
        try:
            v.set_option(KNOB, 1)
            s0, i0, st0 = ix.search(q, 10, algo="mfma", return_stats=True)
            s1, i1, st1 = v.search(q, 10, algo="mfma", return_stats=True)
            assert st0["screened"] == 1 and st1["screened"] == 0, (st0, st1)
            assert np.array_equal(i0, i1) and np.array_equal(np.asarray(s0).view(np.uint32), np.asarray(s1).view(np.uint32))
        finally:
            v.close()
    finally:
        ix.set_option(KNOB, None)


@pytest.mark.parametrize("k", [10, 100, 256])
def test_against_fp64_truth(ts, gauss_index, k):
    """Not only against itself: with the option on, the ids equal the fp64 truth at every pinned position (fp64 gap to both
    neighbours > 1e-6, the rule of the other search tests), and at least 95 % of the positions are pinned."""
    ix, q = gauss_index
    c = gaussian()[0]
    ix.set_option(KNOB, 1)
    try:
        s, i, st = ix.search(q, k, algo="mfma", return_stats=True)
    finally:
        ix.set_option(KNOB, None)
    assert st["screened"] == 1, st
    truth = oracle.scores_fp64(bf16_bits_to_f32(q), bf16_bits_to_f32(c))
    r = oracle.check_topk_against_truth(truth, np.asarray(i), np.asarray(s), k)
    print("k", k, "pinned", r["pinned"], "of", r["positions"], "recall", r["recall"])
    assert r["pinned"] >= 0.95 * r["positions"], r
    assert r["recall"] == 1.0, r


def test_adversarial(ts):
    c, q = adversarial()
    ix = make(ts, c)
    try:
        for nq, k in ((64, 10), (64, 100), (33, 1), (256, 10), (200, 100)):
            assert_same(both(ix, q[:nq], k), ("adversarial", nq, k))
    finally:
        ix.close()


def test_fresh_after_threaded_uploads_and_append(ts):
    c, q = gaussian()
    n0 = 300_001
    ix = make(ts, c[:n0], chunk=25_013)           # chunks that are not whole tiles, written in random order by 16 threads
    try:
        assert_same(both(ix, q, 10), "threaded uploads")
        ix.append(c[n0:])                          # grows the allocation: the image is made anew
        assert_same(both(ix, q, 10), "append")
        ix.upload(c[:1000][::-1].copy(), 5)       # overwrite rows the image already holds
        assert_same(both(ix, q, 10), "overwrite")
        assert_same(both(ix, q[:100], 10), "overwrite, 100 queries")
    finally:
        ix.close()


def test_d768_untouched(ts):
    """d = 768 is screened by default, whatever the wide option says."""
    rng = np.random.default_rng(31)
    c = bf16_bits(unit(rng.standard_normal((150_001, 768), dtype=np.float32)))
    q = bf16_bits(unit(rng.standard_normal((256, 768), dtype=np.float32)))
    ix = ts.TheoremIndex(c.shape[0], 768, dtype="bf16", metric="ip")
    try:
        ix.upload(c, 0)
        res = {}
        for v in (None, 0, 1):
            ix.set_option(KNOB, v)
            s, i, st = ix.search(q, 10, algo="mfma", return_stats=True)
            assert st["screened"] == 1 and st["levels"] >= 2, (v, st)
            res[v] = (np.asarray(s).copy(), np.asarray(i).copy())
        ix.set_option(KNOB, None)
        for v in (0, 1):
            assert np.array_equal(res[None][1], res[v][1])
            assert np.array_equal(res[None][0].view(np.uint32), res[v][0].view(np.uint32))
        ix.set_option("TS_MFMA_SCREEN", 0)
        s, i, st = ix.search(q, 10, algo="mfma", return_stats=True)
        assert st["screened"] == 0, st
    finally:
        ix.close()
