"""The int8 screen of the d = 768 bf16 full pass (kernels_screen8.h) returns exactly what the unscreened bf16 pass returns:
on one index, TS_MFMA_SCREEN=1 and TS_MFMA_SCREEN=0 must give identical ids and identical score bits - Gaussian rows,
the clustered corpus of the exact-tie tests, adversarial rows (coarse scales, rounding errors aligned with a query, rows on
the threshold, duplicates, zero / NaN / Inf rows), masks, n not a multiple of 32, batch sizes, k, views, and rows written
after the image was made."""
import concurrent.futures
import functools

import numpy as np
import pytest

import exact_common as E
from synthetic import bf16_bits

pytestmark = pytest.mark.gpu

D = 768


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
def gaussian(n=400_003, nq=256, seed=11):
    rng = np.random.default_rng(seed)
    return bf16_bits(unit(rng.standard_normal((n, D), dtype=np.float32))), bf16_bits(unit(rng.standard_normal((nq, D), dtype=np.float32)))


def adversarial(n=200_017, nq=64, seed=12, huge_every=640):
    """Gaussian rows with: one huge element per row (a coarse tile scale), rows whose rounding error points along a query,
    rows on a query's threshold (copies of its best rows), duplicates, zero rows, NaN and +-Inf rows."""
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


def both(ix, q, k, mask=None):
    out = {}
    for on in (0, 1):
        ix.set_option("TS_MFMA_SCREEN", on)
        s, i, st = ix.search(q, k, algo="mfma", return_stats=True, mask=mask)
        out[on] = (np.asarray(s).copy(), np.asarray(i).copy(), st)
    ix.set_option("TS_MFMA_SCREEN", None)
    return out


def assert_same(out, what):
    (s0, i0, _), (s1, i1, _) = out[0], out[1]
    bad = np.argwhere(i0 != i1)
    assert bad.size == 0, (what, bad[:5].tolist())
    assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), what


@pytest.mark.parametrize("nq,k", [(1, 10), (17, 1), (64, 100), (200, 10), (256, 10), (256, 256)])
def test_gaussian(ts, nq, k):
    c, q = gaussian()
    ix = make(ts, c)
    try:
        assert_same(both(ix, q[:nq], k), ("gaussian", nq, k))
    finally:
        ix.close()


def test_gaussian_mask_and_view(ts):
    c, q = gaussian()
    ix = make(ts, c)
    try:
        mask = np.random.default_rng(3).random(c.shape[0]) < 0.3
        assert_same(both(ix, q, 10, mask=mask), "mask")
        v = ix.view()
        try:
            s0, i0 = ix.search(q, 10, algo="mfma")
            s1, i1 = v.search(q, 10, algo="mfma")
            assert np.array_equal(i0, i1) and np.array_equal(np.asarray(s0).view(np.uint32), np.asarray(s1).view(np.uint32))
        finally:
            v.close()
    finally:
        ix.close()


def test_adversarial(ts):
    c, q = adversarial()
    ix = make(ts, c)
    try:
        for nq, k in ((64, 10), (64, 100), (33, 1)):
            assert_same(both(ix, q[:nq], k), ("adversarial", nq, k))
    finally:
        ix.close()


def test_adversarial_coarse_everywhere(ts):
    """A huge element in one row of 20: most tiles get a scale so coarse that the screen passes more pairs than its lists
    hold.  Those queries go to the exact re-run - as an over-full list of the unscreened pass does - whose scores are exact
    in another summation order: the same rows, scores within fp32 rounding."""
    c, q = adversarial(huge_every=20)
    ix = make(ts, c)
    try:
        out = both(ix, q, 10)
        if out[0][2]["fallback_queries"] == 0 and out[1][2]["fallback_queries"] == 0:
            assert_same(out, "coarse")
        else:
            assert np.array_equal(out[0][1], out[1][1])
            assert np.allclose(out[0][0], out[1][0], rtol=1e-5, atol=1e-6)
    finally:
        ix.close()


def test_clustered_corpus(ts):
    q, c, _ = E.make_corpus("ip", 150_001, D, 256, 1768)
    ix = make(ts, bf16_bits(c))
    try:
        qb = bf16_bits(q)
        for nq, k in ((256, 10), (64, 256), (17, 100)):
            assert_same(both(ix, qb[:nq], k), ("clustered", nq, k))
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
    finally:
        ix.close()
