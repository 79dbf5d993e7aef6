"""The opt-in int8 screen of the fp32 full pass at d = 768 and d = 1024 (TS_MFMA_SCREEN_F32; kernels_screen8_f32.h,
launch_screen8_f32.hip) returns exactly what the unscreened fp32 pass returns: on one index, the option on and off must give
identical ids and identical score bits for every query that neither call sent to the exact re-run (both calls report
fallback_queries == 0; otherwise the ids must still be equal - the rule of tests/test_screen8_gpu.py).  Gaussian rows at every
batch size around today's launch boundaries (the unscreened pass holds 64 or 128 queries a launch, the screened one up to 256),
the smallest corpus of the matrix path, screened lists that end on every boundary of a rescore chunk, adversarial rows (coarse
scales, rounding errors aligned with a query, rows on the threshold, zero / NaN / Inf rows), tiles far out of the usual range,
masks, views, the search forms no screen serves (TS_MFMA_STAT=0, TS_MFMA_SAMPLE=0), and rows written after the image was made.  With the option on the ids also equal the fp64 truth where that pins
them."""
import concurrent.futures
import functools

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

KNOB = "TS_MFMA_SCREEN_F32"
SHAPES = {768: 100_003, 1024: 60_001}          # rows of the Gaussian corpus per width: neither a multiple of 32


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


def unit(x):
    x = x.astype(np.float32)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


@functools.lru_cache(maxsize=None)
def gaussian(d, n=None, nq=256):
    rng = np.random.default_rng(31 + d)
    return unit(rng.standard_normal((n or SHAPES[d], d), dtype=np.float32)), unit(rng.standard_normal((nq, d), dtype=np.float32))


def adversarial(d, n=50_017, nq=256, seed=32, huge_every=640):
    """The recipe of the bf16 screen tests in fp32: Gaussian rows with one huge element per row (a coarse tile scale), rows whose
    rounding error points along a query, rows on a query's threshold (copies of its best rows, across tiles), duplicates, zero
    rows, NaN and +-Inf rows."""
    rng = np.random.default_rng(seed + d)
    c = unit(rng.standard_normal((n, d), dtype=np.float32))
    q = unit(rng.standard_normal((nq, d), dtype=np.float32))
    huge = rng.choice(n, n // huge_every, replace=False)
    c[huge, rng.integers(0, d, huge.size)] = 40.0
    al = rng.choice(n, n // 20, replace=False)
    base = np.round(rng.standard_normal((al.size, d)) * 4) / 4
    c[al] = unit(base + 0.05 * q[rng.integers(0, nq, al.size)])
    s = c[:20000] @ q[:8].T
    top = np.argsort(-s, axis=0)[:12].ravel()
    dst = rng.choice(np.setdiff1d(np.arange(n), np.concatenate([huge, al])), top.size * 6, replace=False)
    c[dst] = np.repeat(c[top], 6, axis=0)
    z = rng.choice(n, 100, replace=False)
    c[z] = 0.0
    c[z[:10], 5] = np.nan
    c[z[10:20], 7] = np.inf
    c[z[20:30], 9] = -np.inf
    return c, q


def make(ts, c, chunk=None, metric="ip"):
    ix = ts.TheoremIndex(c.shape[0], c.shape[1], dtype="f32", metric=metric)
    if chunk is None:
        ix.upload(c, 0)
    else:
        starts = list(range(0, c.shape[0], chunk))
        np.random.default_rng(5).shuffle(starts)
        with concurrent.futures.ThreadPoolExecutor(16) as pool:
            list(pool.map(lambda a: ix.upload(c[a:a + chunk], a), starts))
    return ix


def both(ix, q, k, mask=None, matrix_path=True, screened_when_on=1):
    """The search with the option off (0) and on (1); asserts that the stats say which pass ran.  matrix_path=False: a search
    the library serves with the streaming scan whatever the option says (it is asked for with algo="auto").
    screened_when_on=0: a matrix-path search that no screen serves even with the option on."""
    out = {}
    try:
        for on in (0, 1):
            ix.set_option(KNOB, on)
            s, i, st = ix.search(q, k, algo="mfma" if matrix_path else "auto", return_stats=True, mask=mask)
            out[on] = (np.asarray(s).copy(), np.asarray(i).copy(), st)
            if matrix_path:
                assert st["algo"] == 2 and st["levels"] >= 2, st
                assert st["screened"] == (screened_when_on if on else 0), (on, st)
            else:
                assert st["algo"] == 1 and st["screened"] == 0, (on, st)
    finally:
        ix.set_option(KNOB, None)
    return out


def assert_same(out, what, no_fallbacks=False):
    (s0, i0, st0), (s1, i1, st1) = out[0], out[1]
    print(what, "fallback_queries off / on:", st0["fallback_queries"], st1["fallback_queries"],
          "candidates off / on:", st0["candidates"], st1["candidates"])
    if no_fallbacks:
        assert st0["fallback_queries"] == 0 and st1["fallback_queries"] == 0, (what, st0, st1)
    bad = np.argwhere(i0 != i1)
    assert bad.size == 0, (what, bad[:5].tolist())
    if st0["fallback_queries"] == 0 and st1["fallback_queries"] == 0:
        assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), what


@pytest.fixture(scope="module", params=sorted(SHAPES))
def gauss_index(ts, request):
    d = request.param
    c, q = gaussian(d)
    ix = make(ts, c)
    yield ix, q, d
    ix.close()


def test_knob_and_stats(ts, gauss_index):
    """The option exists, is off by default, `screened` tells which full pass ran; the screen's main switch covers it, the
    32x32x2 kernel and a view are never screened."""
    ix, q, d = gauss_index
    s, i, st = ix.search(q, 10, algo="mfma", return_stats=True)
    assert st["levels"] >= 2 and st["screened"] == 0, st
    ix.set_option(KNOB, 1)
    try:
        s1, i1, st1 = ix.search(q, 10, algo="mfma", return_stats=True)
        assert st1["levels"] >= 2 and st1["screened"] == 1, st1
        ix.set_option("TS_MFMA_SCREEN", 0)
        try:
            s, i, st = ix.search(q, 10, algo="mfma", return_stats=True)
            assert st["screened"] == 0, st
        finally:
            ix.set_option("TS_MFMA_SCREEN", None)
        ix.set_option("TS_MFMA_F32", 32)
        try:
            s, i, st = ix.search(q, 10, algo="mfma", return_stats=True)
            assert st["screened"] == 0, st
        finally:
            ix.set_option("TS_MFMA_F32", None)
        v = ix.view()                       # a view reads rows it does not own: never screened, the same answers
        try:
            v.set_option(KNOB, 1)
            sv, iv, stv = v.search(q, 10, algo="mfma", return_stats=True)
            assert stv["screened"] == 0 and stv["levels"] >= 2, stv
            assert stv["fallback_queries"] == 0 and st1["fallback_queries"] == 0, (stv, st1)
            assert np.array_equal(i1, iv) and np.array_equal(np.asarray(s1).view(np.uint32), np.asarray(sv).view(np.uint32))
        finally:
            v.close()
    finally:
        ix.set_option(KNOB, None)
    s, i, st = ix.search(q, 10, algo="mfma", return_stats=True)
    assert st["screened"] == 0, st


@pytest.mark.parametrize("nq,k", [(1, 10), (17, 1), (64, 100), (65, 10), (128, 10), (129, 100), (200, 10), (256, 10), (256, 256)])
def test_gaussian(ts, gauss_index, nq, k):
    ix, q, d = gauss_index
    assert_same(both(ix, q[:nq], k), ("gaussian", d, nq, k), no_fallbacks=True)


@pytest.mark.parametrize("opt", ["TS_MFMA_STAT", "TS_MFMA_SAMPLE"])
def test_other_search_forms_are_not_screened(ts, gauss_index, opt):
    """The guaranteed threshold chain (TS_MFMA_STAT=0: three levels on these corpora, the sparse ones on the fp32 matrix kernel)
    and the list-form sample (TS_MFMA_SAMPLE=0: level 0 on the fp32 matrix kernel) run launches that hold 64 or 128 queries, not
    the screen's 256: with the option on such a search is NOT screened (`screened` == 0), keeps today's query block, and
    returns the ids and score bits it returns with the option off."""
    ix, q, d = gauss_index
    ix.set_option(opt, 0)
    try:
        for nq, k in ((256, 10), (129, 100)):
            assert_same(both(ix, q[:nq], k, screened_when_on=0), ("not screened", opt, d, nq, k))
    finally:
        ix.set_option(opt, None)
    assert_same(both(ix, q, 10), ("screened again", opt, d), no_fallbacks=True)


@pytest.mark.parametrize("d", sorted(SHAPES))
def test_gaussian_cosine(ts, d):
    """The other metric: the rows are normalised at upload, the screen sees what is stored."""
    c, q = gaussian(d)
    ix = make(ts, c[:40_001] * np.float32(3.0), metric="cos")
    try:
        for nq, k in ((256, 10), (100, 100)):
            assert_same(both(ix, q[:nq] * np.float32(0.5), k), ("cosine", d, nq, k), no_fallbacks=True)
    finally:
        ix.close()


@pytest.mark.parametrize("d", sorted(SHAPES))
def test_smallest_matrix_path_corpus(ts, d):
    c, q = gaussian(d)
    ix = make(ts, c[:16_384])
    try:
        assert_same(both(ix, q[:13], 1), ("smallest", d), no_fallbacks=True)
    finally:
        ix.close()


@pytest.mark.parametrize("d", sorted(SHAPES))
def test_rescore_chunk_edges(ts, d):
    """One query's best row copied 1, 15, 16, 17 and 33 times into different tiles: its screened list ends on every boundary of
    a rescore chunk of 16, and the copies come back first, in ascending id order, with equal score bits."""
    c0, q = gaussian(d)
    n = 20_011
    c0 = c0[:n]
    best = int(np.argmax(c0.astype(np.float64) @ q[0].astype(np.float64)))
    rng = np.random.default_rng(7)
    for copies in (1, 15, 16, 17, 33):
        c = c0.copy()
        tiles = rng.choice(np.setdiff1d(np.arange(n // 32), [best // 32]), copies, replace=False)
        dst = np.sort(tiles * 32 + rng.integers(0, 32, copies))
        c[dst] = c0[best]
        ix = make(ts, c)
        try:
            out = both(ix, q[:5], copies + 3)
            assert_same(out, ("chunk edges", d, copies), no_fallbacks=True)
            s1, i1, _ = out[1]
            want = np.sort(np.concatenate([dst, [best]]))
            assert np.array_equal(i1[0, :copies + 1], want), (copies, i1[0], want)
            assert np.unique(s1[0, :copies + 1].view(np.uint32)).size == 1, s1[0]
        finally:
            ix.close()


@pytest.mark.parametrize("d", sorted(SHAPES))
def test_adversarial(ts, d):
    c, q = adversarial(d)
    ix = make(ts, c)
    try:
        for nq, k in ((64, 10), (64, 100), (33, 1), (256, 10), (200, 100)):
            assert_same(both(ix, q[:nq], k), ("adversarial", d, nq, k))
    finally:
        ix.close()


@pytest.mark.parametrize("d", sorted(SHAPES))
def test_scaled_tiles_inner_product(ts, d):
    """Tiles scaled by 2^-60 and 2^40 under the inner-product metric (inside the screen's range: they are quantised with their own
    scales), and by 2^-110 and 2^70 (outside: such tiles admit every pair, the rescore decides)."""
    c, q = gaussian(d)
    c = c[:50_017].copy()
    for t, e in ((100, -60), (101, -60), (700, 40), (900, 40), (300, -110), (1200, 70)):
        c[32 * t:32 * t + 32] *= np.float32(2.0) ** e
    c[32 * 500 + 3] *= np.float32(2.0) ** 40          # one such row inside an ordinary tile
    ix = make(ts, c)
    try:
        for nq, k in ((256, 10), (100, 1), (64, 100)):
            assert_same(both(ix, q[:nq], k), ("scaled tiles", d, nq, k))
    finally:
        ix.close()


def test_masks(ts, gauss_index):
    """Row masks through the masked form of the screen.  The matrix path serves host masks that keep at least a tenth of the rows
    (sparser ones take the scan, as before): the 50 % mask and a 12 % one drive the screen; the 5 % mask must still give the same
    answers with the option on and off, and `screened` must say that no screen ran."""
    ix, q, d = gauss_index
    n = SHAPES[d]
    rng = np.random.default_rng(3)
    for share in (0.5, 0.12, 0.05):
        mask = rng.random(n) < share
        for nq in (256, 64):
            assert_same(both(ix, q[:nq], 10, mask=mask, matrix_path=share >= 0.1), ("mask", d, share, nq))


@pytest.mark.parametrize("d", sorted(SHAPES))
def test_fresh_after_threaded_uploads_and_append(ts, d):
    c, q = gaussian(d)
    n0 = SHAPES[d] * 7 // 10 + 1
    ix = make(ts, c[:n0], chunk=9_013)            # chunks that are not whole tiles, written in random order by 16 threads
    try:
        for nq in (256, 100):
            assert_same(both(ix, q[:nq], 10), ("threaded uploads", d, nq), no_fallbacks=True)
        ix.append(c[n0:])                          # grows the allocation: the image is made anew
        for nq in (256, 100):
            assert_same(both(ix, q[:nq], 10), ("append", d, nq), no_fallbacks=True)
        ix.upload(c[:1000][::-1].copy(), 5)       # overwrite rows the image already holds
        for nq in (256, 100):
            assert_same(both(ix, q[:nq], 10), ("overwrite", d, nq), no_fallbacks=True)
    finally:
        ix.close()


@functools.lru_cache(maxsize=None)
def truth(d):
    c, q = gaussian(d)
    return oracle.scores_fp64(q, c)


@pytest.mark.parametrize("k", [10, 100, 256])
def test_against_fp64_truth(ts, gauss_index, k):
    """Not only against itself: with the option on, the ids equal the fp64 truth at every pinned position (fp64 gap to both
    neighbours > 1e-6, the rule of the other search tests), and at least 95 % of the positions are pinned."""
    ix, q, d = gauss_index
    ix.set_option(KNOB, 1)
    try:
        s, i, st = ix.search(q, k, algo="mfma", return_stats=True)
    finally:
        ix.set_option(KNOB, None)
    assert st["screened"] == 1, st
    r = oracle.check_topk_against_truth(truth(d), np.asarray(i), np.asarray(s), k)
    print("d", d, "k", k, "pinned", r["pinned"], "of", r["positions"], "recall", r["recall"])
    assert r["pinned"] >= 0.95 * r["positions"], r
    assert r["recall"] == 1.0, r
