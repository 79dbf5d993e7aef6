"""A numpy mirror of the int8 screen's bound for fp32 indexes (kernels_screen8.h, "fp32 rows"; the quantisers of
kernels_screen8_f32.h; screen_fold_query / screen_thr_piece of kernels_screen8_tile.h) at W = 768 and 1024: the quantisers
with gamma = W * 2^-22, the underflow term W * 2^-85 * (1 + a_t) and the range rule (tiles outside [2^-100, 2^64], queries
outside [2^-40, 2^40]: 1 / s = NaN), the query's side folded in fp64 and rounded to fp32 on the admitting side, three fp32 FMAs
per (tile, query), the clamp and floor.  The fp32 score of the unscreened pass is emulated in the kernel's order of the terms,
k = 16 s + 4 g + i (k-step s ascending, then MFMA i = 0 .. 3, then lane group g = 0 .. 3 inside the instruction), one rounding
per term (the fp64 product plus the accumulator, rounded to fp32: close enough to an fma, the bound carries a factor of 4).
No pair whose emulated score - or whose fp64 score - reaches the threshold has an integer dot product below the integer
threshold; out-of-range tiles and queries get INT_MIN; and on Gaussian rows the screen does screen."""
import numpy as np
import pytest

f32 = np.float32
INT_MIN = -2 ** 31
SCREEN_CAP = 65536             # kScreenCap (kernels_screen8.h)
TILE_RANGE = (2.0 ** -100, 2.0 ** 64)
QUERY_RANGE = (2.0 ** -40, 2.0 ** 40)


def up(v):
    """fp64 -> fp32, never below (NaN stays NaN)."""
    f = v.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f)


def down(v):
    """fp64 -> fp32, never above (NaN stays NaN)."""
    f = v.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f)


def in_range(amax, lo, hi):
    return (amax == 0) | ((amax >= f32(lo)) & (amax <= f32(hi)))


def quantize_tiles(x):
    """quantize_tiles_f32_kernel<W>: x [n x W] fp32, n a multiple of 32 -> int8 rows, per tile (1 / s_t, E_t, X_t)."""
    W = x.shape[1]
    t = x.reshape(-1, 32, W)
    fin = np.isfinite(t)
    amax = np.where(fin, np.abs(t), 0).max(axis=(1, 2)).astype(np.float32)
    bad = ~fin.all(axis=(1, 2)) | ~in_range(amax, *TILE_RANGE)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.where((amax > 0) & ~bad, amax / f32(127), f32(1)).astype(np.float32)
        qx = np.where(fin, np.clip(np.rint(t / s[:, None, None]), -127, 127), 0).astype(np.float32)
        sx = s[:, None, None].astype(np.float64) * qx
        e = np.where(fin, t.astype(np.float64) - sx, 0)
        emax = np.sqrt((e * e).sum(axis=2)).max(axis=1) * (1 + 2.0 ** -40)
        xmax = np.sqrt((sx * sx).sum(axis=2)).max(axis=1) * (1 + 2.0 ** -40)
        gamma = float(f32(W * 2.0 ** -22))
        et = emax + gamma * (xmax + emax) * (1 + 2.0 ** -20) + W * 2.0 ** -85 * (1.0 + amax.astype(np.float64))
        rs = np.where(bad, np.float32(np.nan), f32(1) / s).astype(np.float32)
        return (qx.reshape(-1, W).astype(np.int8), rs, np.where(bad, f32(0), up(et)).astype(np.float32),
                np.where(bad, f32(0), up(xmax)).astype(np.float32), bad)


def quantize_queries(q):
    """quantize_queries_f32_kernel<W>: int8 rows, 1 / s_q, |e_q|, |q|."""
    fin = np.isfinite(q)
    amax = np.where(fin, np.abs(q), 0).max(axis=1).astype(np.float32)
    bad = ~fin.all(axis=1) | ~in_range(amax, *QUERY_RANGE)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.where((amax > 0) & ~bad, amax / f32(127), f32(1)).astype(np.float32)
        qx = np.where(fin, np.clip(np.rint(q / s[:, None]), -127, 127), 0).astype(np.float32)
        e = np.where(fin, q.astype(np.float64) - s[:, None].astype(np.float64) * qx, 0)
        rq = np.where(bad, np.float32(np.nan), f32(1) / s).astype(np.float32)
        eq = up(np.sqrt((e * e).sum(axis=1)) * (1 + 2.0 ** -40))
        qn = up(np.sqrt((np.where(fin, q, 0).astype(np.float64) ** 2).sum(axis=1)) * (1 + 2.0 ** -40))
    return qx.astype(np.int8), rq, np.where(bad, f32(0), eq).astype(np.float32), np.where(bad, f32(0), qn).astype(np.float32), bad


def fma32(a, b, c):
    """fp32 fma emulated through fp64: the product of two fp32 values is exact in fp64, the sum is rounded twice."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def fold_query(thr, rq, eq, qn):
    """screen_fold_query: [queries] -> q1, q2, q3."""
    athr = np.where(np.isinf(thr), 0.0, np.abs(thr.astype(np.float64)))
    with np.errstate(invalid="ignore", over="ignore"):
        v1 = rq.astype(np.float64) * (thr.astype(np.float64) - athr * 2.0 ** -18)
        v2 = rq.astype(np.float64) * qn.astype(np.float64) * (1 + 2.0 ** -18)
        v3 = rq.astype(np.float64) * eq.astype(np.float64) * (1 + 2.0 ** -18)
        return down(v1), up(v2), up(v3)


def folded_thr(tx, ty, tz, q1, q2, q3):
    """screen_thr_piece 0 .. 3: [tiles] x [queries]."""
    T = lambda v: np.broadcast_to(v[:, None], (tx.size, q1.size))
    Q = lambda v: np.broadcast_to(v[None, :], (tx.size, q1.size))
    t = fma32(-T(ty), Q(q2), Q(q1))
    t = fma32(-T(tz), Q(q3), t)
    t = fma32(T(tx), t, np.full(t.shape, -1.0, np.float32))
    w = np.fmin(np.fmax(t, f32(-2.0 ** 31)), f32(2.0 ** 30))                      # maxNum: NaN -> -2^31
    return np.floor(w).astype(np.int64)


def kernel_order(W):
    """The order in which the fp32 pass adds the terms of a row's score: k = 16 s + 4 g + i."""
    return [16 * s + 4 * g + i for s in range(W // 16) for i in range(4) for g in range(4)]


def fp32_scores(x, qrow):
    """The pass's fp32 score of every row of x [n x W] with one query: a chain from zero in the kernel's order, every term
    the fp64 product added to the accumulator and rounded to fp32."""
    acc = np.zeros(x.shape[0], np.float32)
    xt = np.ascontiguousarray(x.T).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in kernel_order(x.shape[1]):
            acc = (acc.astype(np.float64) + xt[k] * float(qrow[k])).astype(np.float32)
    return acc


def check(x, q, ranks, what):
    xi, tx, ty, tz, tbad = quantize_tiles(x)
    qi, rq, eq, qn, qbad = quantize_queries(q)
    with np.errstate(invalid="ignore", over="ignore"):
        exact = x.astype(np.float64) @ q.astype(np.float64).T                      # [n x nq]
    emu = np.stack([fp32_scores(x, q[j]) for j in range(q.shape[0])], axis=1)
    I = xi.astype(np.float64) @ qi.astype(np.float64).T
    assert np.abs(I).max() <= 127 * 127 * x.shape[1] < 2 ** 24
    srt = np.sort(np.where(np.isfinite(exact), exact, -np.inf), axis=0)
    counts, admitted = [], []
    for rank in ranks:
        thr = srt[-rank].astype(np.float32)                                         # a threshold near the answers
        new = folded_thr(tx, ty, tz, *fold_query(thr, rq, eq, qn))                  # [tiles x nq]
        # out of range, or a non-finite value: everything is admitted
        assert (new[tbad] == INT_MIN).all() and (new[:, qbad] == INT_MIN).all(), what
        passed = I >= np.repeat(new, 32, axis=0)
        with np.errstate(invalid="ignore"):
            must = (exact >= thr.astype(np.float64)[None, :]) | (emu >= thr[None, :])
        missed = np.argwhere(must & ~passed)
        per_query = passed.sum(axis=0)
        print(f"{what} rank {rank}: pairs that must pass {int(must.sum())}, admitted per query min {per_query.min()} "
              f"median {int(np.median(per_query))} max {per_query.max()} of {x.shape[0]} rows; tiles out of range / non-finite {int(tbad.sum())}")
        assert missed.size == 0, (what, rank, missed[:5].tolist())
        counts.append(per_query)
        admitted.append(passed)
    return counts, tbad, qbad, admitted                                             # admitted: [rank][n x nq]


def gaussian(n, W, nq, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n, W)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q = rng.standard_normal((nq, W)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return rng, c, q


@pytest.mark.parametrize("W", [768, 1024])
def test_gaussian_no_false_negatives(W):
    n = 32 * 1024
    rng, c, q = gaussian(n, W, 8, 1 + W)
    counts, tbad, qbad, admitted = check(c, q, (1, 10, 100), f"gaussian {W}")
    assert not tbad.any() and not qbad.any()
    # and it does screen, at every threshold checked: the admitted pairs of a query stay under an eighth of its list
    # (kScreenCap / 8) and far under the corpus - a bound that admits everything fails here
    for per_query in counts:
        assert per_query.max() < SCREEN_CAP // 8 and per_query.mean() < 0.2 * n, per_query


@pytest.mark.parametrize("W", [768, 1024])
def test_adversarial_no_false_negatives(W):
    n = 32 * 256
    rng, c, q = gaussian(n, W, 8, 2 + W)
    c[::7, 3] = 40.0                                                   # one huge element: a coarse tile scale
    al = np.arange(1, n, 5)
    c[al] = (np.round(rng.standard_normal((al.size, W)) * 4) / 4 + 0.05 * q[al % 8]).astype(np.float32)   # e_x along a query
    c[100:164] = c[7]                                                  # duplicates across tiles
    best = np.argsort(-(c.astype(np.float64) @ q[0].astype(np.float64)))[:3]
    c[2000:2096:8] = c[best[2]]                                        # rows on the threshold of rank 3 .. 14, across tiles
    c[300:332] = 0.0                                                   # a zero tile
    c[400, 9] = np.nan
    c[500, 2] = np.inf
    c[600, 1] = -np.inf
    q[3, 0] = 30.0                                                     # a query with a coarse scale
    counts, tbad, qbad, admitted = check(c, q, (1, 3, 10, 100), f"adversarial {W}")
    assert tbad[[400 // 32, 500 // 32, 600 // 32]].all() and not tbad[300 // 32] and int(tbad.sum()) == 3


@pytest.mark.parametrize("W", [768, 1024])
def test_scaled_tiles_and_the_range_rule(W):
    """Inner-product rows far from unit length: tiles scaled by 2^-60 and 2^40 are inside the range and are screened with their
    own scales; tiles scaled by 2^-110, 2^-140 (subnormal values) and 2^70, and queries scaled by 2^-50 and 2^50, are outside:
    INT_MIN, every pair admitted."""
    n = 32 * 128
    rng, c, q = gaussian(n, W, 8, 3 + W)
    scale = {3: -60, 4: -60, 10: 40, 50: 40, 20: -110, 21: -140, 30: 70}
    with np.errstate(under="ignore"):
        for t, e in scale.items():
            c[32 * t:32 * t + 32] *= f32(2.0) ** e if e > -127 else f32(2.0) ** -70 * f32(2.0) ** (e + 70)
    c[32 * 60 + 5] *= f32(2.0) ** 40                                   # one such row inside an ordinary tile
    q[6] *= f32(2.0) ** -50
    q[7] *= f32(2.0) ** 50
    counts, tbad, qbad, admitted = check(c, q, (1, 10, 70, 200), f"scaled {W}")
    assert sorted(np.flatnonzero(tbad)) == [20, 21, 30], np.flatnonzero(tbad)
    assert sorted(np.flatnonzero(qbad)) == [6, 7], np.flatnonzero(qbad)
    # the in-range scaled tiles are screened, not merely admitted: at rank 200 (a threshold among the ordinary rows) the 2^-60
    # tiles pass nothing for the in-range queries
    passed = admitted[3]
    assert not passed[32 * 3:32 * 5, :6].any()
    assert passed[32 * 20:32 * 22].all() and passed[32 * 30:32 * 31].all() and passed[:, 6:].all()


def test_order_is_the_kernels():
    """k = 16 s + 4 (lane >> 4) + i: every term once; a k-step's first MFMA adds elements 0, 4, 8, 12 of its 16."""
    for W in (768, 1024):
        o = kernel_order(W)
        assert sorted(o) == list(range(W))
        assert o[:8] == [0, 4, 8, 12, 1, 5, 9, 13] and o[16:20] == [16, 20, 24, 28]
