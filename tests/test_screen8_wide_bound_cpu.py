"""A numpy mirror of the int8 screen at d = 1024 (kernels_screen8.h with W = 1024; screen_fold_query / screen_thr_piece in
kernels_screen8_tile.h): the quantisers with gamma = 1024 * 2^-22, the query's side folded in fp64 and rounded to fp32 on the
admitting side, three fp32 FMAs per (tile, query), the clamp and floor.  The fp32 score of the unscreened pass is emulated in
both of its summation orders - one chain of 32 k-steps, and the k-split's two chains of 16 k-steps added once - each in two
models of a k-step (its 32 exact products added in fp64 and rounded once into the accumulator; every product added in fp32,
one after the other).  No pair whose score reaches the threshold in any of them, or in fp64, is screened out; the admitted
pairs per query are printed, and on Gaussian rows the screen must screen."""
import numpy as np
import pytest

from synthetic import bf16_bits, bf16_bits_to_f32

D = 1024
GAMMA = np.float32(1024.0 * 2.0 ** -22)
f32 = np.float32
KSTEP = 32                     # elements of a k-step of v_mfma_f32_16x16x32_bf16
UNIT_STEPS = 8                 # k-steps of a unit of the d = 1024 pass; each half of a k-split workgroup's waves takes four


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


def quantize_tiles(x):
    """quantize_tiles_kernel<1024>: x [n x 1024] fp32 values of bf16 rows, n a multiple of 32 -> int8 rows, per tile
    (1 / s_t, E_t, X_t)."""
    t = x.reshape(-1, 32, D)
    fin = np.isfinite(t)
    amax = np.where(fin, np.abs(t), 0).max(axis=(1, 2)).astype(np.float32)
    s = np.where(amax > 0, amax / f32(127), f32(1)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        qx = np.where(fin, np.clip(np.rint(t / s[:, None, None]), -127, 127), 0).astype(np.float32)
    sx = s[:, None, None].astype(np.float64) * qx
    e = np.where(fin, t.astype(np.float64) - sx, 0)
    emax = np.sqrt((e * e).sum(axis=2)).max(axis=1) * (1 + 2.0 ** -40)
    xmax = np.sqrt((sx * sx).sum(axis=2)).max(axis=1) * (1 + 2.0 ** -40)
    bad = ~fin.all(axis=(1, 2))
    rs = np.where(bad, np.float32(np.nan), f32(1) / s).astype(np.float32)
    et = up(emax + float(GAMMA) * (xmax + emax) * (1 + 2.0 ** -20))
    return qx.reshape(-1, D).astype(np.int8), rs, et, up(xmax)


def quantize_queries(q):
    """screen_quantize_query<1024>: int8 rows, 1 / s_q, |e_q|, |q|."""
    fin = np.isfinite(q)
    amax = np.where(fin, np.abs(q), 0).max(axis=1).astype(np.float32)
    s = np.where(amax > 0, amax / f32(127), f32(1)).astype(np.float32)
    qx = np.where(fin, np.clip(np.rint(q / s[:, None]), -127, 127), 0).astype(np.float32)
    e = q.astype(np.float64) - s[:, None].astype(np.float64) * qx
    bad = ~fin.all(axis=1)
    rq = np.where(bad, np.float32(np.nan), f32(1) / s).astype(np.float32)
    return qx.astype(np.int8), rq, up(np.sqrt((e * e).sum(axis=1)) * (1 + 2.0 ** -40)), up(np.sqrt((q.astype(np.float64) ** 2).sum(axis=1)) * (1 + 2.0 ** -40))


def fma32(a, b, c):
    """fp32 fma emulated through fp64: the product of two fp32 values is exact in fp64, the sum is rounded twice."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def fold_query(thr, rq, eq, qn):
    """screen_fold_query: [queries] -> q1, q2, q3."""
    athr = np.where(np.isinf(thr), 0.0, np.abs(thr.astype(np.float64)))
    with np.errstate(invalid="ignore"):
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


CHAIN = [list(range(D // KSTEP))]                                                           # the plain form: k-steps 0 .. 31
HALVES = [[UNIT_STEPS * u + (UNIT_STEPS // 2) * h + i for u in range(D // KSTEP // UNIT_STEPS) for i in range(UNIT_STEPS // 2)]
          for h in (0, 1)]                                                                 # the k-split form


def fp32_scores(x, qrow, chains, sequential):
    """The pass's fp32 score of every row of x [n x 1024] with one query: each chain starts from zero and takes its k-steps in
    order, the chains' sums are added in fp32.  sequential: every product joins the accumulator in fp32, one after the other;
    else a k-step's 32 exact products are added in fp64 and that sum is rounded into the accumulator once."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.ascontiguousarray((x * qrow[None, :]).T)                       # [1024 x n] fp32: bf16 x bf16 products are exact
        total = None
        for steps in chains:
            acc = np.zeros(x.shape[0], np.float32)
            for ks in steps:
                if sequential:
                    for e in range(KSTEP * ks, KSTEP * ks + KSTEP):
                        acc = acc + p[e]
                else:
                    acc = (acc.astype(np.float64) + p[KSTEP * ks:KSTEP * ks + KSTEP].astype(np.float64).sum(axis=0)).astype(np.float32)
            total = acc if total is None else total + acc
    assert total.dtype == np.float32
    return total


def check(c_bits, q_bits, ranks, what):
    x = bf16_bits_to_f32(c_bits)
    q = bf16_bits_to_f32(q_bits)
    xi, tx, ty, tz = quantize_tiles(x)
    qi, rq, eq, qn = quantize_queries(q)
    with np.errstate(invalid="ignore", over="ignore"):
        exact = x.astype(np.float64) @ q.astype(np.float64).T                      # [n x nq]
    # the pass's scores in both orders and both models of a k-step: [4][n x nq]
    emu = [np.stack([fp32_scores(x, q[j], chains, seq) for j in range(q.shape[0])], axis=1)
           for chains in (CHAIN, HALVES) for seq in (False, True)]
    differ = int((emu[0].view(np.uint32) != emu[2].view(np.uint32)).sum())
    print(f"{what}: scores whose bits differ between the chain and the two half-chains: {differ} of {emu[0].size}")
    # integer dot products, exact in fp64 (|x~ . q~| <= 127 * 127 * 1024 < 2^24)
    I = xi.astype(np.float64) @ qi.astype(np.float64).T
    assert np.abs(I).max() <= 127 * 127 * D < 2 ** 24
    srt = np.sort(np.where(np.isnan(exact), -np.inf, exact), axis=0)
    counts = []
    for rank in ranks:
        thr = srt[-rank].astype(np.float32)                                         # a threshold near the answers
        new = folded_thr(tx, ty, tz, *fold_query(thr, rq, eq, qn))                  # [tiles x nq]
        passed = I >= np.repeat(new, 32, axis=0)
        with np.errstate(invalid="ignore"):
            must = exact >= thr.astype(np.float64)[None, :]
            for s in emu:
                must |= s >= thr[None, :]
        missed = np.argwhere(must & ~passed)
        per_query = passed.sum(axis=0)
        print(f"{what} rank {rank}: pairs that must pass {int(must.sum())}, admitted per query min {per_query.min()} "
              f"median {int(np.median(per_query))} max {per_query.max()} of {x.shape[0]} rows")
        assert missed.size == 0, (rank, missed[:5].tolist())
        counts.append(per_query)
    return counts


def gaussian(n, nq, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n, D)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q = rng.standard_normal((nq, D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return rng, c, q


@pytest.mark.timeout(900)
def test_gaussian_no_false_negatives():
    rng, c, q = gaussian(32 * 512, 16, 1)
    counts = check(bf16_bits(c), bf16_bits(q), (1, 10, 100), "gaussian")
    assert counts[1].mean() < 0.2 * c.shape[0]          # and it does screen: a bound that admits everything fails here


@pytest.mark.timeout(900)
def test_adversarial_no_false_negatives():
    n = 32 * 512
    rng, c, q = gaussian(n, 16, 2)
    c[::7, 3] = 40.0                                                   # one huge element: a coarse tile scale
    al = np.arange(1, n, 5)
    c[al] = np.round(rng.standard_normal((al.size, D)) * 4) / 4 + 0.05 * q[al % 16]   # e_x along a query
    c[100:164] = c[7]                                                  # duplicates across tiles
    c[300:332] = 0.0                                                   # a zero tile
    c[400, 9] = np.nan
    c[500, 2] = np.inf
    c[600, 1] = -np.inf
    q[3, 0] = 30.0                                                     # a query with a coarse scale
    check(bf16_bits(c), bf16_bits(q), (1, 10, 100), "adversarial")


def test_orders_are_the_kernels():
    """The two half-chains of the k-split cover every k-step once: half h takes k-steps 8 u + 4 h .. 8 u + 4 h + 3."""
    assert HALVES[0] == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27]
    assert sorted(HALVES[0] + HALVES[1]) == CHAIN[0]
