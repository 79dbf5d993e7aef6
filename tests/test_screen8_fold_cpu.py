"""A numpy mirror of the int8 screen's folded threshold order (screen_fold_query / screen_thr_piece, kernels_screen8_tile.h): the
query's side q1, q2, q3 in fp64 rounded to fp32 on the admitting side, then per (tile, query) three fp32 FMAs, the clamp and
floor.  Against the formula it replaced (the fp32 chain of tests/test_screen8_bound_cpu.py): no pair whose exact score reaches
the threshold is screened out, no finite threshold drops by more than one unit, and the admitted pairs rise by at most 1 %."""
import numpy as np
import pytest

from test_screen8_bound_cpu import GAMMA, int_thr, quantize_queries, quantize_tiles
from synthetic import bf16_bits, bf16_bits_to_f32

f32 = np.float32


def down(v):
    """fp64 -> fp32, never above (NaN stays NaN)."""
    f = v.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f)


def up(v):
    """fp64 -> fp32, never below (NaN stays NaN)."""
    f = v.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f)


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


def check(c_bits, q_bits, ranks, chunk=16384):
    """Every rank: no false negative of the folded order; thresholds and admitted pairs against the replaced formula."""
    x = bf16_bits_to_f32(c_bits)
    q = bf16_bits_to_f32(q_bits)
    qi, rq, eq, qn = quantize_queries(q)
    tiles = [quantize_tiles(x[r:r + chunk]) for r in range(0, x.shape[0], chunk)]
    with np.errstate(invalid="ignore", over="ignore"):
        exact = np.concatenate([x[r:r + chunk].astype(np.float64) @ q.astype(np.float64).T for r in range(0, x.shape[0], chunk)])
    # integer dot products, exact in fp64 (|x~ . q~| <= 127 * 127 * 768 < 2^53)
    I = np.concatenate([t[0].astype(np.float64) @ qi.astype(np.float64).T for t in tiles])
    tx, ty, tz = (np.concatenate([t[k] for t in tiles]) for k in (1, 2, 3))
    srt = np.sort(np.where(np.isnan(exact), -np.inf, exact), axis=0)
    counts = []
    for rank in ranks:
        thr = srt[-rank].astype(np.float32)
        athr = np.where(np.isinf(thr), 0, np.abs(thr)).astype(np.float32)
        old = int_thr(tx, ty, tz, thr, athr, rq, eq, qn)
        new = folded_thr(tx, ty, tz, *fold_query(thr, rq, eq, qn))
        must = exact >= thr.astype(np.float64) - float(GAMMA) * 1e-3
        passed_new = I >= np.repeat(new, 32, axis=0)
        passed_old = I >= np.repeat(old, 32, axis=0)
        missed = np.argwhere(must & ~passed_new)
        fin = (np.abs(old) < 2 ** 30) & (np.abs(new) < 2 ** 30)
        low = np.argwhere(fin & (new < old - 1))
        n_new, n_old = int(passed_new.sum()), int(passed_old.sum())
        d = np.abs(new - old)[fin]
        print(f"rank {rank}: admitted {n_new} (replaced formula {n_old}), max |new - old| {d.max() if d.size else 0}, "
              f"thresholds that differ {int((d != 0).sum())} of {d.size}")
        assert missed.size == 0, (rank, missed[:5].tolist())
        assert low.size == 0, (rank, low[:5].tolist())
        assert n_new <= 1.01 * n_old, (rank, n_new, n_old)
        # the same sentinels: NaN tiles / queries admit everything, an infinite threshold nothing or everything
        assert np.array_equal(new <= -2 ** 31, old <= -2 ** 31)
        counts.append(n_new)
    return counts


RANKS = (1, 10, 100, 600)


@pytest.mark.timeout(600)
def test_fold_gaussian():
    rng = np.random.default_rng(11)
    n = 32 * 4096
    c = rng.standard_normal((n, 768)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q = rng.standard_normal((64, 768)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    counts = check(bf16_bits(c), bf16_bits(q), RANKS)
    assert counts[0] < 0.2 * n * 64                      # and it does screen


@pytest.mark.timeout(600)
def test_fold_adversarial():
    # the corpus of test_screen8_bound_cpu.test_adversarial_no_false_negatives
    rng = np.random.default_rng(2)
    n = 32 * 512
    c = rng.standard_normal((n, 768)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q = rng.standard_normal((16, 768)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c[::7, 3] = 40.0
    al = np.arange(1, n, 5)
    c[al] = np.round(rng.standard_normal((al.size, 768)) * 4) / 4 + 0.05 * q[al % 16]
    c[100:164] = c[7]
    c[300:332] = 0.0
    c[400, 9] = np.nan
    c[500, 2] = np.inf
    c[600, 1] = -np.inf
    q[3, 0] = 30.0
    check(bf16_bits(c), bf16_bits(q), RANKS)


def test_fold_sentinels():
    """Infinite thresholds and non-finite tile / query scalars give the replaced formula's sentinels."""
    tx = np.array([1.0, np.nan, 3.0e3, 0.5], np.float32)
    ty = np.array([0.01, 0.01, 0.02, 0.0], np.float32)
    tz = np.array([0.002, 0.002, 0.001, 0.0], np.float32)
    thr = np.array([np.inf, -np.inf, 0.5, -0.25, 0.0], np.float32)
    rq = np.array([100.0, 100.0, np.nan, 80.0, 90.0], np.float32)
    eq = np.array([0.01, 0.01, 0.01, 0.02, 0.0], np.float32)
    qn = np.array([1.0, 1.0, 1.0, 2.0, 1.0], np.float32)
    athr = np.where(np.isinf(thr), 0, np.abs(thr)).astype(np.float32)
    old = int_thr(tx, ty, tz, thr, athr, rq, eq, qn)
    new = folded_thr(tx, ty, tz, *fold_query(thr, rq, eq, qn))
    big = (old >= 2 ** 30) | (old <= -2 ** 31)
    assert np.array_equal(new[big], old[big])
    assert np.all(np.abs(new - old)[~big] <= 1)
