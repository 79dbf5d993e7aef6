"""A numpy mirror of the int8 screen's quantiser and integer threshold (kernels_screen8.h; screen_fold_query / screen_thr_piece in kernels_screen8_tile.h):
no pair whose exact score reaches the threshold is screened out, on Gaussian and adversarial rows, with the fp32 steps of the
threshold computed in fp32 as the kernel computes them."""
import numpy as np

from synthetic import bf16_bits, bf16_bits_to_f32

D = 768
GAMMA = np.float32(768.0 * 2.0 ** -22)
f32 = np.float32


def up(v):
    """fp64 -> fp32, never below (f32_up)."""
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) >= v, f, np.nextafter(f, np.float32(np.inf)))


def quantize_tiles(x):
    """x: [n x 768] fp32 values of bf16 rows, n a multiple of 32 -> int8 rows, per tile (1 / s_t, E_t, X_t)."""
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
    fin = np.isfinite(q)
    amax = np.where(fin, np.abs(q), 0).max(axis=1).astype(np.float32)
    s = np.where(amax > 0, amax / f32(127), f32(1)).astype(np.float32)
    qx = np.where(fin, np.clip(np.rint(q / s[:, None]), -127, 127), 0).astype(np.float32)
    e = q.astype(np.float64) - s[:, None].astype(np.float64) * qx
    bad = ~fin.all(axis=1)
    rq = np.where(bad, np.float32(np.nan), f32(1) / s).astype(np.float32)
    return qx.astype(np.int8), rq, up(np.sqrt((e * e).sum(axis=1)) * (1 + 2.0 ** -40)), up(np.sqrt((q.astype(np.float64) ** 2).sum(axis=1)) * (1 + 2.0 ** -40))


def int_thr(tx, ty, tz, thr, athr, rq, eq, qn):
    """screen_fold_query + screen_thr_piece in fp32: [tiles] x [queries]."""
    with np.errstate(invalid="ignore", over="ignore"):
        sub = (ty[:, None] * qn[None, :] + tz[:, None] * eq[None, :]).astype(np.float32)
        mag = (athr[None, :] + sub).astype(np.float32)
        v = ((thr[None, :] - sub - mag * f32(2.0 ** -18)) * tx[:, None] * rq[None, :]).astype(np.float32)
        w = np.fmin(np.fmax(v - f32(1), f32(-2.0 ** 31)), f32(2.0 ** 30))
    return np.floor(w).astype(np.int64)


def check(c_bits, q_bits, rank):
    x = bf16_bits_to_f32(c_bits)
    q = bf16_bits_to_f32(q_bits)
    xi, tx, ty, tz = quantize_tiles(x)
    qi, rq, eq, qn = quantize_queries(q)
    with np.errstate(invalid="ignore", over="ignore"):
        exact = x.astype(np.float64) @ q.astype(np.float64).T                      # [n x nq]
    srt = np.sort(np.where(np.isnan(exact), -np.inf, exact), axis=0)
    thr = srt[-rank].astype(np.float32)                                             # a threshold near the answers
    athr = np.where(np.isinf(thr), 0, np.abs(thr)).astype(np.float32)
    T = int_thr(tx, ty, tz, thr, athr, rq, eq, qn)                                  # [tiles x nq]
    I = xi.astype(np.int64) @ qi.astype(np.int64).T                                  # exact integer dot products
    must = exact >= thr.astype(np.float64) - float(GAMMA) * 1e-3                   # rows the fp32 score could pass with
    passed = I >= np.repeat(T, 32, axis=0)
    missed = np.argwhere(must & ~passed)
    assert missed.size == 0, missed[:5].tolist()
    return passed.sum(axis=0)


def test_gaussian_no_false_negatives():
    rng = np.random.default_rng(1)
    c = rng.standard_normal((32 * 1024, D)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q = rng.standard_normal((16, D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    passed = check(bf16_bits(c), bf16_bits(q), 10)
    assert passed.mean() < 0.2 * c.shape[0]          # and it does screen


def test_adversarial_no_false_negatives():
    rng = np.random.default_rng(2)
    n = 32 * 512
    c = rng.standard_normal((n, D)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    q = rng.standard_normal((16, D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c[::7, 3] = 40.0                                                   # one huge element: a coarse tile scale
    al = np.arange(1, n, 5)
    c[al] = np.round(rng.standard_normal((al.size, D)) * 4) / 4 + 0.05 * q[al % 16]   # e_x along a query
    c[100:164] = c[7]                                                  # duplicates across tiles
    c[300:332] = 0.0                                                   # a zero tile
    c[400, 9] = np.nan
    c[500, 2] = np.inf
    c[600, 1] = -np.inf
    q[3, 0] = 30.0                                                     # a query with a coarse scale
    for rank in (1, 10, 100):
        check(bf16_bits(c), bf16_bits(q), rank)
