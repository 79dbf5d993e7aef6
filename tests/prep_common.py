"""Reference and inputs for the bit-exact tests of row preparation (kernels_prep.h), in plain numpy.

The reference restates the rule at the top of kernels_prep.h:
    ss    = sum_i (double)x_i^2                          fp64
    norm  = (float)sqrt(ss)
    denom = fmaxf(norm, 1e-12f)                          a NaN norm gives 1e-12f
    x_n   = (float)((double)x / (double)denom)
and oracle.f32_to_bf16_bits of that for bf16 storage; a bf16 source is widened first.

Two families of rows make "bit for bit" a fair demand on a kernel whose summation order is its own:
- order-free rows: entries m * 2^e with integer |m| <= 2047 and one e per row.  Every square is an integer below 2^22
  times 2^(2e), so a sum of up to 16,384 of them is below 2^36 * 2^(2e): exact in fp64 in any order.  Rounded to bf16
  (the bf16 source) the entries keep that form with a shorter m.
- Gaussian rows: ss is taken exactly (math.fsum); any summation order is within eps = d * 2^-52 of it (relative), and a
  row is "decided" when float32(sqrt(ss (1 - eps))) == float32(sqrt(ss (1 + eps))).  Only decided rows are compared.

A row that holds a NaN is not compared beyond its NaN positions: F.normalize / oracle.l2_normalize make the whole row
NaN, the kernel's fmaxf divides the other entries by 1e-12.  Either way the row can never score.
"""
import functools
import math

import numpy as np

from oracle import oracle

EPS = np.float32(1e-12)
EXPONENTS = (-20, -7, 0, 5)
MAX_M = 2047
WIDTHS = (1, 63, 64, 65, 100, 200, 768, 1000, 1024)      # just under / at / over the 64-lane trip, ld == d and ld > d
N_FREE = 515                                             # order-free rows per width case (two allocations' worth + 3)
GAUSS_N, GAUSS_D = 4099, 768
GAUSS_SEED = {"f32": 7681, "bf16": 7682}
UNDECIDED_CAP = 0.001                                    # share of Gaussian rows that may be left out of a comparison
SNAN_BITS = 0x7F800001                                   # a NaN whose upper 16 bits alone read as +Inf


# ---- the rule --------------------------------------------------------------------------------------------------
def widen(rows: np.ndarray) -> np.ndarray:
    """Source rows as fp32 values: fp32 as given, uint16 taken as bf16 bits."""
    rows = np.asarray(rows)
    return oracle.bf16_bits_to_f32(rows) if rows.dtype == np.uint16 else np.ascontiguousarray(rows, dtype=np.float32)


def denominators(x: np.ndarray) -> np.ndarray:
    """fmaxf((float)sqrt(fp64 sum of squares), 1e-12f) per row of the fp32 matrix x."""
    out = np.empty(x.shape[0], dtype=np.float32)
    step = max(1, (1 << 22) // max(1, x.shape[1]))
    with np.errstate(over="ignore", invalid="ignore"):
        for r0 in range(0, x.shape[0], step):
            v = x[r0:r0 + step].astype(np.float64)
            out[r0:r0 + step] = np.fmax(np.sqrt(np.einsum("ij,ij->i", v, v)).astype(np.float32), EPS)
    return out


def normalize_f32(x: np.ndarray) -> np.ndarray:
    out = np.empty(x.shape, dtype=np.float32)
    denom = denominators(x).astype(np.float64)
    step = max(1, (1 << 22) // max(1, x.shape[1]))
    with np.errstate(over="ignore", invalid="ignore"):
        for r0 in range(0, x.shape[0], step):
            out[r0:r0 + step] = (x[r0:r0 + step].astype(np.float64) / denom[r0:r0 + step, None]).astype(np.float32)
    return out


def prepare(rows: np.ndarray, metric: str, storage: str) -> np.ndarray:
    """What the index stores for these source rows: fp32 values, or bf16 bits (uint16) for bf16 storage."""
    x = widen(rows)
    if metric == "cos":
        x = normalize_f32(x)
    elif metric != "ip":
        raise ValueError(metric)
    if storage == "bf16":
        return oracle.f32_to_bf16_bits(x)
    if storage != "f32":
        raise ValueError(storage)
    return x


def as_source(x: np.ndarray, src: str) -> np.ndarray:
    """fp32 rows as the source array of that dtype (bf16: the RNE bits)."""
    return oracle.f32_to_bf16_bits(x) if src == "bf16" else np.ascontiguousarray(x, dtype=np.float32)


# ---- inputs ----------------------------------------------------------------------------------------------------
def order_free_rows(n: int, d: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    m = rng.integers(-MAX_M, MAX_M + 1, size=(n, d), dtype=np.int16)
    scale = np.float32(2.0) ** rng.choice(np.int32(EXPONENTS), size=(n, 1)).astype(np.float32)
    x = m.astype(np.float32)
    x *= scale
    return x


def special_rows(d: int) -> np.ndarray:
    """The fixed block of special rows of width d.  Values sit at columns 0, d // 2 and d - 1 (the last lane's tail);
    where these coincide (d = 1, 2) the later value stands, and the reference is taken on the rows as built."""
    lo, mid, hi = 0, d // 2, d - 1
    ramp = (np.arange(d, dtype=np.float32) % 7.0) + 1.0
    rows = []
    rows.append(np.zeros(d, dtype=np.float32))                               # 0: all zero
    r = np.zeros(d, dtype=np.float32); r[hi] = 1e-30; rows.append(r)         # 1: norm below 1e-12
    rows.append(np.full(d, 3e38, dtype=np.float32))                          # 2: norm overflows to inf -> zeros
    r = ramp.copy(); r[hi] = np.inf; rows.append(r)                          # 3: +Inf and finite entries
    r = ramp.copy(); r[mid] = np.nan; rows.append(r)                         # 4: one NaN
    r = ramp.copy(); r[::2] = -0.0; rows.append(r)                           # 5: -0.0 entries
    r = np.zeros(d, dtype=np.float32); r[lo] = 1e-40; r[hi] = 2.0 ** -133; rows.append(r)        # 6: fp32 denormals only
    r = np.zeros(d, dtype=np.float32); r[lo] = 1.0; r[mid] = 1e-40; r[hi] = 2.0 ** -133; rows.append(r)   # 7: ... beside a 1.0
    r = np.zeros(d, dtype=np.float32)                                        # 8: bf16 rounding edges
    edge = np.float32([1.00390625, 1.01171875, 3.4e38, -0.0])                #    ties down / up to even, overflow, -0.0
    for i, v in enumerate(edge):
        r[(hi - i) % d] = v
    rows.append(r)
    r = ramp.copy(); r.view(np.uint32)[hi] = SNAN_BITS; rows.append(r)       # 9: a NaN that only the quiet bit keeps a NaN
    return np.stack(rows)


TIES_ROW = 8
BF16_EDGE_BITS = (0x3F80, 0x3F82, 0x7F80, 0x8000)       # stored bf16 of the edge values above, without normalisation


@functools.lru_cache(maxsize=None)
def _width_case_f32(d: int, n_free: int) -> np.ndarray:
    x = np.concatenate([order_free_rows(n_free, d, 1000 + d), special_rows(d)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def width_case(d: int, src: str, n_free: int = N_FREE) -> np.ndarray:
    """n_free order-free rows followed by the special block, as a source array of dtype `src` (read-only, shared)."""
    x = as_source(_width_case_f32(d, n_free), src)
    x.setflags(write=False)
    return x


def n_special(d: int = 8) -> int:
    return special_rows(d).shape[0]


@functools.lru_cache(maxsize=None)
def gaussian_case(src: str) -> np.ndarray:
    rng = np.random.default_rng(GAUSS_SEED[src])
    x = as_source(rng.standard_normal((GAUSS_N, GAUSS_D), dtype=np.float32), src)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def gaussian_decided(src: str) -> np.ndarray:
    """bool per row of gaussian_case(src): the fp32 norm does not depend on the summation order."""
    mask = decided_rows(widen(gaussian_case(src)))
    mask.setflags(write=False)
    return mask


def decided_rows(x: np.ndarray) -> np.ndarray:
    d = x.shape[1]
    eps = d * 2.0 ** -52
    out = np.empty(x.shape[0], dtype=bool)
    for i, row in enumerate(x.astype(np.float64)):
        ss = math.fsum((row * row).tolist())             # squares of fp32 values are exact in fp64
        out[i] = np.float32(math.sqrt(ss * (1.0 - eps))) == np.float32(math.sqrt(ss * (1.0 + eps)))
    return out


def query_rows(nq: int, d: int, seed: int) -> np.ndarray:
    """Finite queries: order-free rows, with the all-zero and the tiny-norm special at positions 1 and 2."""
    q = order_free_rows(nq, d, seed)
    if nq >= 3:
        q[1] = 0.0
        q[2] = 0.0
        q[2, d - 1] = 1e-30
    return q


# ---- comparison ------------------------------------------------------------------------------------------------
def _bits(a: np.ndarray) -> np.ndarray:
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _values(a: np.ndarray) -> np.ndarray:
    return oracle.bf16_bits_to_f32(a) if a.dtype == np.uint16 else a


def assert_prepared_equal(got: np.ndarray, want: np.ndarray, source: np.ndarray, normalized: bool, rows=None, tag=""):
    """Stored rows `got` equal the reference `want` bit for bit.  NaN positions are compared as a mask (a NaN's payload is
    not part of the rule).  Every NaN of the source must be a NaN in storage; with normalisation a row that holds one is
    not compared otherwise.  `rows`: bool mask of the rows to compare (the decided ones)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, got.dtype, want.shape, want.dtype)
    nan_in = np.isnan(widen(source))
    got_nan = np.isnan(_values(got))
    assert got_nan[nan_in].all(), f"{tag}: a NaN of the source is not a NaN in storage"
    keep = np.ones(got.shape[0], dtype=bool) if rows is None else np.asarray(rows, dtype=bool).copy()
    if normalized:
        keep &= ~nan_in.any(axis=1)
    idx = np.flatnonzero(keep)
    g, w = _bits(got)[idx], _bits(want)[idx]
    gn, wn = got_nan[idx], np.isnan(_values(want))[idx]
    bad = (gn != wn) | (~wn & (g != w))
    if bad.any():
        r, c = np.argwhere(bad)[0]
        first = ", ".join(f"[{idx[i]},{j}] got {int(g[i, j]):#x} want {int(w[i, j]):#x} source {float(widen(source)[idx[i], j])!r}"
                          for i, j in np.argwhere(bad)[:4])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.size} stored elements differ from the reference, "
                             f"in {int(bad.any(axis=1).sum())} rows; first at row {idx[r]} col {c}: {first}")
