"""A numpy / fp64 model of what the matrix path's threshold estimate must come out as, and the lattice cases the CPU and GPU
threshold tests share.  No library call: the planning half of mfma_plan / plan_levels and level_threshold, restated from
their comments and formulas (search_mfma.hip, kernels_level.h).

Why the estimate is observable: on the lattice corpora of tests/exact_common.py every score is a multiple of 2^-8, exact
in bf16 and fp32 in any summation order.  The sample's scores, their fp64 mean and sd and their k-th best are then the same
numbers in the library and here, and stats["candidates"] - the rows with score >= thr, summed over the queries of the
call - pins thr to within the gap between two lattice scores.

The plan (two-level, statistical - the default):
  T = ceil(n / 32) tiles; a corpus of T * 32 <= first_rows rows is ONE unthresholded level (every live row a candidate);
  otherwise stride = the smallest power of two >= 2 with ceil(T / stride) * 32 <= first_rows, and the sample is the rows
  32 * j * stride + r (r < 32) below n.  first_rows = 4096 below 4M rows (8192 from there on, and for the guaranteed
  chain) unless TS_MFMA_FIRST_ROWS sets it.  Masked and NaN rows are not live: they carry no score.

The threshold of one query from its live sample scores (cnt of them):
  thr = k-th best, -inf if cnt < k;
  if cnt >= 256: thr = max(thr, float32(mean + z_tail * sd)), population sd, z_tail = float32(Phi^-1(1 - min(0.25,
      stat_cands / pop))), stat_cands = min(2048, max(2 k, max(64, 6 k))), pop = allowed rows;
  if the tail fit is armed (k * n / sample_rows > 4096; tail_p = float32(min(0.25, max(2048, 8 k) / pop))), cnt >= 1024
      and the sample shows a heavy tail (x_32 > mean + (tail_z + 0.5) sd, tail_z = float32(Phi^-1(1 - min(0.25, 32 /
      sample_rows))), sample_rows = 32 * sample tiles, live or not): thr = max(thr, x_32 + e ln(ratio)) where
      e = (sum_{j=8..31} (x_j - x_32)) / 13.95928363 and ratio = (32 / cnt) / tail_p, used only when ratio > 1 and e > 0.

The guaranteed chain (TS_MFMA_STAT=0): level strides of the non-statistical plan_levels; each level's threshold is the
k-th best score of the level before it, so the full pass's is the k-th best over the second-to-last level's rows.

A query falls back to the exact scan when its candidate count is below min(k, pop) or above 8192 (the list's capacity).
"""
import functools
import math
from statistics import NormalDist

import numpy as np

TILE = 32
SORT_MAX = 8192              # rows one unthresholded level may hold = candidates one select takes
CAND_CAP = 8192              # candidate slots per query
TAIL_M = 32
TAIL_HARMONIC = np.float32(13.95928363)
F32 = np.float32


# ---- the plan ------------------------------------------------------------------------------------------------------------
def normal_tail_z(p):
    """z with P(X > z) = p for a standard normal (the library's Acklam approximation is within 1.2e-9 of it)."""
    if p <= 0.0:
        return 8.0
    if p >= 0.5:
        return 0.0
    return NormalDist().inv_cdf(1.0 - p)


def first_level_rows(n, statistical=True, first_rows=None):
    default = SORT_MAX // 2 if (statistical and n < 4_000_000) else SORT_MAX
    return min(SORT_MAX, default if first_rows is None else first_rows)


def _pow2_ratio(cands, k):
    r = 2
    while r * 2 * k <= cands:
        r *= 2
    return r


def plan_levels(n, k, statistical=True, first_rows=None):
    """[(stride, tiles)] sparsest level first; the last one is the full pass (stride 1)."""
    T = -(-n // TILE)
    first = first_level_rows(n, statistical, first_rows)
    target = min(2048, max(64, max(int(512.0 * math.sqrt(max(n, 1) / 1e7)), 8 * k)))   # candidates the full pass is planned for
    r_last, r_cap = _pow2_ratio(target, k), max(2, _pow2_ratio(1280, k))
    levels, stride = [], 1
    while True:
        nt = -(-T // stride)
        levels.append((stride, nt))
        if nt * TILE <= first:
            break
        if statistical:
            stride = 2
            while -(-T // stride) * TILE > first:
                stride *= 2
        elif len(levels) == 1:
            stride *= r_last
        else:
            need = 2
            while need < r_cap and -(-T // (stride * need)) * TILE > first:
                need *= 2
            stride *= need
    return levels[::-1]


def level_rows(n, stride, tiles):
    """Rows a level of this stride visits: 32 j stride + r, r < 32, below n (a partial last tile gives its real rows only)."""
    rows = (np.arange(tiles, dtype=np.int64)[:, None] * (TILE * stride) + np.arange(TILE)[None, :]).reshape(-1)
    return rows[rows < n]


def stat_cands(k):
    return min(2048, max(2 * k, max(64, 6 * k)))


# ---- brackets ------------------------------------------------------------------------------------------------------------
def ulps(x, steps):
    """x moved by `steps` fp32 neighbours (negative: down)."""
    x = F32(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, F32(np.inf if steps > 0 else -np.inf))
    return x


def tail_fit_halfwidth(e, log_ratio, thr_tail):
    """How far the kernel's fp32 x_32 + e * __logf(ratio) can lie from this model's fp64 value of the same expression.

    spacing: a 24-term fp32 sum of differences of lattice scores - every term and partial sum a small multiple of 2^-8,
             so the sum is exact in any order: no error.
    e:       spacing * (1.0f / 13.95928363f), one fp32 multiply by a compile-time constant; the model forms the same two
             roundings in np.float32, and is charged one more rounding of e anyway: 2^-24 e |L|.
    ratio:   two fp32 divisions of values the model also holds in fp32; charged 2 ulps (divisions need not be correctly
             rounded on the device): |d ratio / ratio| <= 2^-22, that is |dL| <= 2^-22.
    __logf:  the fast logarithm, v_log_f32 times ln 2; the documented bound of the intrinsic is an absolute error of
             2^-21.41 for arguments in [0.5, 2] and 3 ulps (3 * 2^-23 |L|) elsewhere; the larger of the two is charged.
    fma:     e * L + x_32, fused or not: one rounding of the product (2^-24 e |L|) and one of the sum (half an ulp of thr).
    Sum: e (2^-22 + max(2^-21.41, 3 * 2^-23 |L|)) + 2 * 2^-24 e |L| + ulp(thr) / 2.  The caller adds the two ulps every
    estimate gets for the cast and the quantile's 1.2e-9."""
    L = abs(float(log_ratio))
    d_log = 2.0 ** -22 + max(2.0 ** -21.41, 3.0 * 2.0 ** -23 * L)
    half_ulp = 0.5 * float(np.spacing(F32(abs(thr_tail))))
    return float(e) * d_log + 2.0 * 2.0 ** -24 * float(e) * L + half_ulp


# ---- the threshold of one query ----------------------------------------------------------------------------------------------
class Thr:
    """lo <= the library's threshold <= hi; `term` names the estimate that sets it ('kth', 'gauss', 'tail', 'none')."""
    __slots__ = ("lo", "hi", "mid", "term", "kth", "gauss", "tail", "mean", "sd", "cnt", "heavy_margin")


def sample_threshold(scores, k, z_tail, tail_p=0.0, tail_z=0.0):
    """`scores`: the live sample scores of one query (fp32-exact values, any order).  z_tail / tail_p / tail_z as the host
    passes them (fp32 values; 0 = that estimate is off)."""
    s = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    cnt = s.size
    r = Thr()
    r.cnt = cnt
    r.kth = float(s[k - 1]) if cnt >= k else -np.inf
    r.mean = float(s.sum() / cnt) if cnt else 0.0
    r.sd = math.sqrt(max(float((s * s).sum() / cnt) - r.mean * r.mean, 0.0)) if cnt else 0.0
    r.gauss = r.tail = -np.inf
    r.heavy_margin = None
    lo = hi = mid = r.kth
    r.term = "kth" if cnt >= k else "none"
    if z_tail > 0.0 and cnt >= 256:
        g = r.mean + float(F32(z_tail)) * r.sd
        r.gauss = float(F32(g))
        # sd = 0 (every live sample score the same lattice value): sum / cnt and sum of squares / cnt are exact, the
        # estimate is that score itself in the library as here - nothing was rounded, nothing to bracket
        g_lo, g_hi = (r.gauss, r.gauss) if r.sd == 0.0 else (float(ulps(g, -2)), float(ulps(g, 2)))
        if r.gauss > mid:
            r.term = "gauss"
        lo, hi, mid = max(lo, g_lo), max(hi, g_hi), max(mid, r.gauss)
        if tail_p > 0.0 and cnt >= 1024:                       # (cnt >= 1024 > 32: the 32 best exist)
            x_m = s[TAIL_M - 1]
            spacing = F32((s[7:TAIL_M - 1] - x_m).sum())       # order statistics 8 .. 31 (1-based) against the 32nd: exact
            e = spacing * (F32(1.0) / TAIL_HARMONIC)
            ratio = (F32(TAIL_M) / F32(cnt)) / F32(tail_p)
            r.heavy_margin = float(x_m - (r.mean + (float(F32(tail_z)) + 0.5) * r.sd))
            if ratio > 1.0 and e > 0.0 and r.heavy_margin > 0.0:
                L = math.log(float(ratio))
                t = float(x_m) + float(e) * L
                r.tail = t
                w = tail_fit_halfwidth(e, L, t)
                t_lo, t_hi = float(ulps(t - w, -2)), float(ulps(t + w, 2))
                if t > mid:
                    r.term = "tail"
                lo, hi, mid = max(lo, t_lo), max(hi, t_hi), max(mid, float(F32(t)))
    r.lo, r.hi, r.mid = lo, hi, mid
    return r


# ---- a whole search ------------------------------------------------------------------------------------------------------
class Model:
    """What one search must report: per query the bracketed candidate count and whether it falls back."""

    def __init__(self, levels, thr, count_lo, count_hi, min_fill):
        self.levels = levels
        self.thr = thr                                          # [nq] Thr (None for a single level)
        self.count_lo, self.count_hi = count_lo, count_hi      # [nq] candidates at thr.hi / at thr.lo
        self.min_fill = min_fill

    @property
    def undecided(self):
        return self.count_lo != self.count_hi

    def _fb(self, c):
        return (c < self.min_fill) | (c > CAND_CAP)

    def sums(self, sl=slice(None)):
        """(lower, upper) bounds of stats["candidates"] for the queries `sl`."""
        return int(self.count_lo[sl].sum()), int(self.count_hi[sl].sum())

    def fallbacks(self, sl=slice(None)):
        """(fewest, most) queries of `sl` that fall back: equal unless an undecided query sits at a fill limit."""
        a, b = self._fb(self.count_lo[sl]), self._fb(self.count_hi[sl])
        return int((a & b).sum()), int((a | b).sum())

    def under_filled(self):
        return self.count_lo < self.min_fill

    def terms(self):
        return [t.term for t in self.thr] if self.thr is not None else []


def expected_candidates(t, thr, live):
    """Per query: live rows with t >= thr (thr: [nq])."""
    return ((t >= np.asarray(thr, dtype=np.float64)[:, None]) & live[None, :]).sum(axis=1)


def model_search(t, k, allowed=None, statistical=True, first_rows=None, tail_fit=True):
    """t: [nq x n] exact scores (NaN = a NaN row).  allowed: the host mask (bool per row) or None."""
    nq, n = t.shape
    live = ~np.isnan(t[0]) if allowed is None else (allowed & ~np.isnan(t[0]))
    pop = n if allowed is None else int(allowed.sum())
    min_fill = min(k, pop)
    levels = plan_levels(n, k, statistical, first_rows)
    tt = np.where(np.isnan(t), -np.inf, t)
    if len(levels) == 1:
        c = np.full(nq, int(live.sum()), dtype=np.int64)
        return Model(levels, None, c, c.copy(), min_fill)
    thr = []
    if statistical:
        stride, tiles = levels[0]
        rows = level_rows(n, stride, tiles)
        rows = rows[live[rows]]
        sample_rows = tiles * TILE
        z_tail = F32(normal_tail_z(min(0.25, stat_cands(k) / max(pop, 1))))
        armed = tail_fit and z_tail > 0 and k * n / sample_rows > 0.5 * CAND_CAP
        tail_p = F32(min(0.25, max(2048, 8 * k) / max(pop, 1))) if armed else F32(0)
        tail_z = F32(normal_tail_z(min(0.25, 32.0 / sample_rows)))
        for b in range(nq):
            thr.append(sample_threshold(tt[b, rows], k, z_tail, tail_p, tail_z))
    else:
        # every level's threshold: the k-th best of the level before it among the rows at or above THAT level's threshold -
        # the same as the k-th best of all its live rows, because the strides nest (a level holds the rows of the one before)
        stride, tiles = levels[-2]
        rows = level_rows(n, stride, tiles)
        rows = rows[live[rows]]
        for b in range(nq):
            thr.append(sample_threshold(tt[b, rows], k, 0.0))
    lo = expected_candidates(tt, [x.hi for x in thr], live)
    hi = expected_candidates(tt, [x.lo for x in thr], live)
    return Model(levels, thr, lo, hi, min_fill)


def closest_lattice_gap(model, step=2.0 ** -8):
    """Smallest distance of an estimated (not k-th best) threshold to a lattice score: how much room the bracket has."""
    d = [abs(x.mid / step - round(x.mid / step)) * step for x in model.thr if x.term in ("gauss", "tail")]
    return min(d) if d else None


# ---- the cases -----------------------------------------------------------------------------------------------------------
NQ = 82                                       # 1 + 17 + 64: the whole batch, then three sub-batches
SUBS = (slice(0, 1), slice(1, 18), slice(18, 82))
# behind a host mask the matrix path takes batches only (more queries than the scan serves faster: 4, or 1 at k > 64; a
# single masked query is the scan's by rule and asking for the matrix path is an error): 5, 17 and 60 queries there
SUBS_MASKED = (slice(0, 5), slice(5, 22), slice(22, 82))


def lattice(n, d, nq, seed):
    """(queries, rows) with entries in {-2..2} / 16."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-2, 3, size=(n, d)).astype(np.float32) * F32(1 / 16)
    q = rng.integers(-2, 3, size=(nq, d)).astype(np.float32) * F32(1 / 16)
    return q, c


def clustered(n, d, nq, seed):
    """A heavy-tailed lattice corpus: 5 % of the rows lean towards a direction u that every query shares, by a geometric
    number of steps, so the scores of one query over the corpus have a tail far heavier than a Gaussian's.  Entries stay
    multiples of 1/16 below 1/2 in magnitude: exact in bf16, products multiples of 2^-8."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    u = np.zeros(d, dtype=np.float32)
    u[rng.choice(d, 32, replace=False)] = rng.choice(np.float32([-1, 1]), 32)
    members = rng.choice(n, n // 20, replace=False)
    steps = np.minimum(rng.geometric(0.5, members.size), 4).astype(np.float32)
    c[members] += steps[:, None] * u[None, :]
    q = rng.integers(-1, 2, size=(nq, d)).astype(np.float32) + 2 * u[None, :]
    return q * F32(1 / 16), c * F32(1 / 16)


def all_equal(n, d, nq, seed):
    q, c = lattice(1, d, nq, seed)
    return q, np.tile(c, (n, 1))


def two_valued(n, d, nq, seed, high_rows):
    """Rows are `one` (the rows listed) or `other`: two scores per query."""
    q, c = lattice(2, d, nq, seed)
    rows = np.tile(c[1], (n, 1))
    rows[high_rows] = c[0]
    return q, rows


def pile_rows(n, stride, in_sample, outside, seed):
    """`in_sample` rows of the stride's sample and `outside` rows that no sample tile holds."""
    rng = np.random.default_rng(seed)
    sampled = np.zeros(n, dtype=bool)
    tiles = -(-n // TILE)
    sampled[level_rows(n, stride, -(-tiles // stride))] = True
    return np.sort(np.concatenate([rng.choice(np.flatnonzero(sampled), in_sample, replace=False),
                                   rng.choice(np.flatnonzero(~sampled), outside, replace=False)]))


class Case:
    """One index + one search of the GPU test, and everything the model needs to predict it."""

    def __init__(self, name, dtype, n, d, k, seed, levels, corpus="lattice", options=None, mask=None, statistical=True,
                 first_rows=None, tail_fit=True, may_underfill=False, want_terms=("gauss", "kth"), tail_case=False):
        self.name, self.dtype, self.n, self.d, self.k, self.seed, self.levels = name, dtype, n, d, k, seed, levels
        self.corpus, self.options, self.mask_kind = corpus, dict(options or {}), mask
        self.statistical, self.first_rows, self.tail_fit = statistical, first_rows, tail_fit
        self.may_underfill, self.want_terms, self.tail_case = may_underfill, want_terms, tail_case

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=4)
def corpus_of(kind, n, d, seed):
    if kind == "lattice":
        q, c = lattice(n, d, NQ, seed)
    elif kind == "clustered":
        q, c = clustered(n, d, NQ, seed)
    elif kind == "equal":
        q, c = all_equal(n, d, NQ, seed)
    elif kind == "two_sparse":                  # 5 % high: the k-th best (the pile's score) is the threshold where the pile is on top
        q, c = two_valued(n, d, NQ, seed, np.random.default_rng(seed).choice(n, n // 20, replace=False))
    elif kind == "two_pile":                    # 1,030 of the sample's 4,000 rows and 3,000 others: more than the sample select sorts
        q, c = two_valued(n, d, NQ, seed, pile_rows(n, 8, 1030, 3000, seed))
    else:
        raise ValueError(kind)
    t = (q.astype(np.float64) @ c.astype(np.float64).T) + 0.0
    q.setflags(write=False)
    c.setflags(write=False)
    t.setflags(write=False)
    return q, c, t


def mask_of(case):
    if case.mask_kind is None:
        return None
    rng = np.random.default_rng(case.seed + 7)
    if case.mask_kind == "half":
        return rng.random(case.n) < 0.5
    if case.mask_kind == "starved":
        # 2,100 rows (more than a tenth: the matrix path serves the mask), of which the sample holds 100: fewer than k = 256
        stride, tiles = plan_levels(case.n, case.k)[0]
        sampled = np.zeros(case.n, dtype=bool)
        sampled[level_rows(case.n, stride, tiles)] = True
        m = np.zeros(case.n, dtype=bool)
        m[rng.choice(np.flatnonzero(sampled), 100, replace=False)] = True
        m[rng.choice(np.flatnonzero(~sampled), 2000, replace=False)] = True
        return m
    raise ValueError(case.mask_kind)


@functools.lru_cache(maxsize=4)
def _model_cached(case):
    q, c, t = corpus_of(case.corpus, case.n, case.d, case.seed)
    return model_search(t, case.k, mask_of(case), case.statistical, case.first_rows, case.tail_fit)


def model_of(case):
    return _model_cached(case)


def _cases():
    C = Case
    both, g, kth = ("gauss", "kth"), ("gauss",), ("kth",)
    out = [C(f"anyd-bf16-d128-k{k}", "bf16", 20_011, 128, k, 11, 2, want_terms=w)
           for k, w in ((1, kth), (10, both), (64, both), (65, both), (256, g))]
    out += [
        C("anyd-bf16-d192", "bf16", 40_000, 192, 10, 12, 2, want_terms=g),
        C("anyd-f32-d192", "f32", 40_000, 192, 10, 12, 2, want_terms=g),
        C("mfma16-bf16-d384-k10", "bf16", 20_011, 384, 10, 13, 2),
        C("mfma16-bf16-d384-k65", "bf16", 20_011, 384, 65, 13, 2, want_terms=g),
        C("screen-bf16-d768", "bf16", 20_011, 768, 10, 14, 2),
        C("noscreen-bf16-d768", "bf16", 20_011, 768, 10, 14, 2, options={"TS_MFMA_SCREEN": 0}),
        C("listform-bf16-d768", "bf16", 20_011, 768, 10, 14, 2, options={"TS_MFMA_SAMPLE": 0}),
        C("chain-bf16-d768", "bf16", 20_011, 768, 10, 14, 2, options={"TS_MFMA_STAT": 0}, statistical=False, want_terms=kth),
        C("chain3-bf16-d384", "bf16", 70_001, 384, 10, 15, 3, options={"TS_MFMA_STAT": 0}, statistical=False, want_terms=kth),
        C("mfma16-f32-d768", "f32", 20_011, 768, 10, 14, 2),
        C("armed-bf16-d128-k256", "bf16", 70_001, 128, 256, 16, 2, want_terms=g),
        C("clustered-bf16-d128", "bf16", 200_001, 128, 64, 17, 2, corpus="clustered", options={"TS_MFMA_FIRST_ROWS": 2048},
          first_rows=2048, want_terms=("tail",), tail_case=True),
        C("clustered-nofit-bf16-d128", "bf16", 200_001, 128, 64, 17, 2, corpus="clustered",
          options={"TS_MFMA_FIRST_ROWS": 2048, "TS_MFMA_TAIL_FIT": 0}, first_rows=2048, tail_fit=False, want_terms=g),
        C("mask-half-bf16-d128", "bf16", 20_011, 128, 10, 11, 2, mask="half"),
        C("mask-starved-bf16-d128", "bf16", 20_011, 128, 256, 11, 2, mask="starved", want_terms=("none",)),
        C("equal-bf16-d128", "bf16", 20_011, 128, 10, 18, 2, corpus="equal", want_terms=kth),
        C("two-sparse-bf16-d128", "bf16", 20_011, 128, 10, 19, 2, corpus="two_sparse", may_underfill=True),
        C("two-pile-bf16-d128", "bf16", 32_000, 128, 256, 20, 2, corpus="two_pile", may_underfill=True),
    ]
    return out


CASES = _cases()
