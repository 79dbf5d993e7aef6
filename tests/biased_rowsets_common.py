"""Helpers of tests/test_biased_rowsets_gpu.py, the tests of the citation-weighted search with a weight and a row set per query
(ts_search_biased_rowsets): the exact bias of the lattice cases, the numpy reference of a weighted top k, the oracle check of
tests/test_biased_mfma_gpu.py restated per query, the routing of biased_rowsets_plan.h restated from the issue's rules, and the CPU
model of the threshold estimate (model() of tests/test_bias_plan_cpu.py) with a weight and a mask per query."""
import functools

import numpy as np

import rowsets_common as R
from oracle import oracle

BINS = 1024
BISECTIONS = 26
CAND_CAP = 8192               # candidate slots per query (host.h: kCandCap)
LATTICE_WEIGHTS = (0.0, 0.25, 0.5, 1.0, -0.5)


def lattice_bias(n, seed=17):
    """fp32 bias on multiples of 2^-4 in [0, 8], about 10 % zeros, a dozen rows at 8: with the lattice rows of exact_common
    (scores are multiples of 2^-8) and weights from LATTICE_WEIGHTS every weighted score is exact in fp32 in any order."""
    rng = np.random.default_rng(seed)
    b = rng.integers(1, 8 * 16, n).astype(np.float32) / np.float32(16)
    b[rng.random(n) < 0.1] = 0.0
    b[rng.choice(n, 12, replace=False)] = 8.0
    return b


def classes(nq, nsets, weights, seed, with_unfiltered=True):
    """(which, w): every (set, weight) combination named at least once where nq allows, the rest at random."""
    rng = np.random.default_rng(seed)
    names = list(range(nsets)) + ([-1] if with_unfiltered else [])
    combos = [(s, w) for s in names for w in weights][:nq]
    extra = [(names[a], weights[b]) for a, b in zip(rng.integers(0, len(names), nq - len(combos)), rng.integers(0, len(weights), nq - len(combos)))]
    picked = [(combos + extra)[i] for i in rng.permutation(nq)]
    return np.array([p[0] for p in picked], dtype=np.int32), np.array([p[1] for p in picked], dtype=np.float32)


def weighted_ref(t_row, bias, w, k, allowed=None):
    """(weighted f32 [k], similarities f32 [k], ids [k]) of the exact weighted top k of one query on exact data: weighted
    score descending, row ascending, allowed rows only, padded with (-inf, -inf, -1)."""
    weighted = t_row + float(w) * bias.astype(np.float64)
    rows = np.arange(t_row.shape[0]) if allowed is None else np.flatnonzero(allowed)
    top = rows[np.lexsort((rows, -weighted[rows]))][:k]
    ws, sims, ids = np.full(k, -np.inf, np.float32), np.full(k, -np.inf, np.float32), np.full(k, -1, np.int64)
    ws[: top.size], sims[: top.size], ids[: top.size] = weighted[top], t_row[top], top
    return ws, sims, ids


# ---- the oracle check of tests/test_biased_mfma_gpu.py, one query with its weight and its allowed rows -------------------------
def weighted_topk(sim, bonus, w, k, allowed=None):
    """oracle.citation_weighted_rerank over the whole row (weighted DESC, similarity DESC, row ASC), from the best 4 k + 64."""
    weighted = sim + w * bonus
    rows = np.arange(sim.shape[0]) if allowed is None else allowed
    m = min(rows.shape[0], 4 * k + 64)
    top = rows[np.argpartition(-weighted[rows], m - 1)[:m]] if m < rows.shape[0] else rows
    order = top[np.lexsort((top, -sim[top], -weighted[top]))][:k]
    return order, sim[order], weighted[order]


def check_weighted_query(sim_row, cites, bias, w, k, ws, sims, idx, allowed=None, against_oracle=False):
    """Pinned ranks (fp64 gap > 1e-6 on both sides) exact, nothing worse than the k-th best, weighted scores and similarities
    within 1e-5 - the tolerances of check_weighted there.  allowed: row numbers, or None."""
    bonus = bias.astype(np.float64)
    w = float(w)
    want_i, want_sim, want_w = weighted_topk(sim_row, bonus, w, k, allowed)
    if against_oracle:                       # the helper is the oracle's restatement
        o_i, o_sim, o_w = oracle.citation_weighted_rerank(np.arange(sim_row.shape[0]), sim_row, cites, w, k)
        assert np.array_equal(o_i, want_i) and np.allclose(o_w, want_w, atol=1e-12)
    got_w = (sim_row + w * bonus)[idx]
    gaps = want_w[:-1] - want_w[1:]
    for r in range(k):
        lo = gaps[r - 1] if r else np.inf
        hi = gaps[r] if r < k - 1 else np.inf
        if lo > 1e-6 and hi > 1e-6 and r < k - 1:
            assert idx[r] == want_i[r], r
    assert np.all(got_w >= want_w[-1] - 1e-6)
    assert np.allclose(ws, want_w, atol=1e-5) and np.allclose(sims, sim_row[idx], atol=1e-5)


# ---- the routing of biased_rowsets_plan.h under `auto`, for an index the pass serves ------------------------------------------
def route(n, allowed, which, weights, k, scan_max, min_classes=2):
    """(pass queries, {(set, weight): queries of its per-class call}, calls).  allowed[s]: rows set s allows."""
    which, weights = np.asarray(which), np.asarray(weights, dtype=np.float32)
    cls = [(int(s), float(w) + 0.0) for s, w in zip(which, weights)]          # + 0.0: -0 and 0 are one class
    pop = np.array([n if s < 0 else allowed[s] for s in which])
    dense = pop * 10 >= n
    limit = 1 if k > 64 else scan_max
    rides = dense if (dense.sum() > limit and len({c for c, dn in zip(cls, dense) if dn}) >= min_classes) else np.zeros(len(which), dtype=bool)
    if len(set(cls)) == 1:
        rides = np.zeros(len(which), dtype=bool)                               # delegated: no pass
    groups = {}
    for i, c in enumerate(cls):
        if not rides[i]:
            groups.setdefault(c, []).append(i)
    calls = sum(1 for s, _ in groups if s < 0 or allowed[s] > 0)
    return np.flatnonzero(rides), groups, calls


# ---- the CPU model of the estimate: model() of tests/test_bias_plan_cpu.py with a weight and a mask per query ---------------
def sample_rows(n):
    """search_mfma.hip, plan_levels under the default two-level search: every stride-th 32-row tile, stride the smallest power
    of two that leaves at most 4,096 sample rows (n < 4M)."""
    tiles = (n + 31) // 32
    stride = 2
    while ((tiles + stride - 1) // stride) * 32 > 4096:
        stride *= 2
    rows = (np.arange((tiles + stride - 1) // stride)[:, None] * stride * 32 + np.arange(32)[None, :]).ravel()
    return rows[rows < n]


def _normal_tail(x):
    import torch
    return 0.5 * torch.special.erfc(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)) * 0.70710678118654752440).numpy()


def term_edges(lo, hi, w):
    """The upper edge of a bin's term w * bias (biased_rowsets_plan.h: biased_rowsets_term_edge), all bins."""
    width = np.float32((np.float32(hi) - np.float32(lo)) / np.float32(BINS)) if hi > lo else np.float32(0)
    b = np.arange(BINS, dtype=np.float64)
    if w >= 0:
        return float(w) * np.minimum(float(lo) + (b + 1) * float(width), float(hi))
    return float(w) * (float(lo) + b * float(width))


def solve_threshold(hist, lo, hi, w, mu, sigma, target):
    """biased_rowsets_solve_threshold restated: bisection of E(t) = target on the raw histogram read through w."""
    if not (sigma > 0.0) or not (hi >= lo):
        return -np.inf
    nz = np.flatnonzero(hist)
    edges, cnt = term_edges(lo, hi, w)[nz], hist[nz].astype(np.float64)
    expected = lambda t: float((cnt * _normal_tail((t - edges - mu) / sigma)).sum())
    e0, e1 = float(w) * float(lo), float(w) * float(hi)
    a, b = mu + min(e0, e1) - 9.0 * sigma, mu + max(e0, e1) + 9.0 * sigma
    if expected(a) < target:
        return -np.inf
    for _ in range(BISECTIONS):
        mid = 0.5 * (a + b)
        if expected(mid) >= target:
            a = mid
        else:
            b = mid
    return float(np.float32(a))


def raw_histograms(bias, masks):
    """{set: counts} of the raw finite bias per set (-1: every row), the range (lo, hi) over all rows."""
    finite = np.isfinite(bias)
    lo, hi = bias[finite].min(), bias[finite].max()
    width = np.float32((hi - lo) / np.float32(BINS)) if hi > lo else np.float32(0)
    bins = np.zeros(bias.shape[0], np.int64) if width == 0 else np.clip(((np.where(finite, bias, lo) - lo) / width).astype(np.int64), 0, BINS - 1)
    hists = {-1: np.bincount(bins[finite], minlength=BINS)}
    for s, m in enumerate(masks):
        hists[s] = np.bincount(bins[finite & m], minlength=BINS)
    return hists, lo, hi


def model_candidates(sims, bias, k, masks, which, weights, slack=1e-4):
    """Per query (fewest, most) candidates the full pass admits under thr = max(k-th best weighted sample score, estimate),
    the threshold moved by +- slack (the pass's and the sample's fp32 scores against the fp64 ones here).  sims: [nq x n]
    fp64 scores of the stored values."""
    n = bias.shape[0]
    hists, lo, hi = raw_histograms(bias, masks)
    rows_all = sample_rows(n)
    target = max(64, 6 * k)
    few, most = [], []
    for i, (s, w) in enumerate(zip(which, weights)):
        allowed = np.ones(n, dtype=bool) if s < 0 else masks[s]
        rows = rows_all[allowed[rows_all]]
        term = (np.float32(w) * bias).astype(np.float64)
        weighted = np.where(allowed, sims[i] + term, -np.inf)
        raw = sims[i, rows]
        sw = np.sort(weighted[rows])[::-1]
        bound = sw[k - 1] if sw.size >= k else -np.inf
        est = solve_threshold(hists[int(s)], lo, hi, float(w), raw.mean(), raw.std(), target) if rows.size >= 256 else -np.inf
        thr = max(bound, est)
        few.append(int((weighted >= thr + slack).sum()))
        most.append(int((weighted >= thr - slack).sum()))
    return np.array(few), np.array(most)


def model_fallbacks(q, c, dtype, k, bias, masks, which, weights):
    """How many queries the model sends to the exact re-run: (fewest, most) - a query re-runs with fewer candidates than
    min(k, its rows) or more than the buffer holds."""
    sims = R.stored(q, dtype).astype(np.float64) @ R.stored(c, dtype).astype(np.float64).T
    few, most = model_candidates(sims, bias, k, masks, which, weights)
    pop = np.array([bias.shape[0] if s < 0 else int(masks[s].sum()) for s in which])
    fill = np.minimum(k, pop)
    sure = (most < fill) | (few > CAND_CAP)
    maybe = (few < fill) | (most > CAND_CAP)
    return int(sure.sum()), int(maybe.sum())


@functools.lru_cache(maxsize=2)
def recipe(n):
    """Citation counts of tests/test_biased_mfma_gpu.py: None / 0 / 1..399, twelve rows at 1e6..1e8 - and their bias."""
    from theoremsearch_amd import pgvector
    rng = np.random.default_rng(9)
    cites = [None if u < 0.1 else (0 if u < 0.2 else int(v)) for u, v in zip(rng.random(n), rng.integers(1, 400, n))]
    for r in rng.choice(n, 12, replace=False):
        cites[int(r)] = int(10 ** rng.integers(6, 9))
    return cites, pgvector.citation_bias(cites)
