"""Every regime of the matrix path's final select (level_select_kernel in kernels_level.h, lds_select_top in
kernels_select.h), entered on purpose.

A corpus that fits the first level (n <= 4096 rows, or 8192 with TS_MFMA_FIRST_ROWS=8192) runs as ONE unthresholded level:
every live row is a candidate, so the select sees exactly n_live keys and n picks the regime -
  n <= 128 and k <= 128, no private lists   the one-wave path (kFinalFast)
  n <= 2048                                 the direct sort (kLevelSmall)
  2049 .. 8192                              the 1024-bin histogram cut, then the sort of the bins above the cut
  ... with more than 2048 keys in the cut bin   the streaming WaveTopK<1> (k <= 64) / <4> path
and the kernel picks the lists: the general-width bf16 pass appends to the shared list only, the 16x16 pass stages lists
that overflow into the direct append (every score is a candidate), TS_MFMA_SHAPE=32 writes private lists of 32 plus spill
(the gather loop), fp32 at d = 384 is the 16x16x4 form.  Every search asserts algo == 2, levels == 1, no re-run, and
candidates == queries * n_live - which proves the regime - and compares scores and ids bit for bit with the canonical
order (score descending, row ascending).  (The counters describe the last launch block of a call: 256 queries are one block
everywhere except fp32 at d = 384, where a block is 128.)

Scores are designed, on the lattice: row r carries an integer D[r] in [-2048, 2047] in two columns that the "pure" queries
read with weight +1, -1 (the same scores in the opposite order) or +2, so a family is a choice of D; the other queries
add, or are only, a random lattice part.  k > n pads with (-inf, -1).

The product n x k x nq is pruned to the pairs that change regime:
  n:  1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4096, 4097, 8191, 8192 all run on the general-width kernel with
      the staircase family; the other kernels and families take the sizes next to a regime edge they can reach (lists
      below);
  k:  all of 1, 10, 64, 65, 128, 129, 256 with 17 queries (k <= 64 / > 64 switches WaveTopK<1> / <4>, k <= 128 / > 128 the
      one-wave path, k > n the padding);
  nq: 1 and 256 with k = 10 and 129 only - the select is one workgroup per query, the batch size changes the pass and the
      list layout, not the regime."""
import functools

import numpy as np
import pytest

import exact_common as E
import threshold_common as M

pytestmark = pytest.mark.gpu

NQ = 256
KS = (1, 10, 64, 65, 128, 129, 256)
ALL_N = (1, 2, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4096, 4097, 8191, 8192)
EDGE_N = (1, 65, 128, 129, 2048, 2049, 4097, 8192)
KERNELS = {                                   # name: (dtype, d, options, queries of a launch block at 256 queries)
    "anyd-bf16": ("bf16", 128, {}, 256),
    "mfma16-bf16": ("bf16", 384, {}, 256),
    "mfma32-bf16": ("bf16", 384, {"TS_MFMA_SHAPE": 32}, 256),
    "mfma16-f32": ("f32", 384, {}, 128),
}


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


# ---- designed scores -----------------------------------------------------------------------------------------------------
def designed(D, d, seed, flat=False):
    """(queries, rows): row r scores w * D[r] / 256 for the pure queries (b % 4 == 0: w = +1, 1: w = -1), that plus a random
    lattice part for b % 4 == 2 (w = +2), the random part alone for b % 4 == 3.  `flat`: no random part in the rows."""
    D = np.asarray(D, dtype=np.int64)
    assert D.min() >= -2048 and D.max() <= 2047
    rng = np.random.default_rng(seed)
    n = D.size
    c = np.zeros((n, d), dtype=np.float32)
    if not flat:
        c[:, 16:] = rng.integers(-2, 3, size=(n, d - 16)).astype(np.float32) / np.float32(16)
    c[:, 0] = (D % 16).astype(np.float32) / np.float32(16)
    c[:, 1] = (D // 16).astype(np.float32) / np.float32(16)
    q = np.zeros((NQ, d), dtype=np.float32)
    kind = np.arange(NQ) % 4
    w = np.float32([1, -1, 2, 0])[kind]
    q[:, 0] = w / np.float32(16)
    q[:, 1] = w
    noisy = kind >= 2
    q[noisy, 16:] = rng.integers(-2, 3, size=(int(noisy.sum()), d - 16)).astype(np.float32) / np.float32(16)
    return q, c


def family(name, n, d, seed):
    rng = np.random.default_rng(seed)
    if name == "staircase":                   # increasing with the row (two and more rows per step from 4097 rows on); w = -1: decreasing
        return designed(np.arange(n) * 4096 // max(n, 4096) - 2048, d, seed)
    if name == "equal":                       # every row the same: sd = 0, every key in bin 0, more than 2048 of them stream
        q, c = designed(np.full(n, 37), d, seed, flat=True)
        c[:, 16:] = np.float32(1 / 16)
        return q, c
    if name.startswith("pile"):               # a top pile of P rows over a spread of lower scores
        D = rng.integers(-1500, 1501, size=n)
        D[rng.choice(n, int(name[4:]), replace=False)] = 2000
        return designed(D, d, seed, flat=True)
    if name == "outliers":                    # one row far above, one far below, the bulk on two values: the sd is the outliers'
        D = rng.integers(0, 2, size=n)
        if n >= 2:
            D[n // 3], D[2 * n // 3] = 2047, -2048
        return designed(D, d, seed, flat=True)
    if name == "corpus":                      # tests/exact_common.py: piles straddling ranks 1, 10, 100, 256
        q, c, _ = E.make_corpus("ip", n, d, NQ, seed)
        return q, c
    raise ValueError(name)


@functools.lru_cache(maxsize=16)
def reference(name, n, d, seed):
    q, c = family(name, n, d, seed)
    t = E.truth(q, c, "ip")
    order = E.canonical_order(t)
    refs = {k: E.ref_topk(t.astype(np.float32), order, k) for k in KS}
    return q, c, refs


def run_searches(ix, q, refs, n_live, block256, what):
    seen = []
    for nq, ks in ((17, KS), (1, (10, 129)), (NQ, (10, 129))):
        for k in ks:
            s, i, st = ix.search(q[:nq], k, algo="mfma", return_stats=True)
            last = nq if nq < NQ else block256
            seen.append((nq, k, last * n_live, st["candidates"]))
            assert st["algo"] == 2 and st["levels"] == 1, (what, nq, k, st)
            assert st["candidates"] == last * n_live, (what, nq, k, st)
            assert st["fallback_queries"] == 0, (what, nq, k, st)
            want_s, want_i = refs[k]
            bad = np.argwhere(i != want_i[:nq])
            assert bad.size == 0, (what, nq, k, bad[:5].tolist(), [(int(i[b, r]), int(want_i[b, r])) for b, r in bad[:5]])
            assert np.array_equal(s, want_s[:nq]), (what, nq, k)
    return seen


def sizes(kernel, fam):
    if fam == "staircase":
        return ALL_N if kernel == "anyd-bf16" else EDGE_N
    if fam == "equal":
        return (128, 129, 2049, 8192)
    if fam == "outliers":
        return (2049, 4097, 8192)
    if fam == "corpus":
        return (2047, 4096, 8191)
    return (8192,) if kernel in ("anyd-bf16", "mfma16-bf16") else (4097,)


PILES = tuple(f"pile{p}" for p in (9, 10, 11, 128, 129, 130, 2047, 2048, 2049))      # k - 1, k, k + 1 at k = 10 and 129; the sort's limit
CASES = [(kn, fam) for kn in KERNELS for fam in ("staircase", "equal", "outliers")]
CASES += [(kn, "corpus") for kn in ("anyd-bf16", "mfma16-bf16")]
CASES += [(kn, p) for kn in ("anyd-bf16", "mfma16-bf16") for p in PILES] + [(kn, "pile2049") for kn in ("mfma32-bf16", "mfma16-f32")]
CASES.sort(key=lambda c: (c[1], KERNELS[c[0]][1]))          # a family's corpora are made once per width


@pytest.mark.parametrize("kernel,fam", CASES, ids=lambda v: str(v))
def test_every_regime_returns_the_canonical_order(ts, kernel, fam):
    dtype, d, options, block256 = KERNELS[kernel]
    printed = []
    for n in sizes(kernel, fam):
        q, c, refs = reference(fam, n, d, 100 + n)
        with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip") as ix:
            for name, v in options.items():
                ix.set_option(name, v)
            if n > 4096:
                ix.set_option("TS_MFMA_FIRST_ROWS", 8192)
            seen = run_searches(ix, q, refs, n, block256, (kernel, fam, n))
            printed.append((n, seen[0][2:], seen[-1][2:]))
    print(f"{kernel} {fam}: (n, (modelled, observed) candidates of the first and last search) {printed}")


# ---- NaN rows ------------------------------------------------------------------------------------------------------------
def test_nan_rows_are_no_candidates_and_an_unfillable_k_reruns(ts):
    """100 rows, three of them NaN.  k = 50: 97 candidates per query, the one-wave path, exact.  k = 100: the 97 candidates
    are fewer than min(k, rows) = 100, which is what an estimate that overshot looks like, so the query is re-run by the
    exact scan.  That re-run is by design (the select cannot tell 'three rows have no score' from 'the threshold lost
    three rows'); its answer is the 97 rows and three (-inf, -1)."""
    n, d, nq = 100, 128, 17
    q, c = family("staircase", n, d, 5)
    c = c.copy()
    c[[7, 64, 99], 20] = np.nan
    t = E.truth(q, np.nan_to_num(c), "ip")
    t[:, [7, 64, 99]] = -np.inf                              # ranked last, then cut off
    order = E.canonical_order(np.where(np.isinf(t), -1000.0, t))
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        for k, fb in ((50, 0), (100, nq)):
            s, i, st = ix.search(q[:nq], k, algo="mfma", return_stats=True)
            want_s, want_i = E.ref_topk(t[:nq].astype(np.float32), order[:nq], k)
            want_i[np.isinf(want_s)] = -1
            assert (st["algo"], st["levels"], st["candidates"], st["fallback_queries"]) == (2, 1, nq * 97, fb), st
            assert np.array_equal(i, want_i) and np.array_equal(s, want_s), k
            if k == 100:
                assert (i[:, 97:] == -1).all() and np.isinf(s[:, 97:]).all() and (i[:, :97] >= 0).all()
            print(f"nan rows k={k}: modelled candidates {nq * 97}, observed {st['candidates']}, re-runs {st['fallback_queries']}")


# ---- subset index, row offset ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [100, 200], ids=lambda v: f"keep{v}")
def test_subset_and_offset_indexes_return_global_ids(ts, keep):
    """A subset of a 300-row parent (id_map) and an index with a row offset, through the one-wave path (100 rows, k <= 128)
    and the general one (k = 129, or 200 rows): ids are the parent's, ties still go to the lower id."""
    n, d, nq, off = 300, 128, 17, 1000
    q, c = family("staircase", n, d, 6)
    c = c.copy()
    c[:, 0] = 0                                              # sixteen rows per score: ties everywhere
    rows = np.sort(np.random.default_rng(keep).choice(n, keep, replace=False))
    t = E.truth(q[:nq], c, "ip")
    order = E.canonical_order(t)
    allowed = np.zeros(n, dtype=bool)
    allowed[rows] = True
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip", row_offset=off) as ix:
        with ix.subset(rows + off) as sub:
            for k in (10, 128, 129, 256):
                s, i, st = sub.search(q[:nq], k, algo="mfma", return_stats=True)
                want_s, want_i = E.ref_topk(t.astype(np.float32), order, k, allowed)
                want_i[want_i >= 0] += off
                assert (st["algo"], st["levels"], st["candidates"], st["fallback_queries"]) == (2, 1, nq * keep, 0), st
                assert np.array_equal(i, want_i) and np.array_equal(s, want_s), ("subset", k)
        for k in (10, 128, 129, 256):
            s, i, st = ix.search(q[:nq], k, algo="mfma", return_stats=True)
            want_s, want_i = E.ref_topk(t.astype(np.float32), order, k)
            want_i[want_i >= 0] += off
            assert (st["algo"], st["levels"], st["candidates"], st["fallback_queries"]) == (2, 1, nq * n, 0), st
            assert np.array_equal(i, want_i) and np.array_equal(s, want_s), ("offset", k)
    with ts.TheoremIndex.from_embeddings(c[:100], dtype="bf16", metric="ip", row_offset=off) as small:
        s, i, st = small.search(q[:nq], 10, algo="mfma", return_stats=True)       # 100 candidates: the one-wave path adds the offset
        want_s, want_i = E.ref_topk(t[:, :100].astype(np.float32), E.canonical_order(t[:, :100]), 10)
        assert st["candidates"] == nq * 100 and np.array_equal(i, want_i + off) and np.array_equal(s, want_s)


# ---- two levels, candidates lost -------------------------------------------------------------------------------------------
def test_a_tie_pile_larger_than_the_candidate_list_reruns_exactly(ts):
    """100,000 rows, every 11th (9,091 rows) tied at the top score of every query, k = 256.  The sample holds 285 of
    the pile, so the k-th best - the pile's score - is the threshold (the model: the Gaussian estimate lies below it) and
    the full pass appends 9,091 candidates to a list of 8,192: the `lost` branch.  Every query re-runs; the answer is the
    256 lowest rows of the pile."""
    n, d, nq, k = 100_000, 128, 17, 256
    rng = np.random.default_rng(3)
    D = rng.integers(-200, 201, size=n)                      # (a narrow bulk: the Gaussian estimate stays below the pile)
    D[::11] = 2000
    q, c = designed(D, d, 3, flat=True)
    q = q[np.arange(NQ) % 4 == 0][:nq] * np.float32([[1], [2]])[np.arange(nq) % 2]         # pure queries, weights +1 and +2
    t = E.truth(q, c, "ip")
    m = M.model_search(t, k)
    assert len(m.levels) == 2 and set(m.terms()) == {"kth"} and m.sums() == (nq * 9091, nq * 9091) and m.fallbacks() == (nq, nq)
    with ts.TheoremIndex.from_embeddings(c, dtype="bf16", metric="ip") as ix:
        s, i, st = ix.search(q, k, algo="mfma", return_stats=True)
    print(f"tie pile: modelled candidates {m.sums()}, observed {st['candidates']}, re-runs {st['fallback_queries']}")
    assert (st["algo"], st["levels"], st["candidates"], st["fallback_queries"]) == (2, 2, nq * 9091, nq), st
    assert np.array_equal(i, np.tile(np.arange(0, 11 * k, 11), (nq, 1)))
    assert np.array_equal(s, t[:, :1].astype(np.float32).repeat(k, axis=1))
