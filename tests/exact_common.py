"""Corpora whose fp32 dot products are exact in any summation order, with planted piles of exactly tied scores, and the
canonical reference (score descending, then row ascending) shared by the CPU and GPU exact-tie tests.

Two lattices:
- ip:  entries k / 16, k in [-2, 2].  Every product is a multiple of 2^-8 and every partial sum stays below 2^8 in
       magnitude (d <= 1024), so fp32 adds it exactly in any order, and bf16 stores the entries exactly.
- cos: a row holds m = 4^j entries of +-1 (m in 1, 4, 16, 64, 256) and zeros elsewhere; some rows are all zero.  Its
       norm is exactly 2^j, so the prepared row is +-2^-j (exact in bf16) and every score is dyadic.

The first RES columns belong to the "pile" queries.  Background rows are zero there, so a pile query scores every
background row exactly 0 (one huge pile at 0, with -0 products where the query is negative); planted rows carry values
there that put them on a few score levels: piles of distinct rows with one score each, placed around the 16 / 32 / 64-row
tile edges, the 256-row padding edge, the shard cuts and the last rows.  The fp64 truth is then the bit-exact answer of
every kernel, and every check compares with np.array_equal.
"""
import numpy as np

RES = 16                     # columns reserved for the pile queries
KINDS = ("pileA", "pileB", "neg", "dense", "dense", "dense", "dense", "dense")   # query kind = KINDS[i % 8]
EPS_BREAK = 2.0 ** -30       # tie-break step for the metric checks: eps * n < 2^-8 (the lattices' smallest score gap)

# pileA: levels straddling ranks 1, 10, 100 and 256 (rows 0-2, 3-14, 15-114, 115-314), then the zero pile, then 50 rows
# below zero (the top of the `neg` query, which is pileA's query negated).  pileB: 7 rows above the zero pile, so every
# k > 7 cuts inside a pile of ~n rows (the threshold sample's bisection and candidate overflow).
PILE_A = (3, 12, 100, 200, -50)
PILE_B = (2, 5)


def edges(n):
    """Row positions where a kernel's work splits: tile edges (multiples of 16 / 32 / 64), padding edges (multiples of 256),
    the cuts of 2 and 3 balanced shards, and the end of the corpus."""
    e = [64, 256, 1024 + 32, 4096 + 16, 16384, 16384 + 64 * 7, n // 3, n // 2, 2 * n // 3, n - 1]
    e += [256 * (n // 256), 256 * (n // 512)]
    return sorted({x for x in e if 0 < x < n})


def _positions(rng, count, m, lo, hi):
    """count sets of m distinct columns in [lo, hi) (sorted gaps plus a random rotation: distinct by construction)."""
    width = hi - lo
    step = max(1, width // m)
    pos = np.cumsum(rng.integers(1, step + 1, size=(count, m)), axis=1) - 1
    pos = (pos + rng.integers(0, width, size=(count, 1))) % width
    return pos + lo


def _put_sparse(rows, which, m, lo, hi, rng):
    if which.size == 0 or m == 0:
        return
    cols = _positions(rng, which.size, m, lo, hi)
    signs = rng.choice(np.float32([-1.0, 1.0]), size=cols.shape)
    rows[which[:, None], cols] = signs


def _pick_rows(rng, n, size, used, edge_list):
    """`size` unused rows: up to half of them the nearest unused rows on both sides of edges (so the pile straddles
    them), the rest random."""
    out = []
    want_edge = (size + 1) // 2 if len(edge_list) else 0
    for e in rng.permutation(np.asarray(edge_list, dtype=np.int64)):
        if len(out) >= want_edge:
            break
        half = max(1, min(8, (want_edge - len(out) + 1) // 2))
        for start, step in ((int(e) - 1, -1), (int(e), 1)):
            r, got = start, 0
            while 0 <= r < n and got < half and len(out) < want_edge:
                if not used[r]:
                    used[r] = True
                    out.append(r)
                    got += 1
                r += step
    while len(out) < size:
        r = int(rng.integers(0, n))
        if not used[r]:
            used[r] = True
            out.append(r)
    return np.array(sorted(out), dtype=np.int64)


def _ip_levels(rng, count, total, ncols):
    """count rows of ncols lattice integers in [-2, 2] summing to `total` (|total| <= 2 * ncols)."""
    out = np.zeros((count, ncols), dtype=np.int64)
    sign = 1 if total >= 0 else -1
    for r in range(count):
        left = abs(total)
        while left:
            j = int(rng.integers(0, ncols))
            if out[r, j] * sign < 2:
                out[r, j] += sign
                left -= 1
    return out


def make_corpus(metric, n, d, nq, seed):
    """(queries [nq x d] f32, rows [n x d] f32, piles): piles[kind] = list of row arrays, one per planted level in rank
    order of that kind's query.  Rows and queries are on the metric's lattice (module docstring)."""
    assert metric in ("ip", "cos") and d > RES + 64 and d <= 1024 and n < (1 << 22)
    rng = np.random.default_rng(seed)
    c = np.zeros((n, d), dtype=np.float32)
    if metric == "ip":
        c[:, RES:] = rng.integers(-2, 3, size=(n, d - RES)).astype(np.float32) * np.float32(1 / 16)
    else:
        ms = [m for m in (1, 4, 16, 64, 256) if m <= d - RES]
        m_of = rng.choice(ms, size=n)
        for m in ms:
            _put_sparse(c, np.flatnonzero(m_of == m), m, RES, d, rng)
    used = np.zeros(n, dtype=bool)
    el = edges(n)
    zero = np.concatenate([_pick_rows(rng, n, 8, used, [n // 2]),  # all-zero rows: score 0 for every query
                           _pick_rows(rng, n, n // 200, used, [])])
    c[zero] = 0
    piles = {"pileA": [], "pileB": [], "neg": []}
    # pileA's query: columns 0..7 (ip) or 0..3 (cos, +1 each); pileB's: columns 8..15 / 8..11
    for kind, sizes, col0 in (("pileA", PILE_A, 0), ("pileB", PILE_B, 8)):
        for li, size in enumerate(sizes):
            rows = _pick_rows(rng, n, abs(size), used, el)
            c[rows] = 0
            if metric == "ip":
                total = (16, 12, 8, 4)[li] if size > 0 else -4          # sum of lattice integers on the 8 columns
                c[rows, col0:col0 + 8] = _ip_levels(rng, rows.size, total, 8).astype(np.float32) / np.float32(16)
                _rest = rng.integers(-2, 3, size=(rows.size, d - RES)).astype(np.float32) * np.float32(1 / 16)
                c[rows, RES:] = _rest
            else:
                # (agreeing entries among the query's 4, entries in all): score = agree / (2 sqrt(m)) = 1, 1/2, 1/4, 1/8
                agree, m = ((4, 4), (4, 16), (4, 64), (2, 64))[li] if size > 0 else (4, 16)
                sign = 1.0 if size > 0 else -1.0
                c[rows, col0:col0 + agree] = sign
                _put_sparse(c, rows, m - agree, RES, d, rng)
            piles[kind].append(rows)
    piles["neg"] = [piles["pileA"][-1]]                          # the negated query ranks pileA's last level first
    q = np.zeros((nq, d), dtype=np.float32)
    for i in range(nq):
        kind = KINDS[i % len(KINDS)]
        if kind in ("pileA", "neg", "pileB"):
            col0 = 8 if kind == "pileB" else 0
            sign = -1.0 if kind == "neg" else 1.0
            if metric == "ip":
                q[i, col0:col0 + 8] = sign * 2 / 16
            else:
                q[i, col0:col0 + 4] = sign
        elif metric == "ip":
            q[i] = rng.integers(-2, 3, size=d).astype(np.float32) / np.float32(16)
        else:
            m = int(rng.choice([16, 64, 256] if d >= 256 else [16, 64]))
            _put_sparse(q, np.array([i]), m, 0, d, rng)
    return q, c, piles


def prepare(x, metric):
    """The operand values the kernels multiply: the rows as given (ip) or divided by their norm (cos; exact here, since
    every norm is a power of two).  A zero row stays zero."""
    x = np.asarray(x, dtype=np.float32)
    if metric == "ip":
        return x
    norm = np.sqrt(np.einsum("ij,ij->i", x, x, dtype=np.float64))
    return (x / np.maximum(norm, 1e-12)[:, None]).astype(np.float32)


def truth(q, c, metric):
    """fp64 score matrix.  On these lattices the fp32 BLAS product is exact, so it stands in for the fp64 one (asserted by
    tests/test_exact_ties_cpu.py)."""
    qp, cp = prepare(q, metric), prepare(c, metric)
    return (qp @ cp.T).astype(np.float64) + 0.0            # + 0.0: -0 folded into +0


def canonical_order(t):
    """Per query, every row in the canonical order: score descending, then row ascending."""
    key = -t * 256.0                      # lattice scores are multiples of 2^-8: small integers, sorted by radix sort
    if np.abs(key).max(initial=0) < 2 ** 15 and np.array_equal(key, np.rint(key)):
        return np.argsort(key.astype(np.int16), axis=1, kind="stable")
    return np.argsort(-t, axis=1, kind="stable")


def rank_matrix(order):
    """rank[i, row] = position of row in query i's canonical order = #(s > s_row) + #(s == s_row and r < row)."""
    r = np.empty_like(order)
    np.put_along_axis(r, order, np.arange(order.shape[1])[None, :].repeat(order.shape[0], 0), axis=1)
    return r


def ref_topk(t, order, k, allowed=None):
    """(scores f32 [nq x k], ids int64 [nq x k]) of the canonical top k (of the allowed rows), padded with (-inf, -1)."""
    nq = t.shape[0]
    s = np.full((nq, k), -np.inf, dtype=np.float32)
    i = np.full((nq, k), -1, dtype=np.int64)
    for b in range(nq):
        o = order[b] if allowed is None else order[b][allowed[order[b]]]
        o = o[:k]
        i[b, :o.size] = o
        s[b, :o.size] = t[b, o]
    return s, i


def ref_count_above(t_row, lo, hi, score, gid):
    """Rows of [lo, hi) that rank before a document with this score and global id."""
    s = t_row[lo:hi]
    rows = np.arange(lo, hi)
    return int(np.sum(s > score) + np.sum((s == score) & (rows < gid)))


def tie_broken(t):
    """truth - row * eps: no ties left, same canonical order, exact in fp64 (scores need 16 bits, rows 18 bits)."""
    assert t.shape[1] < (1 << 22)
    return t - np.arange(t.shape[1], dtype=np.float64)[None, :] * EPS_BREAK


def kind_of(i):
    return KINDS[i % len(KINDS)]
