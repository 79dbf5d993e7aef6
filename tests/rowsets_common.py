"""Helpers of tests/test_rowsets_gpu.py, the tests of the search behind a row set per query (ts_search_rowsets): seeded masks
of a given density, row sets made from arbitrary masks, the corpora (exact lattices of tests/exact_common.py,
Gaussian rows of oracle.inputs) with their references computed once, the routing restated from the issue's rules, and the
CPU model's verdict on which queries a threshold would send to the exact re-run (tests/threshold_common.py)."""
import functools

import numpy as np

import exact_common as E
import threshold_common as M
from oracle import oracle

N = 20_000                    # above TS_MFMA_MIN_ROWS (16,384); the last 64-row staging tile is half full
N_ODD = 16_417                # ... and a last mask word of one bit
MFMA, SCAN = 2, 1


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same_rows(a, b):
    """(scores, idx) pairs equal bit for bit."""
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def dense_mask(n, density, seed):
    """bool[n] with exactly round(density * n) rows allowed, seeded."""
    m = np.zeros(n, dtype=bool)
    m[np.random.default_rng(seed).permutation(n)[: int(round(density * n))]] = True
    return m


class SetMaker:
    """Row sets from arbitrary bool masks: a table whose one column is the row number, and the program  row IN {allowed rows}."""

    def __init__(self, ts, n):
        from theoremsearch_amd.metadata import IN, Atom, code_set
        self._atom = lambda mask: [Atom(IN, 0, set=code_set(np.flatnonzero(mask), n), set_bits=n)]
        self.table = ts.MetaTable.from_columns([np.arange(n, dtype=np.int32)])
        self.made = []

    def __call__(self, mask):
        rs = self.table.eval(self._atom(mask))
        assert rs.allowed == int(mask.sum())
        self.made.append(rs)
        return rs

    def close(self):
        for rs in self.made:
            rs.close()
        self.table.close()


@functools.lru_cache(maxsize=4)
def lattice(n, d, nq, seed=5):
    """(queries, rows, truth, canonical order) of an inner-product lattice corpus: every score exact in any summation order."""
    q, c, _ = E.make_corpus("ip", n, d, nq, seed)
    t = E.truth(q, c, "ip")
    return q, c, t, E.canonical_order(t)


@functools.lru_cache(maxsize=2)
def gaussian(d, nq, seed):
    return oracle.inputs(N, nq, d, seed, "ip")


def stored(x, dtype):
    """The values the index holds and multiplies."""
    return oracle.round_to_bf16(x) if dtype == "bf16" else np.asarray(x, dtype=np.float32)


def model_fallbacks(q, c, dtype, k, masks, which):
    """How many queries the CPU model of the threshold estimate sends to the exact re-run, each query behind its own mask:
    (fewest, most) over the bracket of every threshold."""
    t = stored(q, dtype).astype(np.float64) @ stored(c, dtype).astype(np.float64).T
    lo = hi = 0
    for i, w in enumerate(which):
        a, b = M.model_search(t[i:i + 1], k, allowed=None if w < 0 else masks[w]).fallbacks()
        lo, hi = lo + a, hi + b
    return lo, hi


def route(n, allowed, which, k, scan_max):
    """The routing of rowsets_plan.h restated for an index the pass serves, under `auto`: (pass queries, {set: queries of its
    per-set call}, calls).  allowed[s]: rows set s allows."""
    which = np.asarray(which)
    pop = np.array([n if w < 0 else allowed[w] for w in which])
    dense = pop * 10 >= n
    limit = 1 if k > 64 else scan_max
    rides = dense if (dense.sum() > limit and len(set(which[dense].tolist())) >= 2) else np.zeros(len(which), dtype=bool)
    groups = {}
    for i, w in enumerate(which.tolist()):
        if not rides[i]:
            groups.setdefault(w, []).append(i)
    calls = sum(1 for w in groups if w < 0 or allowed[w] > 0)
    return np.flatnonzero(rides), groups, calls
