"""Numpy models of the grouped search (include/tsearch.h: ts_search_grouped) shared by the CPU and GPU tests.

- `collapse_walk`: the collapse step on sorted lists, entry by entry.
- `brute_force`: the semantics - a walk of a query's whole canonical order (score descending, row ascending) over the allowed
  rows that keeps the first row of every group, NULL rows being groups of their own.
- `ladder`: the method - over-fetch at depth `first`, collapse, certify; deepen to `deep`; exclude the groups found so far
  and search again until k groups or no rows are left - with the depths taken from ts_group_depth.  It returns the answer
  and, per query, the last stage it needed and the exclusion passes it ran: what ts_grouped_stats must count.
- `designs`, `corpus`, `reference`: the group columns and exact corpora (tests/exact_common.py: the same score bits in every
  arithmetic) the tests run on, the order computed once per corpus.
"""
import functools

import numpy as np

import exact_common as ec

NULL = -2**31
N, NQ, SEED = 16869, 16, 7            # no multiple of 256, above the matrix path's 16,384-row floor
CORPORA = {"ip128": ("ip", 128), "cos768": ("cos", 768)}
KS = (1, 10, 32, 100)


# ---- the collapse step ------------------------------------------------------------------------------------------------------
def collapse_walk(scores, idx, column, k_out, row_offset=0):
    """(scores, idx, groups [nq x k_out], found [nq], complete [nq]) of sorted lists [nq x k_in]: an entry is kept when its
    code is NULL or no earlier entry of its list has the code; ids outside the column and NaN scores are padding."""
    scores, idx = np.asarray(scores, dtype=np.float32), np.asarray(idx, dtype=np.int64)
    column = np.asarray(column, dtype=np.int32)
    nq, k_in = scores.shape
    n = column.shape[0]
    os_ = np.full((nq, k_out), -np.inf, dtype=np.float32)
    oi = np.full((nq, k_out), -1, dtype=np.int64)
    og = np.full((nq, k_out), NULL, dtype=np.int32)
    found = np.zeros(nq, dtype=np.int32)
    complete = np.zeros(nq, dtype=bool)
    for q in range(nq):
        seen, padded, m = set(), False, 0
        for j in range(k_in):
            i, s = int(idx[q, j]), scores[q, j]
            if i < 0 or not (row_offset <= i < row_offset + n) or s != s:
                padded = True
                continue
            code = int(column[i - row_offset])
            if code != NULL:
                if code in seen:
                    continue
                seen.add(code)
            if m < k_out:
                os_[q, m], oi[q, m], og[q, m] = s, i, code
            m += 1
        found[q] = m
        complete[q] = m >= k_out or padded
    return os_, oi, og, found, complete


# ---- the semantics ---------------------------------------------------------------------------------------------------------
def _group_firsts(order_codes):
    """positions, ascending, of the entries of a code sequence that are the first of their group"""
    null = order_codes == NULL
    _, first = np.unique(order_codes, return_index=True)
    first = first[order_codes[first] != NULL]
    return np.sort(np.concatenate([first, np.flatnonzero(null)]))


def brute_force(t, order, codes, k, allowed=None, row_offset=0):
    """(scores f32, ids int64, groups int32), each [nq x k]: a walk of every query's whole canonical order."""
    nq = t.shape[0]
    s = np.full((nq, k), -np.inf, dtype=np.float32)
    i = np.full((nq, k), -1, dtype=np.int64)
    g = np.full((nq, k), NULL, dtype=np.int32)
    for b in range(nq):
        o = order[b] if allowed is None else order[b][allowed[order[b]]]
        o = o[~np.isnan(t[b, o])]
        rows = o[_group_firsts(codes[o])[:k]]
        s[b, :rows.size], i[b, :rows.size], g[b, :rows.size] = t[b, rows], rows + row_offset, codes[rows]
    return s, i, g


# ---- the method ------------------------------------------------------------------------------------------------------------
def depths(k):
    from theoremsearch_amd import group_depth
    return group_depth(k)


def _list(t_row, rows, depth):
    """the search's answer at `depth` over the rows `rows` (already in canonical order): one list, padded"""
    s = np.full((1, depth), -np.inf, dtype=np.float32)
    i = np.full((1, depth), -1, dtype=np.int64)
    rows = rows[:depth]
    s[0, :rows.size], i[0, :rows.size] = t_row[rows], rows
    return s, i


def ladder(t, order, codes, k, allowed=None):
    """The answer by the three stages, with LOCAL ids; returns (scores, ids, groups, stage [nq] in 1..3, passes [nq])."""
    first, deep = depths(k)
    nq = t.shape[0]
    s = np.full((nq, k), -np.inf, dtype=np.float32)
    i = np.full((nq, k), -1, dtype=np.int64)
    g = np.full((nq, k), NULL, dtype=np.int32)
    stage = np.zeros(nq, dtype=np.int64)
    passes = np.zeros(nq, dtype=np.int64)
    for b in range(nq):
        o = order[b] if allowed is None else order[b][allowed[order[b]]]
        stage[b] = 1
        cs, ci, cg, _, complete = collapse_walk(*_list(t[b], o, first), codes, k)
        if not complete[0] and first < deep:
            stage[b] = 2
            cs, ci, cg, _, complete = collapse_walk(*_list(t[b], o, deep), codes, k)      # replaces the stage-1 list
        if not complete[0]:
            stage[b] = 3
            have, gone = 0, np.zeros(codes.shape[0], dtype=bool)
            cs, ci, cg = cs.copy(), ci.copy(), cg.copy()
            cs[:], ci[:], cg[:] = -np.inf, -1, NULL                                       # the first pass replaces the stage-2 list
            while True:
                passes[b] += 1
                assert passes[b] <= k + 1
                rs, ri, rg, found, complete = collapse_walk(*_list(t[b], o[~gone[o]], deep), codes, k - have)
                fresh = min(int(found[0]), k - have)
                cs[0, have:have + fresh], ci[0, have:have + fresh], cg[0, have:have + fresh] = rs[0, :fresh], ri[0, :fresh], rg[0, :fresh]
                have += fresh
                if complete[0]:
                    break
                assert fresh >= 1, "a full list without padding holds at least one new group"
                for row, code in zip(ri[0, :fresh], rg[0, :fresh]):
                    if code == NULL:
                        gone[row] = True
                    else:
                        gone |= codes == code
        s[b], i[b], g[b] = cs[0], ci[0], cg[0]
    return s, i, g, stage, passes


# ---- corpora and designs ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus(name):
    """(queries, rows, piles, truth, order) of a corpus of CORPORA, computed once and left unchanged"""
    metric, d = CORPORA[name]
    q, c, piles = ec.make_corpus(metric, N, d, NQ, seed=SEED)
    t = ec.truth(q, c, metric)
    order = ec.canonical_order(t)
    for a in (q, c, t, order):
        a.setflags(write=False)
    return q, c, piles, t, order


@functools.lru_cache(maxsize=None)
def row_mask():
    """the 60 % random row set of the tests"""
    m = np.random.default_rng(SEED + 1).random(N) < 0.6
    m.setflags(write=False)
    return m


def designs(piles):
    """name -> int32 group column [N].  code = row // 8 unless the design says otherwise."""
    base = (np.arange(N) // 8).astype(np.int32)
    pile = base.copy()
    pile[np.concatenate(piles["pileA"][:4])] = -7          # all 315 rows of pileA's four top levels are one group (a negative id)
    two = (np.arange(N) % 2).astype(np.int32)
    null = np.full(N, NULL, dtype=np.int32)
    mixed = base.copy()                                   # NULLs and negative ids among ordinary codes
    mixed[::3] = NULL
    mixed[1::6] = -1 - base[1::6]
    out = {"row8": base, "pile": pile, "two": two, "null": null, "mixed": mixed}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, design, masked, k):
    """brute force and ladder of one case, agreeing; returns (scores, ids, groups, stage, passes)"""
    q, c, piles, t, order = corpus(name)
    codes = designs(piles)[design]
    allowed = row_mask() if masked else None
    want = brute_force(t, order, codes, k, allowed)
    s, i, g, stage, passes = ladder(t, order, codes, k, allowed)
    assert np.array_equal(s, want[0]) and np.array_equal(i, want[1]) and np.array_equal(g, want[2]), (name, design, masked, k)
    return s, i, g, stage, passes


def stage_counts(name, design, k):
    """queries whose last stage was 1 / 2 / 3 over the 2 x NQ (query, mask) cases of a design"""
    stages = np.concatenate([reference(name, design, masked, k)[3] for masked in (False, True)])
    return tuple(int((stages == s).sum()) for s in (1, 2, 3))
