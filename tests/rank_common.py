"""Helpers shared by the many-targets rank and count tests (test_rank_many_anywidth_gpu.py, test_count_above_many_gpu.py):
target lists with the awkward members, and the check of ranks and scores against the fp64 truth of the oracle."""
import numpy as np

import exact_common as E
from oracle import oracle

GAP = 1e-6        # fp64 gap below which two ranks count as tied
SCORE_TOL = 1e-5


def _targets(truth, seed, n_real):
    """Ragged lists: best, worst, row 7, random rows, a repeat, an out-of-range row; one empty list, one longer than a pass."""
    nq, n = truth.shape
    rng = np.random.default_rng(seed)
    order = np.argsort(-truth, axis=1, kind="stable")
    out = []
    for i in range(nq):
        if nq > 1 and i == 1:
            out.append([])
            continue
        t = [int(order[i, 0]), int(order[i, -1]), int(order[i, min(7, n - 1)])] + [int(x) for x in rng.integers(0, n, 3)]
        t += [t[3], n_real + 5]
        if i == nq - 1:
            t += [int(x) for x in rng.integers(0, n, 33)]       # 41 targets: three passes of 16
        out.append(t)
    return out


def _check_lists(truth, targets, ranks, scores, n):
    for i, t in enumerate(targets):
        r, s = ranks[i], scores[i]
        assert r.shape == (len(t),) and s.shape == (len(t),)
        if not t:
            continue
        exp = oracle.rank_of(truth[[i] * len(t)], t)
        for j, row in enumerate(t):
            if not (0 <= row < n) or truth[i, row] != truth[i, row]:
                assert r[j] == -1 and np.isnan(s[j]), (i, j, row)
                continue
            assert abs(float(s[j]) - truth[i, row]) <= SCORE_TOL, (i, j)
            close = int(np.sum(np.abs(truth[i] - truth[i, row]) <= GAP)) - 1
            assert abs(int(r[j]) - int(exp[j])) <= close, (i, j, row, r[j], exp[j])
        # self-consistency, exact: ranks follow (returned score desc, row asc); repeats share a rank
        seen = {}
        for j, row in enumerate(t):
            if r[j] >= 0:
                if row in seen:
                    assert seen[row] == (int(r[j]), float(s[j]))
                seen[row] = (int(r[j]), float(s[j]))
        rows = sorted(seen, key=lambda x: (-seen[x][1], x))
        rk = [seen[x][0] for x in rows]
        assert rk == sorted(rk) and len(set(rk)) == len(rk), (i, rows, rk)


def exact_many_targets(D, i, rng):
    """Targets of query i on an exact lattice corpus (D: .c, .t, .order, .piles of tests/exact_common.py): a whole pile, more
    than 16 rows of one pile (a pass boundary inside it), rows of the zero pile, whose score many lower rows share (the
    fast reject's equality), repeats and a row past n."""
    n = D.c.shape[0]
    kind = E.kind_of(i)
    if kind == "pileA":
        p2, p3 = D.piles["pileA"][2], D.piles["pileA"][3]
        t = list(np.random.default_rng(i).permutation(p3)) + list(p2[::2][:40]) + [int(p3[0]), int(p2[-1])]
    elif kind in ("pileB", "neg"):
        zeros = D.order[i, 400:]                                      # inside the zero pile
        zeros = zeros[D.t[i, zeros] == 0]
        t = [int(zeros[-1]), int(zeros[-2]), int(zeros[len(zeros) // 2]), int(zeros[0]), n - 1, int(zeros[-1])]
        t += [int(x) for x in D.order[i, :7]]
    else:
        grp = np.flatnonzero(D.t[i] == D.t[i, D.order[i, 256]])       # the tie group at rank 256
        t = [int(x) for x in grp[-20:]] + [int(x) for x in rng.integers(0, n, 8)] + [int(grp[-1]), int(grp[0])]
    return [int(x) for x in t] + [n + 5]


class ExactData:
    """An exact lattice corpus with its truth (fp32 values), canonical order and rank matrix."""

    def __init__(self, metric, n, d, nq, seed):
        self.metric, self.d = metric, d
        self.q, self.c, self.piles = E.make_corpus(metric, n, d, nq, seed)
        t = E.truth(self.q, self.c, metric)
        self.t = t.astype(np.float32)                       # exact: every score is an fp32 value
        self.order = E.canonical_order(t).astype(np.int32)
        self.rank = E.rank_matrix(self.order)
