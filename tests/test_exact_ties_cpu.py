"""The exact-tie corpora of tests/exact_common.py, checked on the host: their fp32 products are exact in any summation order
(so the fp64 truth is every kernel's bit-exact answer), bf16 stores them unchanged, the cos rows normalise to +-2^-j, and
the host search (ts_search_cpu) returns the canonical order - score descending, then row ascending - through piles of
exactly tied rows."""
import numpy as np
import pytest

import exact_common as E
from oracle import oracle


@pytest.fixture(scope="module", params=[("ip", 768), ("ip", 1024), ("ip", 200), ("cos", 768), ("cos", 384), ("cos", 200)],
                ids=lambda p: f"{p[0]}-{p[1]}")
def lattice(request):
    metric, d = request.param
    q, c, piles = E.make_corpus(metric, 9001, d, 24, 11 + d)
    return metric, d, q, c, piles


def test_fp32_products_are_exact_in_any_order(lattice):
    metric, d, q, c, _ = lattice
    qp, cp = E.prepare(q, metric), E.prepare(c, metric)
    t64 = qp.astype(np.float64) @ cp.astype(np.float64).T
    assert np.array_equal(E.truth(q, c, metric), t64)
    assert np.array_equal((qp @ cp.T).astype(np.float64), t64)                       # BLAS order
    assert np.array_equal((qp[:, ::-1] @ cp[:, ::-1].T).astype(np.float64), t64)     # columns reversed
    acc = np.zeros((q.shape[0], c.shape[0]), dtype=np.float32)                       # one column at a time, in fp32
    for j in np.random.default_rng(d).permutation(d):
        acc += np.outer(qp[:, j], cp[:, j]).astype(np.float32)
    assert np.array_equal(acc.astype(np.float64), t64)


def test_bf16_rounding_is_the_identity(lattice):
    metric, _, q, c, _ = lattice
    for x in (E.prepare(q, metric), E.prepare(c, metric), q, c):
        assert np.array_equal(oracle.round_to_bf16(x), x)


@pytest.mark.parametrize("d", [768, 384, 200])
def test_prepared_cos_rows_are_signed_powers_of_two(d):
    q, c, _ = E.make_corpus("cos", 9001, d, 24, 11 + d)
    for x in (q, c):
        p = E.prepare(x, "cos")
        assert np.array_equal(oracle.l2_normalize(x), p)                     # the library's rule gives the same bits
        nnz = np.count_nonzero(x, axis=1)
        assert set(np.unique(nnz).tolist()) <= {0, 1, 4, 16, 64, 256}
        assert (nnz == 0).any() or x is q                                  # the corpus holds all-zero rows
        for m in np.unique(nnz):
            rows = p[nnz == m]
            want = 0.0 if m == 0 else 1.0 / np.sqrt(m)
            assert np.array_equal(np.abs(rows[rows != 0]), np.full(int(np.sum(rows != 0)), want, np.float32))


def test_piles_sit_where_they_were_planted(lattice):
    metric, _, q, c, piles = lattice
    t = E.truth(q, c, metric)
    order = E.canonical_order(t)
    assert np.array_equal(order, np.argsort(-t, axis=1, kind="stable"))
    pos = 0
    for rows in piles["pileA"][:-1]:                                        # levels straddling ranks 1, 10, 100, 256
        got = order[0, pos:pos + rows.size]
        assert np.array_equal(got, rows) and np.unique(t[0, rows]).size == 1
        pos += rows.size
    assert pos > 256 and t[0, order[0, pos]] == 0.0
    assert np.array_equal(order[2, :piles["neg"][0].size], piles["neg"][0])
    assert np.sum(t[1] == 0.0) > 0.99 * c.shape[0] - 400                    # pileB: k > 7 cuts the zero pile
    for e in E.edges(c.shape[0]):                                           # some pile straddles every edge
        both = [rows for lv in piles.values() for rows in lv if (rows < e).any() and (rows >= e).any()]
        assert both, e


def test_reference_rank_count_and_tie_break(lattice):
    metric, _, q, c, piles = lattice
    n = c.shape[0]
    t = E.truth(q, c, metric)
    order = E.canonical_order(t)
    rank = E.rank_matrix(order)
    rng = np.random.default_rng(3)
    for i in range(q.shape[0]):
        rows = np.concatenate([rng.integers(0, n, 20), order[i, [0, 9, 10, 255, 256, n - 1]]])
        assert np.array_equal(oracle.rank_of(t[[i] * rows.size], rows), rank[i, rows])
        cuts = [0, n // 3, n // 2, n]
        for r in rows[:6]:
            total = sum(E.ref_count_above(t[i], a, b, t[i, r], r) for a, b in zip(cuts, cuts[1:]))
            assert total == rank[i, r]
    broken = E.tie_broken(t)
    assert np.unique(broken[0]).size == n
    assert np.array_equal(np.argsort(-broken, axis=1), order)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_host_search_returns_the_canonical_order(lattice, dtype):
    import theoremsearch_amd as ts
    metric, _, q, c, _ = lattice
    t = E.truth(q, c, metric)
    order = E.canonical_order(t)
    with ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric=metric, device=-1) as ix:
        for k in (1, 10, 256):
            s, i = ix.search(q, k)
            want_s, want_i = E.ref_topk(t, order, k)
            assert np.array_equal(i, want_i), (k, np.argwhere(i != want_i)[:5])
            assert np.array_equal(s, want_s), k
