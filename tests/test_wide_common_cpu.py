"""What the k-chunked matrix search's GPU tests (tests/test_wide_gpu.py) take from tests/wide_common.py, checked without a GPU:
the block-marker corpus is exact in fp32 and shows a mishandled 64-element block, and the fp32 chain the kernels add stays
within SCORE_TOL / 2 of the fp64 scores on the parity cases - which is why those keep the narrower widths' tolerance."""
import numpy as np
import pytest

import wide_common as WC
from oracle import oracle

WIDTHS = [(dtype, d) for dtype in ("bf16", "f32") for d in WC.MARKER_WIDTHS[dtype]]


@pytest.mark.parametrize("dtype,d", WIDTHS, ids=lambda v: str(v))
def test_marker_corpus_is_exact_and_shows_a_mishandled_block(dtype, d):
    q, c, exact = WC.marker_corpus(d)
    nb = d // 64
    assert c.shape == (3 * nb + 1, d) and q.shape == (256, d)
    # bf16 holds every value, fp32 adds every score exactly in any order: the fp32 product, the kernels' chain and a reversed
    # chain all give the integers
    assert np.array_equal(oracle.bf16_bits_to_f32(oracle.f32_to_bf16_bits(c)), c) and np.array_equal(oracle.bf16_bits_to_f32(oracle.f32_to_bf16_bits(q)), q)
    assert np.abs(q).astype(np.int64).sum(axis=1).max() * 8 < 2 ** 24           # the bound on every partial sum
    assert np.array_equal((q @ c.T).astype(np.int64), exact)
    assert np.array_equal(WC.chain_scores(q, c, dtype).astype(np.int64), exact)
    assert np.array_equal(WC.chain_scores(q[:, ::-1], c[:, ::-1], dtype).astype(np.int64), exact)
    # rows: one block each, constants 1 .. 8, the three rows of a block distinct; the last row all ones
    for r in (0, 1, nb - 1, nb, 3 * nb - 1):
        nz = np.flatnonzero(c[r])
        assert nz.size == 64 and nz[0] == 64 * (r % nb) and nz[-1] == nz[0] + 63 and 1 <= c[r, nz[0]] <= 8 and (c[r, nz] == c[r, nz[0]]).all()
    assert (c[-1] == 1).all()
    for b in (0, nb - 1):
        assert len({c[b + i * nb, 64 * b] for i in range(3)}) == 3
    # the reference of the assertions the GPU test makes: canonical order, integer scores, for both batch sizes and both k
    for nq in (17, 256):
        for k in (10, 256):
            s, i = WC.canonical_topk(exact[:nq], k)
            assert s.shape == (nq, k) and (i[:, :min(k, c.shape[0])] >= 0).all()
            assert np.array_equal(s[:, :10], np.take_along_axis(exact[:nq], i[:, :10], axis=1).astype(np.float32))
            assert (np.diff(s[:, :min(k, c.shape[0])], axis=1) <= 0).all()
    # a pass that drops or doubles ANY one block, or swaps two blocks a chunk or two apart (or neighbours), changes a row's score -
    # for the first 17 queries alone
    blocks_per_chunk = 8 if dtype == "bf16" else 4
    for b0 in range(nb):
        for fault in ("drop", "double"):
            f = WC.faulty_scores(q, c, exact, fault, b0)
            for nq in (17, 256):
                assert (f[:nq] != exact[:nq]).any(axis=0)[np.arange(b0, 3 * nb, nb)].all(), (fault, b0, nq)   # each of the block's three rows
        for dist in (1, blocks_per_chunk, 2 * blocks_per_chunk):
            if b0 + dist < nb:
                f = WC.faulty_scores(q, c, exact, "swap", b0, b0 + dist)
                for nq in (17, 256):
                    assert (f[:nq] != exact[:nq]).any(axis=0)[[b0, b0 + dist]].all(), ("swap", b0, dist, nq)


def test_blocks_five_apart_share_a_query_pattern():
    """The limit of the corpus, as its docstring says: such a swap is invisible to the marker rows."""
    q, c, exact = WC.marker_corpus(2560)
    assert np.array_equal(WC.faulty_scores(q, c, exact, "swap", 0, 5)[:, :-1], exact[:, :-1])


@pytest.mark.parametrize("dtype,d,n,nq,k,metric", WC.PARITY, ids=lambda v: str(v))
def test_the_chain_model_stays_within_half_the_score_tolerance(dtype, d, n, nq, k, metric):
    """The first 1,024 rows of each parity case (the rows are independent draws: the error of a score does not depend on the
    row's position), every query."""
    q, c = oracle.inputs(n, nq, d, WC.PARITY_SEED, metric)
    qp, cp = oracle.prepared_inputs(q, c[:1024], metric, dtype)
    truth = oracle.scores_fp64(qp, cp)
    model = WC.chain_scores(np.asarray(qp, dtype=np.float32), np.asarray(cp, dtype=np.float32), dtype)
    worst = float(np.abs(model.astype(np.float64) - truth).max())
    print(dtype, d, metric, "worst |chain - fp64|", worst)
    assert worst <= WC.SCORE_TOL / 2
