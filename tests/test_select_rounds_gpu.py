"""The scan path's select rounds under many slots: up to 256 queries through `algo="scan"` over a corpus just past the
small-corpus clamp (n > 16,384), so every workgroup of the full grid hands k keys per query to the select and its rounds
run with 256 slots - the golden k = 200 case goes through the matrix path, and the ragged shapes have small n.

Corpus and queries hold small integers (entries in {-2..2}, inner product): every fp32 and bf16 dot product is exact and
ties are frequent.  The expected answer is numpy's int64 dot products in the library's order (score descending, row
ascending); scores and indices are compared exactly.  Which kernels and rounds a shape takes is pinned on the CPU
(tests/scan_plan_check.cpp), not here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 16_640                                  # 16,384 + 256: the full grid's lists reach the select
NQ = 256
SHAPES = [(5, 13), (256, 64), (256, 200), (256, 256)]      # (nq, k)


@pytest.fixture(scope="module", params=[("f32", 64), ("bf16", 768)], ids=lambda p: f"{p[0]}-d{p[1]}")
def case(request):
    """f32 at d = 64 runs the generic kernel, bf16 at d = 768 a specialised one.  One index and one reference per case."""
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    dtype, d = request.param
    rng = np.random.default_rng(13 + d)
    c = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
    q = rng.integers(-2, 3, size=(NQ, d)).astype(np.float32)
    t = q.astype(np.int64) @ c.astype(np.int64).T
    order = np.argsort(-t, axis=1, kind="stable")[:, :256]              # score descending, then row ascending
    want_s = np.take_along_axis(t, order, axis=1).astype(np.float32)
    want_s.setflags(write=False)
    order.setflags(write=False)
    ix = ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip")
    yield q, want_s, order, ix
    ix.close()


@pytest.mark.parametrize("nq,k", SHAPES, ids=lambda v: str(v))
def test_scan_select_rounds_return_the_exact_order(case, nq, k):
    q, want_s, want_i, ix = case
    s, i = ix.search(q[:nq], k, algo="scan")
    s, i = np.asarray(s), np.asarray(i)
    assert s.shape == (nq, k) and i.shape == (nq, k)
    bad = np.argwhere(i != want_i[:nq, :k])
    assert bad.size == 0, (bad[:5].tolist(), [(int(i[b, r]), int(want_i[b, r])) for b, r in bad[:5]])
    assert np.array_equal(s, want_s[:nq, :k])


# ---- piles of equal scores through the one-launch histogram select --------------------------------------------------------
# At k = 12 the 1,024 workgroups of the full grid hand 12,288 keys per query to ONE launch of select_hist_kernel
# (scan_plan.h: select_plan); k = 1 is one sort of 1,024 keys and (5, 13) takes the rounds.  A pile of equal scores larger
# than the short sort's 2,048 keys puts the histogram's cut bin over that limit, so the select streams every key through
# the per-wave running top-k: "equal" (every row the same: sd = 0, every key in bin 0) and "pile" (3,000 copies of the row
# that scores highest for every query, over random rows).  Ties go to the lower row through every form.
PILE_SHAPES = [(1, 1), (1, 12), (4, 12), (5, 13)]


@pytest.fixture(scope="module", params=[(dt, d, fam) for dt, d in (("f32", 64), ("bf16", 768)) for fam in ("equal", "pile")],
                ids=lambda p: f"{p[0]}-d{p[1]}-{p[2]}")
def pile_case(request):
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    dtype, d, fam = request.param
    rng = np.random.default_rng(29 + d)
    q = rng.integers(0, 3, size=(5, d)).astype(np.float32)              # no negative entry: the all-2 row scores highest
    if fam == "equal":
        c = np.tile(rng.integers(-2, 3, size=(1, d)).astype(np.float32), (N, 1))
    else:
        c = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
        c[rng.choice(N, 3000, replace=False)] = 2
    t = q.astype(np.int64) @ c.astype(np.int64).T
    order = np.argsort(-t, axis=1, kind="stable")[:, :16]
    want_s = np.take_along_axis(t, order, axis=1).astype(np.float32)
    want_s.setflags(write=False)
    order.setflags(write=False)
    ix = ts.TheoremIndex.from_embeddings(c, dtype=dtype, metric="ip")
    yield q, want_s, order, ix
    ix.close()


@pytest.mark.parametrize("nq,k", PILE_SHAPES, ids=lambda v: str(v))
def test_scan_select_of_tie_piles_returns_the_exact_order(pile_case, nq, k):
    q, want_s, want_i, ix = pile_case
    s, i = ix.search(q[:nq], k, algo="scan")
    s, i = np.asarray(s), np.asarray(i)
    assert s.shape == (nq, k) and i.shape == (nq, k)
    bad = np.argwhere(i != want_i[:nq, :k])
    assert bad.size == 0, (bad[:5].tolist(), [(int(i[b, r]), int(want_i[b, r])) for b, r in bad[:5]])
    assert np.array_equal(s, want_s[:nq, :k])
