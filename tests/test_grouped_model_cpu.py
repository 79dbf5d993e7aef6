"""The grouped search's two numpy models (tests/grouped_common.py) agree: the semantics - a brute-force walk of every query's
whole canonical order that keeps the first row of each group - and the method - over-fetch, collapse, certify; deepen;
exclude - with the depths taken from ts_group_depth.  The corpora are tests/exact_common.py's (the same score bits in every
arithmetic), so the GPU test compares the library with these very arrays, bit for bit, and its ts_grouped_stats with the
stages counted here.  The designs the GPU test relies on must reach every stage; that is asserted here, without a device."""
import numpy as np
import pytest

import grouped_common as gc


def test_depths_come_from_the_library():
    assert gc.depths(1) == (17, 256) and gc.depths(10) == (26, 256) and gc.depths(32) == (64, 256)
    assert gc.depths(100) == (200, 256) and gc.depths(128) == (256, 256) and gc.depths(256) == (256, 256)


@pytest.mark.parametrize("name", list(gc.CORPORA))
@pytest.mark.parametrize("design", ["row8", "pile", "two", "null", "mixed"])
def test_ladder_is_the_brute_force_walk(name, design):
    for k in gc.KS + ((256,) if design == "row8" else ()):
        for masked in (False, True):
            gc.reference(name, design, masked, k)         # asserts that the two models agree


@pytest.mark.parametrize("name", list(gc.CORPORA))
def test_designs_reach_the_stages_the_gpu_test_relies_on(name):
    # one group of 315 rows on top of the pile queries: every stage is needed, and stage 1 still certifies most queries
    s1, s2, s3 = gc.stage_counts(name, "pile", 10)
    assert s1 >= 1 and s2 >= 1 and s3 >= 1 and s1 + s2 + s3 == 2 * gc.NQ
    if name == "cos768":
        assert (s1, s2, s3) == (24, 6, 2)
    # groups of 8 consecutive rows at k = 10: stage 2 suffices
    assert gc.stage_counts(name, "row8", 10) == (28, 4, 0)
    # first == deep from k = 128: nothing is ever deepened, the open queries go straight to the exclusion
    assert gc.stage_counts(name, "row8", 100)[1] == 0 and gc.stage_counts(name, "row8", 100)[2] >= 1
    # k = 256: every query is excluded, with up to 8 rounds
    assert gc.stage_counts(name, "row8", 256) == (0, 0, 2 * gc.NQ)
    assert max(int(gc.reference(name, "row8", m, 256)[4].max()) for m in (False, True)) == 8
    # two groups in the whole corpus: k > 2 ends short and padded, after the pass that excludes both
    for k in (10, 32, 100):
        assert gc.stage_counts(name, "two", k) == (0, 0, 2 * gc.NQ)
        for masked in (False, True):
            s, i, g, stage, passes = gc.reference(name, "two", masked, k)
            assert (passes == 2).all() and ((i >= 0).sum(axis=1) == 2).all() and (g[:, 2:] == gc.NULL).all()
    assert gc.stage_counts(name, "two", 1) == (2 * gc.NQ, 0, 0)
    # every row a group of its own: the over-fetch is never needed
    for k in gc.KS:
        assert gc.stage_counts(name, "null", k) == (2 * gc.NQ, 0, 0)


def test_null_groups_give_the_plain_top_k():
    import exact_common as ec
    q, c, piles, t, order = gc.corpus("ip128")
    for masked in (False, True):
        allowed = gc.row_mask() if masked else None
        s, i, g, _, _ = gc.reference("ip128", "null", masked, 32)
        want_s, want_i = ec.ref_topk(t, order, 32, allowed)
        assert np.array_equal(s, want_s) and np.array_equal(i, want_i) and (g == gc.NULL).all()


def test_collapse_walk_on_hand_made_lists():
    column = np.array([5, 5, gc.NULL, -3, gc.NULL, -3, 9], dtype=np.int32)
    scores = np.array([[9, 8, 7, 6, 5, 4, -np.inf, -np.inf]], dtype=np.float32)
    idx = np.array([[0, 1, 2, 3, 4, 5, 6, -1]], dtype=np.int64)
    s, i, g, found, complete = gc.collapse_walk(scores, idx, column, 4)
    assert i.tolist() == [[0, 2, 3, 4]] and g.tolist() == [[5, gc.NULL, -3, gc.NULL]] and s.tolist() == [[9, 7, 6, 5]]
    assert found.tolist() == [5] and complete.tolist() == [True]
    s, i, g, found, complete = gc.collapse_walk(scores[:, :6], idx[:, :6], column, 6)
    assert i.tolist() == [[0, 2, 3, 4, -1, -1]] and found.tolist() == [4] and complete.tolist() == [False]
    # a valid row with score -inf is an entry, an id outside the column is padding; global ids
    s, i, g, found, complete = gc.collapse_walk(scores, idx + 100, column, 8, row_offset=100)
    assert i.tolist() == [[100, 102, 103, 104, 106, -1, -1, -1]] and found.tolist() == [5] and complete.tolist() == [True]
    s, i, g, found, complete = gc.collapse_walk(scores, idx, column[:3], 8)
    assert i.tolist() == [[0, 2, -1, -1, -1, -1, -1, -1]] and complete.tolist() == [True]
