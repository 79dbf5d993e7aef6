"""The host side of the search behind a row set per query, without a device: `MetaTable.eval_many` makes one row set per
distinct filter state and refuses the 257th, `pgvector.search_sessions` hands the sessions to ONE `search_rowsets` call at the
largest top_k and cuts each list to its own, in `pgvector.search`'s shape.  The index and the evaluation are stubs."""
import numpy as np
import pytest

from theoremsearch_amd import _ffi, pgvector
from theoremsearch_amd.metadata import Atom, MetaTable, RANGE


class StubSet:
    def __init__(self, program):
        self.program = program


def stub_table(monkeypatch):
    """An encode-only table of ready-made columns whose `eval` records the programs it is given."""
    t = MetaTable.from_columns([np.arange(16, dtype=np.int32), np.arange(16, dtype=np.int32) % 3], device=None)
    evaluated = []

    def fake_eval(self, atoms, stream=0):
        evaluated.append(list(atoms))
        return StubSet(list(atoms))
    monkeypatch.setattr(MetaTable, "eval", fake_eval)
    return t, evaluated


def program(lo, hi, col=0):
    return [Atom(RANGE, col, lo=lo, hi=hi, group=0)]


def test_eval_many_makes_one_set_per_distinct_state(monkeypatch):
    t, evaluated = stub_table(monkeypatch)
    states = [program(0, 5), program(2, 9), program(0, 5), None, program(2, 9), program(0, 5, col=1), None]
    sets, which = t.eval_many(states)
    assert which.dtype == np.int32 and which.tolist() == [0, 1, 0, -1, 1, 2, -1]
    assert len(sets) == 3 and len(evaluated) == 3
    assert [(a.lo, a.hi, a.col) for s in sets for a in s.program] == [(0, 5, 0), (2, 9, 0), (0, 5, 1)]
    # programs with a code set are compared by their words
    with_set = lambda words: [Atom(1, 1, set=np.asarray(words, dtype=np.uint32), set_bits=40)]
    sets, which = t.eval_many([with_set([5, 1]), with_set([5, 1]), with_set([5, 3])])
    assert which.tolist() == [0, 0, 1] and len(sets) == 2
    sets, which = t.eval_many([])
    assert sets == [] and which.shape == (0,)


def test_eval_many_refuses_the_257th_distinct_state(monkeypatch):
    t, evaluated = stub_table(monkeypatch)
    states = [program(0, i) for i in range(256)]
    sets, which = t.eval_many(states + states[:10] + [None])
    assert len(sets) == 256 == _ffi.TS_MAX_ROWSETS and which.tolist() == list(range(256)) + list(range(10)) + [-1]
    del evaluated[:]
    with pytest.raises(ValueError, match="256 distinct"):
        t.eval_many(states + [program(0, 256)])
    assert evaluated == []                                # refused before anything is evaluated


class StubIndex:
    """`search_rowsets` answers query i with rows 100 i, 100 i + 1, ... at falling scores; a set named "short" allows three."""
    row_offset = 0

    def __init__(self):
        self.calls = []

    def search_rowsets(self, q, k, rowsets, which, algo="auto", return_stats=False):
        self.calls.append((q.shape, k, list(rowsets), np.asarray(which).tolist()))
        scores = np.full((q.shape[0], k), -np.inf, dtype=np.float32)
        idx = np.full((q.shape[0], k), -1, dtype=np.int64)
        for i, w in enumerate(np.asarray(which)):
            have = 3 if (w >= 0 and rowsets[w] == "short") else k
            scores[i, :have] = -0.25 - 0.01 * np.arange(have)
            idx[i, :have] = 100 * i + np.arange(have)
        return scores, idx


def test_search_sessions_cuts_each_list_to_its_top_k():
    ix = StubIndex()
    a, b = "dense", "short"
    top_ks = [1, 20, 7, 5, 2]
    masks = [a, None, b, a, b]
    out = pgvector.search_sessions(ix, np.zeros((5, 8), np.float32), top_ks, masks)
    assert len(ix.calls) == 1                             # one call for all sessions
    shape, k, rowsets, which = ix.calls[0]
    assert shape == (5, 8) and k == 20 and rowsets == [a, b] and which == [0, -1, 1, 0, 1]
    assert [len(o) for o in out] == [1, 20, 3, 5, 2]      # the short set's list ends at its padding
    for i, hits in enumerate(out):
        assert [h["row"] for h in hits] == [100 * i + j for j in range(len(hits))]
        for j, h in enumerate(hits):
            assert set(h) == {"row", "similarity", "score"}           # pgvector.search's dict
            assert isinstance(h["row"], int) and isinstance(h["score"], float)
            assert h["similarity"] == h["score"] == 1.0 + float(np.float32(-0.25 - 0.01 * j))


def test_search_sessions_refuses_ragged_arguments():
    ix = StubIndex()
    with pytest.raises(ValueError):
        pgvector.search_sessions(ix, np.zeros((3, 8), np.float32), [1, 2], [None, None, None])
    with pytest.raises(ValueError):
        pgvector.search_sessions(ix, np.zeros((2, 8), np.float32), [1, 0], [None, None])
    assert pgvector.search_sessions(ix, np.zeros((0, 8), np.float32), [], []) == [] and ix.calls == []
