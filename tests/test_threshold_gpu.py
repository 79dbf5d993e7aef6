"""The threshold estimate of the matrix path, held to the numpy model of tests/threshold_common.py.

Every case is a lattice corpus (scores multiples of 2^-8, exact in bf16 and fp32 in any summation order), so the sample's
scores, mean, sd and k-th best are the same numbers in the library and in the model, and stats["candidates"] - the rows
with score >= thr, summed over the call's queries - must equal the model's count.  tests/test_threshold_model_cpu.py
keeps the cases where that is decidable: no modelled threshold within the rounding bracket of a lattice score.

A search of at most one launch block of queries reports all its queries (the counters describe the last block of a call:
the batches here, 82 queries at most, are one block on every kernel).  Each case runs as the whole batch and again as
sub-batches of 1, 17 and 64 queries (5, 17 and 60 behind a host mask, where the matrix path serves batches only); every
call's sum is held to the model's partial sum, so two errors that cancel in a total still show.  Every case prints its modelled and observed sums once."""
import numpy as np
import pytest

import exact_common as E
import threshold_common as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ts():
    import theoremsearch_amd as ts
    from theoremsearch_amd import _ffi
    assert _ffi.device_count() > 0, "GPU tests need a HIP device"
    return ts


class Held:
    """The index and the canonical order of the corpus in use: consecutive cases share a corpus."""
    key, ix, order = None, None, None


@pytest.fixture(scope="module")
def held():
    h = Held()
    yield h
    if h.ix is not None:
        h.ix.close()


def _index(ts, held, case, c, t):
    key = (case.corpus, case.dtype, case.n, case.d, case.seed)
    if held.key != key:
        if held.ix is not None:
            held.ix.close()
        held.ix = ts.TheoremIndex.from_embeddings(c, dtype=case.dtype, metric="ip")
        held.order = E.canonical_order(t).astype(np.int32)
        held.key = key
    return held.ix, held.order


@pytest.mark.parametrize("case", M.CASES, ids=repr)
def test_candidates_and_fallbacks_are_the_models(ts, held, case):
    q, c, t = M.corpus_of(case.corpus, case.n, case.d, case.seed)
    m, mask = M.model_of(case), M.mask_of(case)
    ix, order = _index(ts, held, case, c, t)
    t32 = t.astype(np.float32)
    want_s, want_i = E.ref_topk(t32, order, case.k, mask)
    seen = []
    try:
        for name, v in case.options.items():
            ix.set_option(name, v)
        for sl in (slice(0, M.NQ),) + (M.SUBS if mask is None else M.SUBS_MASKED):
            s, i, st = ix.search(q[sl], case.k, algo="mfma", return_stats=True, mask=mask)
            lo, hi = m.sums(sl)
            fb_lo, fb_hi = m.fallbacks(sl)
            seen.append((sl.start, sl.stop, (lo, hi), st["candidates"], (fb_lo, fb_hi), st["fallback_queries"]))
            assert st["algo"] == 2 and st["levels"] == case.levels == len(m.levels), st
            assert lo <= st["candidates"] <= hi, seen[-1]
            assert fb_lo <= st["fallback_queries"] <= fb_hi, seen[-1]
            if case.name.startswith(("screen", "noscreen")):
                assert st["screened"] == (1 if case.name.startswith("screen") else 0), st
            if not case.statistical:
                assert st["fallback_queries"] == 0, st             # the guaranteed chain never re-runs
            bad = np.argwhere(i != want_i[sl])
            assert bad.size == 0, (sl, bad[:5].tolist(), [(int(i[b, r]), int(want_i[sl][b, r])) for b, r in bad[:5]])
            assert np.array_equal(s, want_s[sl]), sl
    finally:
        for name in case.options:
            ix.set_option(name, None)
        print(f"{case.name}: (first query, end, modelled candidates, observed, modelled fallbacks, observed) {seen}")
