"""The threshold model (tests/threshold_common.py) against hand-computed samples, and the conditions under which the GPU
test (tests/test_threshold_gpu.py) may hold the library to it: for every case of that test the model's threshold lies
clear of every lattice score (no query "undecided"; a tail-fit case may leave one in 16), nobody is under-filled unless
the case is built for it, the estimates the case is about do set thresholds in the batch, and the plan has the level count
the GPU test asserts."""
import math

import numpy as np
import pytest

import threshold_common as M


# ---- the model against numbers worked out by hand ----------------------------------------------------------------------------
def test_plan_of_the_documented_corpora():
    # 20,011 rows: 626 tiles; stride 8 leaves 79 tiles = 2,528 rows <= 4,096 (stride 4: 157 tiles = 5,024)
    assert M.plan_levels(20_011, 10) == [(8, 79), (1, 626)]
    assert M.plan_levels(40_000, 10) == [(16, 79), (1, 1250)]
    assert M.plan_levels(70_001, 256) == [(32, 69), (1, 2188)]
    # one unthresholded level up to first_rows rows, whole tiles counted
    assert M.plan_levels(4096, 10) == [(1, 128)] and len(M.plan_levels(4097, 10)) == 2
    assert M.plan_levels(8192, 10, first_rows=8192) == [(1, 256)] and len(M.plan_levels(8193, 10, first_rows=8192)) == 2
    # the guaranteed chain at k = 10: the full pass is planned for max(64, 8 k) = 80 candidates -> ratio 8; 70,001 rows need a
    # third level (274 tiles of stride 8 = 8,768 rows > 8,192)
    assert M.plan_levels(20_011, 10, statistical=False) == [(8, 79), (1, 626)]
    assert M.plan_levels(70_001, 10, statistical=False) == [(16, 137), (8, 274), (1, 2188)]
    # the last tile of a sample is partial when n ends inside it: 20,011 = 625 * 32 + 11, tile 625 is not sampled (625 % 8 = 1)
    assert M.level_rows(20_011, 8, 79).size == 2528 and M.level_rows(20_011, 8, 79)[-1] == 78 * 256 + 31
    assert M.level_rows(70, 2, 2).tolist() == list(range(32)) + [64, 65, 66, 67, 68, 69]


def test_quantiles_and_candidate_aims():
    assert [M.stat_cands(k) for k in (1, 10, 64, 65, 256)] == [64, 64, 384, 390, 1536]
    assert M.normal_tail_z(0.5) == 0.0 and M.normal_tail_z(0.0) == 8.0
    assert abs(M.normal_tail_z(0.15865525393145707) - 1.0) < 1e-9 and abs(M.normal_tail_z(0.0013498980316301035) - 3.0) < 1e-9


def test_sample_of_64_rows_by_hand():
    """64 live rows: below the 256 the Gaussian estimate needs, so the threshold is the k-th best alone."""
    s = np.arange(64) / 256.0                                   # 0, 1/256 .. 63/256
    r = M.sample_threshold(s, 10, z_tail=2.0)
    assert r.cnt == 64 and r.kth == 54 / 256 and r.term == "kth" and r.lo == r.hi == 54 / 256
    assert r.mean == 31.5 / 256 and abs(r.sd - math.sqrt((64 * 64 - 1) / 12.0) / 256) < 1e-15
    r = M.sample_threshold(s, 65, z_tail=2.0)
    assert r.term == "none" and r.lo == r.hi == -np.inf         # fewer live rows than k: no bound at all


def test_sample_of_256_rows_by_hand():
    """128 rows at +1 and 128 at -1: mean 0, sd 1, so with z = 2 the Gaussian estimate is 2 and beats the k-th best (1);
    with z = 0.5 the k-th best wins.  The bracket is two fp32 neighbours either side of the estimate."""
    s = np.concatenate([np.ones(128), -np.ones(128)])
    r = M.sample_threshold(s, 10, z_tail=2.0)
    assert (r.mean, r.sd, r.kth, r.gauss, r.term) == (0.0, 1.0, 1.0, 2.0, "gauss")
    assert r.lo == 2.0 - 2 * 2.0 ** -23 and r.hi == 2.0 + 2 * 2.0 ** -22
    r = M.sample_threshold(s, 10, z_tail=0.5)
    assert r.term == "kth" and r.lo == r.hi == 1.0
    r = M.sample_threshold(s, 129, z_tail=0.5)                  # the 129th best is -1: the estimate 0.5 wins
    assert r.term == "gauss" and r.kth == -1.0 and r.gauss == 0.5
    # every score equal: sd = 0, the estimate is the score itself and exact
    r = M.sample_threshold(np.full(300, 0.25), 10, z_tail=3.0)
    assert r.sd == 0.0 and r.lo == r.hi == 0.25


def test_tail_fit_by_hand():
    """1,024 rows: 992 zeros and 32 rows on a staircase 32/256 .. 1/256.  x_32 = 1/256, spacing = sum_{j=8..31} (x_j - x_32)
    = sum_{m=1..24} m / 256 = 300 / 256, e = spacing / 13.959..., and with tail_p = 1/128 the ratio is (32/1024) * 128 = 4."""
    s = np.concatenate([np.zeros(992), np.arange(1, 33) / 256.0])
    r = M.sample_threshold(s, 10, z_tail=1.0, tail_p=1.0 / 128, tail_z=-0.5)      # (tail_z = -0.5: heavy when x_32 > mean)
    e = (300 / 256) / 13.95928363
    want = 1 / 256 + e * math.log(4.0)
    assert r.heavy_margin > 0 and r.term == "tail" and abs(r.tail - want) < 1e-7
    assert r.lo < want < r.hi and r.hi - r.lo < 2e-6
    # not armed (tail_p = 0), or the 32nd best is already past the aim (ratio <= 1): the fit says nothing
    assert M.sample_threshold(s, 10, z_tail=1.0).tail == -np.inf
    assert M.sample_threshold(s, 10, z_tail=1.0, tail_p=1.0 / 32, tail_z=-0.5).tail == -np.inf
    # a sample that shows no heavy tail is never extrapolated
    assert M.sample_threshold(s, 10, z_tail=1.0, tail_p=1.0 / 128, tail_z=8.0).term != "tail"


def test_counts_and_fallbacks_by_hand():
    t = np.array([[0.0, 1.0, 2.0, 3.0, np.nan], [3.0, 3.0, 3.0, 3.0, np.nan]])
    live = ~np.isnan(t[0])
    assert M.expected_candidates(np.where(np.isnan(t), -np.inf, t), [2.0, 3.5], live).tolist() == [2, 0]
    m = M.model_search(t, 2)                                     # one level: every live row is a candidate
    assert m.levels == [(1, 1)] and m.sums() == (8, 8) and m.fallbacks() == (0, 0)
    m = M.model_search(t, 5)                                     # 4 live rows < min(k, pop) = 5: both queries re-run
    assert m.fallbacks() == (2, 2)


# ---- the GPU test's cases stay within the model's conditions -------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES, ids=repr)
def test_case_is_decidable(case):
    m = M.model_of(case)
    assert len(m.levels) == case.levels
    undecided = int(m.undecided.sum())
    assert undecided <= (M.NQ // 16 if case.tail_case else 0), (undecided, M.closest_lattice_gap(m))
    if not case.may_underfill:
        assert not m.under_filled().any()
    terms = set(m.terms())
    assert set(case.want_terms) <= terms, terms
    if case.tail_case:
        # the heavy-tail verdict is not a close call either: x_32 is clear of mean + (tail_z + 0.5) sd by far more than rounding
        assert min(x.heavy_margin for x in m.thr) > 1e-3
    if case.name.startswith("armed"):
        assert all(x.heavy_margin is not None and x.heavy_margin < -1e-3 for x in m.thr)     # armed, and rightly silent
    lo, hi = m.sums()
    print(f"{case.name}: levels {len(m.levels)}, modelled candidates {lo}..{hi}, fallbacks {m.fallbacks()}, "
          f"terms { {t: m.terms().count(t) for t in sorted(terms)} }, closest lattice point {M.closest_lattice_gap(m)}")


def test_cases_cover_what_they_claim():
    by = {c.name: M.model_of(c) for c in M.CASES if c.corpus != "clustered"}
    # the mask cases: half the rows, and a sample with fewer live rows than k (no bound: every allowed row is a candidate)
    assert by["mask-starved-bf16-d128"].count_lo.tolist() == [2100] * M.NQ
    assert 39 <= by["mask-half-bf16-d128"].count_lo.min()
    # every row equal: n candidates, over the cap, every query re-runs
    assert by["equal-bf16-d128"].fallbacks() == (M.NQ, M.NQ)
    # two values: where the pile is on top its score is the threshold and the pile is the candidate set, elsewhere the
    # estimate overshoots both values and the query re-runs
    for name, pile in (("two-sparse-bf16-d128", 20_011 // 20), ("two-pile-bf16-d128", 4030)):
        c = by[name].count_lo
        assert (c == pile).sum() >= 16 and (c == 0).sum() >= 16, (name, np.unique(c))
    # the same corpus through the screen, without it, and through the list-form sample: one model
    assert by["screen-bf16-d768"].sums() == by["noscreen-bf16-d768"].sums() == by["listform-bf16-d768"].sums()
