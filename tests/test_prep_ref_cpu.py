"""The inputs and the reference of the row-preparation tests (prep_common.py) have the properties the GPU file relies on:
order-free rows sum exactly in any order, few enough Gaussian rows are undecided, and the reference agrees with
oracle.l2_normalize / oracle.f32_to_bf16_bits wherever those are defined the same way (rows without a NaN)."""
import numpy as np
import pytest

import prep_common as pc
from oracle import oracle

SOURCES = ("f32", "bf16")


def _sums_three_ways(x):
    v = x.astype(np.float64) ** 2
    forward = np.cumsum(v, axis=1)[:, -1]                 # strictly left to right
    reverse = np.cumsum(v[:, ::-1], axis=1)[:, -1]
    blocked = np.einsum("ij,ij->i", x.astype(np.float64), x.astype(np.float64))
    return forward, reverse, blocked


def _exact_sums(x):
    """Sum of squares in integer arithmetic: every finite entry is m * 2^-149 with an integer m."""
    out = []
    for row in x.astype(np.float64):
        m = [int(v * 2.0 ** 149) for v in row.tolist()]   # exact: a power-of-two scaling of an fp32 value
        out.append(sum(k * k for k in m))
    return out


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("d", pc.WIDTHS + (8, 16384))
def test_order_free_rows_sum_exactly_in_any_order(d, src):
    n = 24 if d == 16384 else 200
    x = pc.widen(pc.as_source(pc.order_free_rows(n, d, 77 + d), src))
    assert x.shape == (n, d) and np.isfinite(x).all()
    forward, reverse, blocked = _sums_three_ways(x)
    assert np.array_equal(forward, reverse) and np.array_equal(forward, blocked)
    for i, e in enumerate(_exact_sums(x[:8])):            # and that common value is the true sum
        assert int(forward[i] * 2.0 ** 298) == e
    # the form itself: per row, integer multiples of one of the four powers of two, at most 2048 of them in magnitude
    ok = np.zeros(n, dtype=bool)
    for e in pc.EXPONENTS:
        s = x / np.float32(2.0) ** e
        ok |= ((s == np.round(s)) & (np.abs(s) <= pc.MAX_M + 1)).all(axis=1)
    assert ok.all()


def test_order_free_rows_use_every_exponent_and_the_full_range():
    x = pc.order_free_rows(pc.N_FREE, 100, 1100)
    top = np.abs(x).max(axis=1)
    seen = {e for e in pc.EXPONENTS if ((top > 1024 * 2.0 ** e) & (top <= pc.MAX_M * 2.0 ** e)).any()}
    assert seen == set(pc.EXPONENTS)


@pytest.mark.parametrize("src", SOURCES)
def test_gaussian_cases_leave_few_rows_undecided(src):
    mask = pc.gaussian_decided(src)
    assert mask.shape == (pc.GAUSS_N,)
    undecided = int((~mask).sum())
    print(f"gaussian {src}: {undecided} of {mask.size} rows undecided")
    assert undecided <= pc.UNDECIDED_CAP * mask.size


def test_decided_rows_marks_a_norm_on_a_rounding_boundary():
    """[1, 2^-12, 2^-12, 2^-24] has ss = (1 + 2^-24)^2 exactly: its root is the midpoint of two fp32 neighbours, so the
    smallest summation error moves the fp32 norm.  [3, 4] has norm 5, far from any boundary."""
    x = np.zeros((2, 4), dtype=np.float32)
    x[0, :2] = [3.0, 4.0]
    x[1] = [1.0, 2.0 ** -12, 2.0 ** -12, 2.0 ** -24]
    assert float((x[1].astype(np.float64) ** 2).sum()) == (1.0 + 2.0 ** -24) ** 2
    assert pc.decided_rows(x).tolist() == [True, False]


def _equal_outside_nan(a, b):
    an, bn = np.isnan(a), np.isnan(b)
    return np.array_equal(an, bn) and np.array_equal(a.view(np.uint32)[~an], b.view(np.uint32)[~bn])


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("d", pc.WIDTHS + (8,))
def test_reference_equals_the_oracle_on_rows_without_a_nan(d, src):
    rows = pc.width_case(d, src)
    x = pc.widen(rows)
    clean = ~np.isnan(x).any(axis=1)
    assert clean.sum() >= pc.N_FREE + 6
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        want = oracle.l2_normalize(x)
    got = pc.prepare(rows, "cos", "f32")
    assert _equal_outside_nan(got[clean], want[clean])
    gotb = pc.prepare(rows, "cos", "bf16")
    assert gotb.dtype == np.uint16
    gb, wb = gotb[clean], oracle.f32_to_bf16_bits(want)[clean]
    nan = np.isnan(want[clean])
    assert np.array_equal(gb[~nan], wb[~nan]) and np.isnan(oracle.bf16_bits_to_f32(gb)[nan]).all()
    # without normalisation: the values as given / their RNE bits, NaN rows included
    assert np.array_equal(pc.prepare(rows, "ip", "f32").view(np.uint32), x.view(np.uint32))
    assert np.array_equal(pc.prepare(rows, "ip", "bf16"), oracle.f32_to_bf16_bits(x))


@pytest.mark.parametrize("src", SOURCES)
def test_reference_equals_the_oracle_on_decided_gaussian_rows(src):
    rows = pc.gaussian_case(src)
    x = pc.widen(rows)
    mask = pc.gaussian_decided(src)
    want = oracle.l2_normalize(x)
    assert np.array_equal(pc.prepare(rows, "cos", "f32")[mask].view(np.uint32), want[mask].view(np.uint32))
    assert np.array_equal(pc.prepare(rows, "cos", "bf16")[mask], oracle.f32_to_bf16_bits(want)[mask])


def test_fp64_quotient_rounded_once_more_equals_fp32_division():
    """x_n = float32(float64(x) / float64(denom)) is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2 bits)."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal(1 << 20, dtype=np.float32) * np.float32(2.0) ** rng.integers(-30, 30, 1 << 20).astype(np.float32)
    y = np.abs(rng.standard_normal(1 << 20, dtype=np.float32)) + np.float32(1e-3)
    assert np.array_equal((x.astype(np.float64) / y.astype(np.float64)).astype(np.float32), x / y)


@pytest.mark.parametrize("d", [1, 2, 65, 768])
def test_special_rows_prepare_as_described(d):
    s = pc.special_rows(d)
    assert s.shape == (pc.n_special(), d)
    cos = pc.prepare(s, "cos", "f32")
    assert not cos[0].any() and not np.signbit(cos[0]).any()                  # a zero row stays zero
    assert cos[1, d - 1] == np.float32(1e-30) / pc.EPS                        # divided by 1e-12, not by its norm
    if d >= 2:
        assert not cos[2].any()                                               # norm = inf: every entry becomes 0
        assert np.isnan(cos[3, d - 1]) and not cos[3, :d - 1].any()           # finite / inf = 0, inf / inf = NaN
        assert np.isnan(cos[4, d // 2]) and np.array_equal(np.delete(cos[4], d // 2), np.delete(s[4], d // 2) / pc.EPS)
    assert np.signbit(cos[5, ::2]).all() and not cos[5, ::2].any()            # -0.0 stays -0.0
    assert cos[6, d - 1] == np.float32(2.0 ** -133) / pc.EPS                  # denormals: below 1e-12 as a row
    if d >= 3:
        assert cos[7, d - 1] == np.float32(2.0 ** -133) and cos[7, d // 2] == np.float32(1e-40)   # and stored as denormals
    ip16 = pc.prepare(s, "ip", "bf16")
    if d >= 4:
        assert tuple(int(ip16[pc.TIES_ROW, d - 1 - i]) for i in range(4)) == pc.BF16_EDGE_BITS
    assert int(ip16[9, d - 1]) == 0x7FC0                                      # the quiet bit keeps it a NaN
    assert np.isnan(pc.widen(pc.as_source(s, "bf16"))[9, d - 1])


def test_query_rows_are_finite_with_the_two_specials():
    for nq in (1, 3, 257):
        q = pc.query_rows(nq, 100, 9)
        assert q.shape == (nq, 100) and np.isfinite(q).all()
        if nq >= 3:
            assert not q[1].any() and np.count_nonzero(q[2]) == 1 and q[2, 99] == np.float32(1e-30)
