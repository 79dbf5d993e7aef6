"""metadata.MetaTable's host half - the dictionary encoding of the rows and the compilation of a filter state into a program
of atoms - against the per-row predicates it replaces: the numpy model of the atom semantics (tests/metadata_common.py)
applied to ``table.compile(state)`` over the table's columns equals filters.filter_mask / filters.sql_filter_mask (and
oracle.sql_where) bit for bit.  The tables are built with device=None: nothing here creates a device handle."""
import numpy as np
import pytest

from filters_common import filter_states, make_sql_rows, make_theorems, sql_filter_states
from metadata_common import I32_MAX, model_mask, random_columns, random_programs
from oracle import oracle
from theoremsearch_amd.filters import filter_mask, sql_filter_mask
from theoremsearch_amd.metadata import ANY_IN, IN, IS_NULL, NULL, RANGE, Atom, MetaTable, code_set

_CACHE = {}


def showcase():
    if "showcase" not in _CACHE:
        data = make_theorems(3000)
        _CACHE["showcase"] = (data, MetaTable.from_theorems(data, device=None))
    return _CACHE["showcase"]


def sql():
    if "sql" not in _CACHE:
        rows = make_sql_rows(4000)
        _CACHE["sql"] = (rows, MetaTable.from_sql_rows(rows, device=None))
    return _CACHE["sql"]


@pytest.mark.parametrize("state", list(filter_states()))
def test_compiled_showcase_state_is_filter_mask(state):
    data, table = showcase()
    f = filter_states()[state]
    atoms = table.compile(f)
    assert len(atoms) <= 32 and len({a.group for a in atoms}) <= 16
    assert np.array_equal(model_mask(atoms, table.columns, table.n), filter_mask(data, f))


@pytest.mark.parametrize("state", list(sql_filter_states()))
def test_compiled_sql_state_is_sql_filter_mask_and_the_where_clause(state):
    rows, table = sql()
    f = sql_filter_states()[state]
    atoms = table.compile(f)
    assert len(atoms) <= 32 and len({a.group for a in atoms}) <= 16
    got = model_mask(atoms, table.columns, table.n)
    assert np.array_equal(got, sql_filter_mask(rows, f))
    assert np.array_equal(got, np.array([oracle.sql_where(r, f) for r in rows]))


def test_encoding_keeps_nulls_and_the_loops_defaults():
    data, table = showcase()
    cols = dict(zip(table.names, table.columns))
    assert all(c.dtype == np.int32 and c.shape == (3000,) for name, c in cols.items() if name != "authors")
    # a missing year is 0 and a missing flag False, as the reference loop's .get defaults: not NULL
    assert not any((c == NULL).any() for name, c in cols.items() if name != "authors")
    missing = np.array(["year" not in it for it in data])
    assert missing.any() and (cols["year"][missing] == 0).all() and (cols["year"][~missing] > 0).all()
    assert sorted(table.dicts["type"].values) == ["corollary", "lemma", "proposition", "theorem"]      # type.lower()
    offsets, codes = cols["authors"]
    assert offsets[0] == 0 and offsets[-1] == codes.shape[0] and (np.diff(offsets) >= 1).all()
    rows, table = sql()
    cols = dict(zip(table.names, table.columns))
    for name, key in (("primary_category", "primary_category"), ("type_name", "type_name"), ("year", "year"), ("citations", "citations"),
                      ("source", "link")):
        assert np.array_equal(cols[name] == NULL, np.array([r[key] is None for r in rows])), name
    assert set(np.unique(cols["source"])) == {NULL, 0, 1} and set(np.unique(cols["has_journal_ref"])) == {0, 1}
    assert (cols["paper"] >= 0).all() and len(table.dicts["paper"]) == len({(r["link"], r["title"]) for r in rows})
    offsets, _ = cols["authors"]
    assert np.array_equal(np.diff(offsets) == 0, np.array([r["authors"] is None for r in rows]))       # a NULL list is an empty one


def test_year_and_citation_clauses_have_the_stated_form():
    _, table = sql()
    f = sql_filter_states()["years"]
    atoms = table.compile(f)
    src, year, cit = table.col["source"], table.col["year"], table.col["citations"]
    by_group = {}
    for a in atoms:
        by_group.setdefault(a.group, []).append(a)
    forms = sorted(sorted((a.kind, a.col) for a in g) for g in by_group.values())
    # sources {0, 1}; the year: {source IN {0, 1}} and {year RANGE, source IN {1}}; citations {RANGE, IS_NULL}
    assert forms == sorted([[(IN, src)], [(IN, src)], sorted([(RANGE, year), (IN, src)]), sorted([(RANGE, cit), (IS_NULL, cit)])])
    pair = next(g for g in by_group.values() if sorted((a.kind, a.col) for a in g) == sorted([(RANGE, year), (IN, src)]))
    assert next(a for a in pair if a.kind == IN).set.tolist() == [0b10] and next(a for a in pair if a.kind == RANGE).lo == 2010
    known = table.compile(dict(f, include_unknown_citations=False))
    assert [a.kind for a in known if a.col == cit] == [RANGE]
    # a range beyond int32 is clamped, an empty one allows nothing (but the unknown citations, when asked for)
    a = next(a for a in table.compile(dict(f, citation_range=(-10**12, 10**12))) if a.col == cit and a.kind == RANGE)
    assert (a.lo, a.hi) == (NULL + 1, I32_MAX)
    empty = table.compile(dict(sql_filter_states()["open"], citation_range=(9, 3)))
    got = model_mask(empty, table.columns, table.n)
    assert np.array_equal(got, sql_filter_mask(sql()[0], dict(sql_filter_states()["open"], citation_range=(9, 3)))) and got.any()


def test_string_predicates_become_sets_over_the_dictionaries():
    rows, table = sql()
    f = sql_filter_states()["paper_filter"]
    a = next(a for a in table.compile(f) if a.col == table.col["paper"])
    assert a.kind == IN and a.set_bits == len(table.dicts["paper"]) and a.set.dtype == np.uint32 and a.set.shape[0] == (a.set_bits + 31) // 32
    t = next(a for a in table.compile(sql_filter_states()["types"]) if a.col == table.col["type_name"])
    names = table.dicts["type_name"].values
    want = [i for i, v in enumerate(names) if "theorem" in v.lower() or "lemma" in v.lower()]
    assert np.array_equal(t.set, code_set(want, len(names))) and "Main Theorem" in [names[i] for i in want]


def test_set_rows_re_encodes_a_range_on_the_host():
    data = make_theorems(600)
    table = MetaTable.from_theorems(data, device=None)
    other = make_theorems(100, seed=77)
    other[3] = dict(other[3], authors=["Z. Newcomer"], primary_math_tag="math.ZZ")       # values no dictionary holds yet
    table.set_rows(200, other)
    merged = data[:200] + other + data[300:]
    for name, f in filter_states().items():
        assert np.array_equal(model_mask(table.compile(f), table.columns, table.n), filter_mask(merged, f)), name
    f = dict(filter_states()["open"], authors=["Z. Newcomer"], tags=["math.ZZ"])
    assert np.flatnonzero(model_mask(table.compile(f), table.columns, table.n)).tolist() == [203]
    with pytest.raises(ValueError):
        table.set_rows(550, other)


def test_model_on_hand_made_rows():
    """The model itself, on rows small enough to read: NULL is never true, negated or not, except for IS_NULL."""
    v = np.array([NULL, -1, 0, 3, 8], dtype=np.int32)
    lists = (np.array([0, 0, 2, 3, 3, 5], dtype=np.int64), np.array([1, 9, 4, 0, 40], dtype=np.int32))
    cols = [v, lists]
    s = code_set([0, 3], 8)
    case = lambda *atoms: model_mask(list(atoms), cols, 5).tolist()
    assert case() == [True] * 5
    assert case(Atom(RANGE, 0, 0, 5)) == [False, False, True, True, False]
    assert case(Atom(RANGE, 0, 0, 5, negate=1)) == [False, True, False, False, True]
    assert case(Atom(RANGE, 0, NULL + 1, I32_MAX)) == [False, True, True, True, True]
    assert case(Atom(IN, 0, set=s, set_bits=8)) == [False, False, True, True, False]
    assert case(Atom(IN, 0, negate=1, set=s, set_bits=8)) == [False, True, False, False, True]       # below 0, at set_bits: not in the set
    assert case(Atom(IS_NULL, 0)) == [True, False, False, False, False]
    assert case(Atom(IS_NULL, 0, negate=1)) == [False, True, True, True, True]
    assert case(Atom(ANY_IN, 1, set=code_set([9, 40], 41), set_bits=41)) == [False, True, False, False, True]
    assert case(Atom(ANY_IN, 1, set=code_set([9, 40], 41), set_bits=40)) == [False, True, False, False, False]
    assert case(Atom(RANGE, 0, 0, 5, group=1), Atom(IS_NULL, 0, group=1)) == [True, False, True, True, False]
    assert case(Atom(RANGE, 0, 0, 5, group=1), Atom(RANGE, 0, 3, 9, group=2)) == [False, False, False, True, False]


def test_random_programs_cover_what_the_gpu_test_claims():
    progs = random_programs()
    assert len(progs) == 50 and progs[0] == []
    kinds = {(a.kind, a.negate) for p in progs for a in p}
    assert {(RANGE, 0), (RANGE, 1), (IN, 0), (IN, 1), (ANY_IN, 0), (IS_NULL, 0), (IS_NULL, 1)} <= kinds
    assert max(len(p) for p in progs) == 32 and max(len({a.group for a in p}) for p in progs) == 16
    assert any(a.set_bits == 100_000 for p in progs for a in p)
    assert any(a.kind == RANGE and (a.lo, a.hi) == (NULL + 1, I32_MAX) for p in progs for a in p)
    cols = random_columns(5000)
    offsets, codes = cols[5]
    lens = np.diff(offsets)
    assert lens.min() == 0 and lens.max() == 40 and (cols[0] == NULL).any() and (cols[0] < 0).any() and (cols[4] >= 100_000).any()
    fractions = [model_mask(p, cols, 5000).mean() for p in progs]
    assert min(fractions) == 0.0 and max(fractions) == 1.0 and sum(0.0 < x < 1.0 for x in fractions) >= 30
