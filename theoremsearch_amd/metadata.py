"""The rows' metadata as columns in HBM, and filter states evaluated to the row mask on the device.

`filters.filter_mask` / `filters.sql_filter_mask` call a Python predicate once per row.  Here the same predicates are
compiled once per filter state into a short program of atoms over dictionary-encoded columns (`MetaTable.compile`): every
string predicate - a tag list, an ILIKE over type names, the paper box - is evaluated on the host over the column's
DICTIONARY (a few distinct values, or the distinct papers) and handed over as a set of codes, never per row.  One kernel
(``ts_meta_eval``) then reads the columns the program names and writes the bitmask and its population count: a `RowSet`,
which `TheoremIndex.search(..., mask=)` and `search_biased(..., mask=)` take wherever they take a bool array.  Because a row
set knows how many rows it allows, a query batch behind it runs on the matrix path (a bare device mask cannot).

A program is in conjunctive normal form: atoms of one ``group`` are OR-ed, the groups are AND-ed; an atom on a NULL value is
not true, negated or not (SQL's WHERE), except IS_NULL.  The semantics are those of ``include/tsearch.h``.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Mapping, Optional, Sequence

import numpy as np

from . import _ffi

RANGE, IN, ANY_IN, IS_NULL = 0, 1, 2, 3
NULL = -2**31                              # TS_META_NULL
_I32_MAX = 2**31 - 1

# set: uint32 words (bit c & 31 of word c >> 5 = code c) or None; set_bits: codes the set ranges over
Atom = namedtuple("Atom", "kind col lo hi negate group set set_bits", defaults=(0, 0, 0, 0, None, 0))


def code_set(codes, nbits: int) -> np.ndarray:
    """The bitset of ``codes`` over ``nbits`` codes, as the uint32 words an IN / ANY_IN atom carries."""
    bits = np.zeros((int(nbits) + 31) // 32 * 32, dtype=bool)
    codes = np.asarray(list(codes), dtype=np.int64)
    if codes.size:
        bits[codes] = True
    return np.packbits(bits, bitorder="little").view(np.uint32) if bits.size else np.zeros(0, dtype=np.uint32)


class RowSet:
    """A device row bitmask (the layout of ``ts_search_filtered``) and the number of rows it allows.  Immutable; owns its
    device memory until `close`."""

    def __init__(self, handle: C.c_void_p):
        self._lib = _ffi.load()
        self._h = handle
        n, allowed, ptr = C.c_int64(0), C.c_int64(0), C.c_void_p()
        _ffi.check(self._lib.ts_rowset_info(self._h, C.byref(n), C.byref(allowed), C.byref(ptr)))
        self.n, self.allowed, self.mask_ptr = n.value, allowed.value, ptr.value or 0

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def words(self) -> np.ndarray:
        """The mask as it lies on the device: ceil(n / 32) uint32 words."""
        out = np.zeros((self.n + 31) // 32, dtype=np.uint32)
        _ffi.check(self._lib.ts_rowset_download(self._h, _ffi.as_ptr(out)))
        return out

    def to_numpy(self) -> np.ndarray:
        """bool[n]: the rows the set allows."""
        return np.unpackbits(self.words().view(np.uint8), bitorder="little")[: self.n].astype(bool)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _ffi.check(self._lib.ts_rowset_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _Dictionary:
    """value -> code, codes in the order of first appearance; grows with the rows that are encoded."""

    def __init__(self):
        self.code = {}
        self.values = []

    def encode(self, v) -> int:
        c = self.code.get(v)
        if c is None:
            c = self.code[v] = len(self.values)
            self.values.append(v)
        return c

    def __len__(self):
        return len(self.values)

    def codes_where(self, pred) -> np.ndarray:
        return code_set([c for c, v in enumerate(self.values) if pred(v)], len(self.values))


_SHOWCASE = ("type", "tag", "source", "citations", "year", "journal", "authors")
_SQL = ("source", "paper", "has_journal_ref", "primary_category", "type_name", "year", "citations", "authors")


class MetaTable:
    """Per-row metadata of one index as int32 columns (dictionary codes, numbers, 0 / 1 flags; `NULL` = SQL NULL) plus the
    authors as a list column.  ``device=None`` only encodes: the columns (``columns``) and `compile` work, nothing touches a
    device and `eval` raises."""

    def __init__(self, form: str, rows: Sequence[Mapping], device: Optional[int] = 0):
        self.form = form
        self.names = _SHOWCASE if form == "showcase" else _SQL
        self.col = {name: i for i, name in enumerate(self.names)}
        self.dicts = {name: _Dictionary() for name in self.names}
        self.n = len(rows)
        self.device = device
        scalars, lists = self._encode(rows)
        self.columns = [None] * len(self.names)          # per column: int32[n], or (offsets int64[n + 1], codes int32)
        for name, a in scalars.items():
            self.columns[self.col[name]] = a
        self._lists = lists                                # authors: one list of codes per row
        self.columns[self.col["authors"]] = self._csr(lists)
        self._create()

    def _create(self) -> None:
        """The device handle and a first upload of every column (``device=None``: neither)."""
        self._lib, self._h = None, C.c_void_p()
        if self.device is None:
            return
        self._lib = _ffi.load()
        _ffi.check(self._lib.ts_meta_create(int(self.device), self.n, len(self.names), C.byref(self._h)))
        for name, c in zip(self.names, self.columns):
            if isinstance(c, tuple):
                self._upload_lists(name)
            else:
                self._upload_scalar(name, 0, self.n)

    # -- construction -----------------------------------------------------------------------
    @classmethod
    def from_columns(cls, columns: Sequence, device: Optional[int] = 0, names: Optional[Sequence[str]] = None,
                     dictionaries: Optional[Mapping] = None) -> "MetaTable":
        """A table of ready-made columns - int32[n] per scalar column (`NULL` = SQL NULL), ``(offsets int64[n + 1], codes
        int32)`` per list column - for callers that hold their metadata as arrays already: `eval` takes programs (lists of
        `Atom`); no `set_rows`.  With ``dictionaries`` ({column name: its values in code order}) and the column names of
        `from_sql_rows` (source, paper, has_journal_ref, primary_category, type_name, year, citations, authors) the table also
        compiles that form's filter states."""
        t = object.__new__(cls)
        t.form = "columns"
        t.names = tuple(names) if names is not None else tuple(f"c{i}" for i in range(len(columns)))
        t.col = {name: i for i, name in enumerate(t.names)}
        t.dicts, t._lists = {}, None
        if dictionaries is not None:
            if t.names != _SQL:
                raise ValueError(f"dictionaries need the columns {_SQL}")
            for name in t.names:
                d = t.dicts[name] = _Dictionary()
                for v in dictionaries.get(name, ()):
                    d.encode(v)
        t.columns = [(np.ascontiguousarray(c[0], dtype=np.int64), np.ascontiguousarray(c[1], dtype=np.int32)) if isinstance(c, tuple)
                     else np.ascontiguousarray(c, dtype=np.int32) for c in columns]
        first = t.columns[0]
        t.n = int(first[0].shape[0] - 1 if isinstance(first, tuple) else first.shape[0])
        t.device = device
        t._create()
        return t

    @classmethod
    def from_theorems(cls, theorems_data: Sequence[Mapping], device: Optional[int] = 0) -> "MetaTable":
        """The showcase app's library (app_showcase_model.py:102-121; the items `filters.filter_mask` takes): ``type.lower()``,
        ``primary_math_tag``, ``source`` and the authors dictionary-encoded, ``citations``, ``year`` (missing: 0) and
        ``journal_published`` (missing: 0) as numbers - the loop's own ``.get`` defaults, not NULLs."""
        return cls("showcase", theorems_data, device)

    @classmethod
    def from_sql_rows(cls, rows: Sequence[Mapping], device: Optional[int] = 0) -> "MetaTable":
        """The joined (paper, theorem) rows behind the embedding table (the rows `filters.sql_filter_mask` takes), NULLs kept:
        ``source`` 0 = the link contains arxiv.org, 1 = any other link, NULL = no link; ``paper`` a code per distinct
        (link, title); ``has_journal_ref`` 0 / 1; ``primary_category``, ``type_name``, ``year``, ``citations`` with None as
        NULL; the authors as a list (None: empty)."""
        return cls("sql", rows, device)

    def _encode(self, rows: Sequence[Mapping]):
        n = len(rows)
        d = self.dicts
        scalars = {name: np.empty(n, dtype=np.int32) for name in self.names if name != "authors"}
        lists = []
        if self.form == "showcase":
            for i, it in enumerate(rows):
                scalars["type"][i] = d["type"].encode(it["type"].lower())
                scalars["tag"][i] = d["tag"].encode(it["primary_math_tag"])
                scalars["source"][i] = d["source"].encode(it["source"])
                scalars["citations"][i] = it["citations"]
                scalars["year"][i] = it.get("year", 0)
                scalars["journal"][i] = 1 if it.get("journal_published", False) else 0
                lists.append([d["authors"].encode(a) for a in it["authors"]])
            return scalars, lists
        for i, r in enumerate(rows):
            link = r.get("link")
            scalars["source"][i] = NULL if link is None else (0 if "arxiv.org" in link.lower() else 1)
            scalars["paper"][i] = d["paper"].encode((link, r.get("title")))
            scalars["has_journal_ref"][i] = 0 if r.get("journal_ref") is None else 1
            cat, name = r.get("primary_category"), r.get("type_name")
            scalars["primary_category"][i] = NULL if cat is None else d["primary_category"].encode(cat)
            scalars["type_name"][i] = NULL if name is None else d["type_name"].encode(name)
            scalars["year"][i] = NULL if r.get("year") is None else r["year"]
            scalars["citations"][i] = NULL if r.get("citations") is None else r["citations"]
            lists.append([d["authors"].encode(a) for a in (r.get("authors") or ())])
        return scalars, lists

    @staticmethod
    def _csr(lists):
        offsets = np.zeros(len(lists) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in lists], out=offsets[1:])
        codes = np.fromiter((c for x in lists for c in x), dtype=np.int32, count=int(offsets[-1]))
        return offsets, codes

    def _upload_scalar(self, name: str, row0: int, nrows: int) -> None:
        a = np.ascontiguousarray(self.columns[self.col[name]][row0:row0 + nrows])
        _ffi.check(self._lib.ts_meta_set_column(self._h, self.col[name], _ffi.as_ptr(a), int(row0), int(nrows)))

    def _upload_lists(self, name: str = "authors") -> None:
        offsets, codes = self.columns[self.col[name]]
        _ffi.check(self._lib.ts_meta_set_lists(self._h, self.col[name], _ffi.as_ptr(offsets), _ffi.as_ptr(codes)))

    def set_rows(self, row0: int, rows: Sequence[Mapping]) -> None:
        """Rows [row0, row0 + len(rows)) replaced by ``rows`` (items of the table's own form): the upsert by ``slogan_id``.
        The scalar columns are re-uploaded for that range only; the list column is set whole, and only when an author list
        of the range changed.  Row sets made earlier keep their bits."""
        row0 = int(row0)
        if self.form == "columns":
            raise ValueError("a table of ready-made columns has no row encoder")
        if row0 < 0 or row0 + len(rows) > self.n:
            raise ValueError("rows outside the table")
        scalars, lists = self._encode(rows)
        for name, a in scalars.items():
            self.columns[self.col[name]][row0:row0 + len(rows)] = a
            if self._h.value:
                self._upload_scalar(name, row0, len(rows))
        if lists != self._lists[row0:row0 + len(rows)]:
            self._lists[row0:row0 + len(rows)] = lists
            self.columns[self.col["authors"]] = self._csr(self._lists)
            if self._h.value:
                self._upload_lists()

    # -- filter state -> program --------------------------------------------------------------
    def _range(self, name: str, lo, hi, group: int) -> Atom:
        lo, hi = max(int(lo), NULL + 1), min(int(hi), _I32_MAX)
        if lo > hi:                                         # no value lies in it: the empty set
            return Atom(IN, self.col[name], group=group, set=np.zeros(0, dtype=np.uint32), set_bits=0)
        return Atom(RANGE, self.col[name], lo, hi, group=group)

    def _in(self, name: str, pred, group: int, negate: int = 0, kind: int = IN) -> Atom:
        return Atom(kind, self.col[name], negate=negate, group=group, set=self.dicts[name].codes_where(pred),
                    set_bits=len(self.dicts[name]))

    def _codes(self, name: str, codes, nbits: int, group: int, negate: int = 0) -> Atom:
        return Atom(IN, self.col[name], negate=negate, group=group, set=code_set(codes, nbits), set_bits=nbits)

    def compile(self, filters: Mapping) -> list:
        """The filter state as a program (a list of `Atom`, conjunctive normal form): `filters.filter_mask`'s predicates for
        a table `from_theorems`, `filters.sql_filter_mask`'s WHERE clause (clause by clause) for one `from_sql_rows`."""
        if self.form == "columns" and not self.dicts:
            raise ValueError("a table of ready-made columns without dictionaries compiles no filter state: hand `eval` a program")
        return self._compile_showcase(filters) if self.form == "showcase" else self._compile_sql(filters)

    def _compile_showcase(self, f: Mapping) -> list:
        atoms, g = [], 0
        if f.get("types"):
            atoms.append(self._in("type", lambda v: v in f["types"], g)); g += 1
        if f.get("tags"):
            atoms.append(self._in("tag", lambda v: v in f["tags"], g)); g += 1
        if f.get("authors"):
            atoms.append(self._in("authors", lambda v: v in f["authors"], g, kind=ANY_IN)); g += 1
        atoms.append(self._in("source", lambda v: v in f["sources"], g)); g += 1
        lo, hi = f["citation_range"]
        atoms.append(self._range("citations", lo, hi, g)); g += 1
        # the year and the journal status bind arXiv items only: {source is not arXiv} OR {the predicate}
        not_arxiv = lambda group: self._in("source", lambda v: v == "arXiv", group, negate=1)
        if f.get("year_range"):
            atoms += [not_arxiv(g), self._range("year", f["year_range"][0], f["year_range"][1], g)]; g += 1
        status = f.get("journal_status")
        if status in ("Journal Article", "Preprint Only"):
            want = 1 if status == "Journal Article" else 0
            atoms += [not_arxiv(g), self._range("journal", want, want, g)]; g += 1
        return atoms

    def _compile_sql(self, f: Mapping) -> list:
        atoms, g = [], 0
        ARXIV, OTHER = 0, 1
        if f.get("sources"):
            cases = [c for c, name in ((ARXIV, "arXiv"), (OTHER, "Stacks Project")) if name in f["sources"]]
            if cases:
                atoms.append(self._codes("source", cases, 2, g)); g += 1
        if f.get("authors"):
            atoms.append(self._in("authors", lambda v: v in f["authors"], g, kind=ANY_IN)); g += 1          # p.authors && %s
        if f.get("tags"):
            atoms.append(self._in("primary_category", lambda v: v in f["tags"], g)); g += 1
        if f.get("year_range"):
            # OR(AND(arx, between), NOT(arx)) = (arx OR NOT arx) AND (between OR NOT arx): the first is "the link is not NULL"
            atoms.append(self._codes("source", [ARXIV, OTHER], 2, g)); g += 1
            atoms += [self._range("year", f["year_range"][0], f["year_range"][1], g), self._codes("source", [OTHER], 2, g)]; g += 1
        status = f.get("journal_status", "All")
        if status in ("Journal Article", "Preprint Only"):
            want = 1 if status == "Journal Article" else 0
            atoms.append(self._codes("source", [ARXIV], 2, g)); g += 1
            atoms.append(self._range("has_journal_ref", want, want, g)); g += 1
        pf = f.get("paper_filter") or {}
        ids, titles = pf.get("ids") or (), pf.get("titles") or ()
        if ids or titles:
            # the ILIKEs run over the distinct papers, not over the rows
            def paper_matches(p):
                link, title = p
                return ((link is not None and any(i.lower() in link.lower() for i in ids)) or
                        (title is not None and any(t.lower() in title.lower() for t in titles)))
            atoms.append(self._in("paper", paper_matches, g)); g += 1
        if f.get("types"):
            atoms.append(self._in("type_name", lambda v: any(t.lower() in v.lower() for t in f["types"]), g)); g += 1   # lower(t.name) ILIKE ANY
        lo, hi = f["citation_range"]
        atoms.append(self._range("citations", lo, hi, g))
        if f.get("include_unknown_citations"):
            atoms.append(Atom(IS_NULL, self.col["citations"], group=g))
        return atoms

    # -- evaluation ---------------------------------------------------------------------------
    def eval(self, filters_or_atoms, stream: int = 0) -> RowSet:
        """The rows a filter state (or a program: a list of `Atom`) allows, evaluated on the device: a `RowSet`."""
        if self._lib is None or not self._h.value:
            raise ValueError("this MetaTable only encodes (device=None): there is no host evaluator")
        atoms = self.compile(filters_or_atoms) if isinstance(filters_or_atoms, Mapping) else list(filters_or_atoms)
        arr = (_ffi.Atom * max(1, len(atoms)))()
        keep = []
        for i, a in enumerate(atoms):
            arr[i].kind, arr[i].col, arr[i].lo, arr[i].hi = int(a.kind), int(a.col), int(a.lo), int(a.hi)
            arr[i].negate, arr[i].group, arr[i].set_bits = int(a.negate), int(a.group), int(a.set_bits)
            if a.set is not None:
                words = np.ascontiguousarray(a.set, dtype=np.uint32)
                if words.shape[0] < (int(a.set_bits) + 31) // 32:
                    raise ValueError(f"atom {i}: a set of {a.set_bits} bits needs {(int(a.set_bits) + 31) // 32} words")
                keep.append(words)
                arr[i].set = words.ctypes.data if words.size else None
        h = C.c_void_p()
        _ffi.check(self._lib.ts_meta_eval(self._h, arr, len(atoms), C.byref(h), C.c_void_p(stream)))
        return RowSet(h)

    @staticmethod
    def _program_key(atoms) -> tuple:
        """A program as a hashable value: equal filter states compile to equal keys."""
        return tuple((int(a.kind), int(a.col), int(a.lo), int(a.hi), int(a.negate), int(a.group), int(a.set_bits),
                      None if a.set is None else np.ascontiguousarray(a.set, dtype=np.uint32).tobytes()) for a in atoms)

    def eval_many(self, states, stream: int = 0):
        """One `RowSet` per DISTINCT program of ``states`` (filter states or programs, one per session) and the ``which``
        array that names each session's set: ``(rowsets, which)`` as `TheoremIndex.search_rowsets` takes them.  Sessions with
        the same sidebar state share a set (a ``None`` state is "no filter": ``which`` = -1).  At most 256 distinct states per
        call (``ts_search_rowsets``' limit), else ``ValueError`` - before anything is evaluated."""
        programs, keys, which = [], {}, []
        for st in states:
            if st is None:
                which.append(-1)
                continue
            atoms = self.compile(st) if isinstance(st, Mapping) else list(st)
            key = self._program_key(atoms)
            if key not in keys:
                if len(programs) == _ffi.TS_MAX_ROWSETS:
                    raise ValueError(f"more than {_ffi.TS_MAX_ROWSETS} distinct filter states in one call: split the batch")
                keys[key] = len(programs)
                programs.append(atoms)
            which.append(keys[key])
        return [self.eval(atoms, stream=stream) for atoms in programs], np.asarray(which, dtype=np.int32)

    def exclude(self, column, codes, rows=(), base: Optional[RowSet] = None, stream: int = 0) -> RowSet:
        """``base AND NOT (the row's code in column `column` is in codes) AND NOT (the row is in rows)`` as a `RowSet`
        (``ts_rowset_exclude``): "hide these papers", and the mask the grouped search's last stage runs behind.  ``column``: a
        name or a number; ``codes``: up to 256 int32 codes (`NULL` is not one: NULL rows are excluded by row); ``rows``: up to
        256 local rows; neither needs to be sorted or unique.  ``base`` None: every row."""
        if self._lib is None or not self._h.value:
            raise ValueError("this MetaTable only encodes (device=None): there is no host evaluator")
        col = self.col[column] if isinstance(column, str) else int(column)
        c = np.ascontiguousarray(np.asarray(list(codes), dtype=np.int32).reshape(-1))
        r = np.ascontiguousarray(np.asarray(list(rows), dtype=np.int64).reshape(-1))
        h = C.c_void_p()
        _ffi.check(self._lib.ts_rowset_exclude(self._h, col, base.handle if base is not None else None,
                                               _ffi.as_ptr(c) if c.size else None, c.shape[0],
                                               _ffi.as_ptr(r) if r.size else None, r.shape[0], C.byref(h), C.c_void_p(stream)))
        return RowSet(h)

    # -- lifetime -----------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _ffi.check(self._lib.ts_meta_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
