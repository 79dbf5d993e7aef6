"""A vectorised numpy model of the metadata filter's atom semantics (include/tsearch.h), random columns and random programs:
the reference of the CPU and GPU metadata tests.  It reads a program (a list of `metadata.Atom`) and the columns as
`MetaTable.columns` holds them - int32[n] per scalar column, (offsets, codes) per list column - and nothing of the library."""
import numpy as np

from theoremsearch_amd.metadata import ANY_IN, IN, IS_NULL, NULL, RANGE, Atom, code_set

I32_MAX = 2**31 - 1


def set_contains(words, set_bits, codes):
    """bool per code: 0 <= code < set_bits and its bit is set in the uint32 words."""
    codes = np.asarray(codes, dtype=np.int64)
    ok = (codes >= 0) & (codes < set_bits)
    safe = np.where(ok, codes, 0)
    words = np.asarray(words, dtype=np.uint32)
    if words.size == 0:
        return np.zeros(codes.shape, dtype=bool)
    return ok & (((words[safe >> 5] >> (safe & 31).astype(np.uint32)) & 1) == 1)


def atom_truth(atom, columns, n):
    """bool[n]: where the atom is TRUE."""
    if atom.kind == ANY_IN:
        assert not atom.negate
        offsets, codes = columns[atom.col]
        hit = set_contains(atom.set, atom.set_bits, codes).astype(np.int64)
        csum = np.concatenate([[0], np.cumsum(hit)])
        return (csum[offsets[1:]] - csum[offsets[:-1]]) > 0
    v = np.asarray(columns[atom.col], dtype=np.int64)
    null = v == NULL
    if atom.kind == IS_NULL:
        return null != bool(atom.negate)
    inside = (atom.lo <= v) & (v <= atom.hi) if atom.kind == RANGE else set_contains(atom.set, atom.set_bits, v)
    return ~null & (inside != bool(atom.negate))


def model_mask(atoms, columns, n):
    """bool[n]: every group holds, a group holds when one of its atoms is true; the empty program allows every row."""
    groups = {}
    for a in atoms:
        t = atom_truth(a, columns, n)
        groups[a.group] = groups[a.group] | t if a.group in groups else t
    out = np.ones(n, dtype=bool)
    for t in groups.values():
        out &= t
    return out


# ---- random tables and programs --------------------------------------------------------------------------------------------
N_SCALAR, LIST_COL = 5, 5
WIDE_BITS = 100_000          # column 4 holds codes up to here: the one large set


def random_columns(n, seed=21):
    """Five scalar columns and a list column: small codes with NULLs and codes below 0; years; counts with NULLs; values at the
    ends of int32; wide codes (some at or above every set's set_bits); lists of 0 .. 40 codes."""
    rng = np.random.default_rng(seed)
    c0 = rng.integers(-2, 12, n).astype(np.int32)
    c0[rng.random(n) < 0.1] = NULL
    c1 = rng.integers(1990, 2030, n).astype(np.int32)
    c2 = rng.integers(0, 300, n).astype(np.int32)
    c2[rng.random(n) < 0.2] = NULL
    c3 = rng.choice(np.array([NULL, NULL + 1, -1, 0, 1, I32_MAX - 1, I32_MAX], dtype=np.int64), n).astype(np.int32)
    c4 = rng.integers(0, WIDE_BITS + 500, n).astype(np.int32)
    lens = rng.choice(np.array([0, 0, 1, 2, 3, 5, 40]), n)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    codes = rng.integers(0, 70, int(offsets[-1])).astype(np.int32)
    return [c0, c1, c2, c3, c4, (offsets, codes)]


def random_set(rng, nbits, density=0.3):
    return code_set(np.flatnonzero(rng.random(nbits) < density), nbits), nbits


def random_atom(rng, group):
    kind = int(rng.integers(0, 4))
    if kind == ANY_IN:
        words, bits = random_set(rng, int(rng.choice([1, 33, 64, 70, 90])))
        return Atom(ANY_IN, LIST_COL, group=group, set=words, set_bits=bits)
    negate = int(rng.integers(0, 2))
    if kind == IS_NULL:
        return Atom(IS_NULL, int(rng.choice([0, 2, 3])), negate=negate, group=group)
    if kind == RANGE:
        col = int(rng.integers(0, 4))
        lo, hi = {0: (2, 7), 1: (2000, 2015), 2: (50, 250), 3: (NULL + 1, I32_MAX)}[col]
        if col == 3 and rng.random() < 0.5:
            lo, hi = (-1, 1)
        return Atom(RANGE, col, lo, hi, negate=negate, group=group)
    col = int(rng.choice([0, 2, 3]))
    words, bits = random_set(rng, {0: 8, 2: 257, 3: 32}[col], 0.5)      # column 0 has codes -2, -1 and 8 .. 11 outside it
    return Atom(IN, col, negate=negate, group=group, set=words, set_bits=bits)


def random_programs(count=50, seed=33):
    """`count` programs: the empty one, one of 32 atoms in 16 groups, one with the set of WIDE_BITS bits, the full int32 range,
    and random ones of 1 .. 12 atoms in 1 .. 5 groups (a single-atom group is the selective case, a large group the dense)."""
    rng = np.random.default_rng(seed)
    progs = [[]]
    progs.append([random_atom(rng, g // 2) for g in range(32)])
    wide, bits = random_set(rng, WIDE_BITS, 0.5)
    progs.append([Atom(IN, 4, group=0, set=wide, set_bits=bits), Atom(IS_NULL, 0, group=0)])
    progs.append([Atom(IN, 4, negate=1, group=5, set=wide, set_bits=bits)])
    progs.append([Atom(RANGE, 3, NULL + 1, I32_MAX, group=0)])
    progs.append([Atom(RANGE, 3, NULL + 1, I32_MAX, negate=1, group=0), Atom(IS_NULL, 3, group=0)])
    progs.append([Atom(IN, 0, group=0, set=np.zeros(0, dtype=np.uint32), set_bits=0)])
    while len(progs) < count:
        ngroups = int(rng.integers(1, 6))
        natoms = int(rng.integers(ngroups, 13))
        groups = list(range(ngroups)) + [int(g) for g in rng.integers(0, ngroups, natoms - ngroups)]
        progs.append([random_atom(rng, 7 * g - 3) for g in groups])
    return progs
