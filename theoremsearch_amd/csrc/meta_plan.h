// The metadata filter's host decisions (meta.hip) as pure functions of plain values: the words and the rounded allocation of a
// row mask, the launch shape for n rows, the validation of a program against the kinds of a table's columns, the packing of
// its atoms into groups and of its sets into one buffer.  No handle, no HIP call, nothing from HIP: the C ABI's codes
// (include/tsearch.h, plain C) and the standard library only, so tests/meta_plan_check.cpp runs all of it on the CPU under the
// host sanitizers.  (Scan or matrix path behind a row set: scan_plan.h, AlgoInputs::allowed_known.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/tsearch.h"

namespace ts {

constexpr int kMetaThreads = 256;         // one lane per row: a workgroup takes a block of 256 rows per step, four waves of 64
constexpr int kMetaBlockRows = 256;       // masks are allocated in whole blocks of this many rows
constexpr int kMetaGridPerCU = 8;

enum MetaColKind { kMetaColUnset = 0, kMetaColScalar = 1, kMetaColList = 2 };

// ---------------------------------------------------------------------------------------------
// the mask of n rows
// ---------------------------------------------------------------------------------------------
inline int64_t mask_words(int64_t n) { return (n + 31) / 32; }                    // what a caller of ts_search_filtered hands over
inline int64_t mask_blocks(int64_t n) { return std::max<int64_t>(1, (n + kMetaBlockRows - 1) / kMetaBlockRows); }
inline int64_t mask_alloc_words(int64_t n) { return mask_blocks(n) * (kMetaBlockRows / 32); }   // what a row set allocates (and the kernel writes)

// workgroups of the evaluator: each walks the blocks blockIdx.x, blockIdx.x + grid, ...
inline int meta_grid(int cu_count, int64_t n) {
    return (int)std::min<int64_t>(mask_blocks(n), (int64_t)std::max(1, cu_count) * kMetaGridPerCU);
}

// ---------------------------------------------------------------------------------------------
// a program
// ---------------------------------------------------------------------------------------------
struct MetaAtom {           // one atom as the kernel reads it
    int32_t kind, col, lo, hi;
    int32_t negate;
    int32_t slot;           // its group: bit `slot` of a row's 16 verdicts
    int64_t set_off;        // first word of its set in the packed buffer
    uint32_t set_bits;
};
struct MetaProgram {
    const char* invalid;    // not NULL: TS_ERR_INVALID with this text, about atom `bad_atom` (-1: the program as a whole)
    int bad_atom;
    int natoms, ngroups;
    MetaAtom atom[TS_META_MAX_ATOMS];
    int32_t group_of_slot[TS_META_MAX_GROUPS];   // the caller's group value of each slot, in the order of first appearance
    int64_t set_words;      // words of the packed sets
};

inline int64_t set_words_of(int64_t set_bits) { return (set_bits + 31) / 32; }

// Validates `atoms` against the kinds of the table's columns and lays the program out.  Groups get slots in the order in
// which their values first appear; sets are packed back to back, whole words each, in atom order.
inline MetaProgram meta_plan(const int* col_kind, int ncols, const ts_atom* atoms, int natoms) {
    MetaProgram p;
    memset(&p, 0, sizeof(p));
    p.bad_atom = -1;
    auto bad = [&p](int i, const char* text) { p.invalid = text; p.bad_atom = i; return p; };
    if (natoms < 0 || natoms > TS_META_MAX_ATOMS) return bad(-1, "a program has at most 32 atoms");
    if (natoms > 0 && !atoms) return bad(-1, "atoms is NULL");
    for (int i = 0; i < natoms; ++i) {
        const ts_atom& a = atoms[i];
        if (a.kind < TS_ATOM_RANGE || a.kind > TS_ATOM_IS_NULL) return bad(i, "atom kind out of range");
        if (a.col < 0 || a.col >= ncols) return bad(i, "column out of range");
        if (col_kind[a.col] == kMetaColUnset) return bad(i, "the column was never set");
        const bool list = a.kind == TS_ATOM_ANY_IN;
        if (list && col_kind[a.col] != kMetaColList) return bad(i, "ANY_IN needs a list column");
        if (!list && col_kind[a.col] != kMetaColScalar) return bad(i, "RANGE, IN and IS_NULL need a scalar column");
        if (a.negate != 0 && a.negate != 1) return bad(i, "negate is 0 or 1");
        if (list && a.negate) return bad(i, "ANY_IN cannot be negated");
        if (a.kind == TS_ATOM_RANGE && a.lo > a.hi) return bad(i, "lo > hi");
        const bool has_set = a.kind == TS_ATOM_IN || a.kind == TS_ATOM_ANY_IN;
        if (has_set && (a.set_bits < 0 || a.set_bits > INT32_MAX)) return bad(i, "set_bits outside [0, INT32_MAX]");
        if (has_set && a.set_bits > 0 && !a.set) return bad(i, "the set is missing");
        int slot = 0;
        while (slot < p.ngroups && p.group_of_slot[slot] != a.group) ++slot;
        if (slot == p.ngroups) {
            if (p.ngroups == TS_META_MAX_GROUPS) return bad(i, "a program has at most 16 groups");
            p.group_of_slot[p.ngroups++] = a.group;
        }
        MetaAtom& m = p.atom[i];
        m.kind = a.kind;
        m.col = a.col;
        m.lo = a.lo;
        m.hi = a.hi;
        m.negate = a.negate;
        m.slot = slot;
        m.set_off = p.set_words;
        m.set_bits = has_set ? (uint32_t)a.set_bits : 0u;
        if (has_set) p.set_words += set_words_of(a.set_bits);
    }
    p.natoms = natoms;
    return p;
}

// The packed sets of a valid program: `out` holds p.set_words words.  Bits past set_bits in a set's last word are cleared
// (the kernel tests the code against set_bits first; the buffer then depends on the sets alone, not on what lies behind them).
inline void meta_pack_sets(const MetaProgram& p, const ts_atom* atoms, uint32_t* out) {
    for (int i = 0; i < p.natoms; ++i) {
        const MetaAtom& m = p.atom[i];
        const int64_t words = set_words_of(m.set_bits);
        if (words == 0) continue;
        memcpy(out + m.set_off, atoms[i].set, (size_t)words * 4);
        const int tail = (int)(words * 32 - m.set_bits);
        if (tail > 0) out[m.set_off + words - 1] &= 0xFFFFFFFFu >> tail;
    }
}

// verdicts of all groups: a row passes when its 16 verdict bits equal this
inline uint32_t meta_all_groups(int ngroups) { return ngroups >= 32 ? 0xFFFFFFFFu : ((1u << ngroups) - 1u); }

}  // namespace ts
