// Stand-alone check of theoremsearch_amd/csrc/meta_plan.h, the metadata filter's host decisions, and of the row-set field of
// scan_plan.h's AlgoInputs (tests/test_meta_plan_cpu.py builds it with the host compiler under -fsanitize=address,undefined
// and runs it).  Exit 0 = every check held; otherwise each failed check is printed.
#include "bias_plan.h"
#include "meta_plan.h"

#include <cstdio>
#include <vector>

using namespace ts;

static int g_failed = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++g_failed <= 40) {                        \
                printf("FAILED %s:%d: %s  [", __func__, __LINE__, #cond); \
                printf(__VA_ARGS__);                       \
                printf("]\n");                             \
            }                                              \
        }                                                  \
    } while (0)

static void mask_shape() {
    const struct { int64_t n, words, alloc; } want[] = {{1, 1, 8},   {31, 1, 8},  {32, 1, 8},   {33, 2, 8},
                                                       {255, 8, 8}, {256, 8, 8}, {257, 9, 16}, {0, 0, 8}, {10000000, 312500, 312504}};
    for (const auto& w : want) {
        CHECK(mask_words(w.n) == w.words, "n %lld: %lld words", (long long)w.n, (long long)mask_words(w.n));
        CHECK(mask_alloc_words(w.n) == w.alloc, "n %lld: %lld words allocated", (long long)w.n, (long long)mask_alloc_words(w.n));
        CHECK(mask_alloc_words(w.n) >= mask_words(w.n) && mask_alloc_words(w.n) % (kMetaBlockRows / 32) == 0, "n %lld", (long long)w.n);
        CHECK(mask_blocks(w.n) * kMetaBlockRows >= w.n && mask_blocks(w.n) * (kMetaBlockRows / 32) == mask_alloc_words(w.n), "n %lld", (long long)w.n);
    }
    // the launch: one workgroup per block until the grid is full, never none, never more blocks than there are
    CHECK(kMetaThreads == kMetaBlockRows, "one lane per row of a block");
    CHECK(meta_grid(256, 1) == 1 && meta_grid(256, 256) == 1 && meta_grid(256, 257) == 2, "small tables");
    CHECK(meta_grid(256, 0) == 1, "an empty table still zeroes its block");
    CHECK(meta_grid(256, 10000000) == 256 * kMetaGridPerCU && meta_grid(0, 10000000) == kMetaGridPerCU, "the grid is capped");
    CHECK(meta_grid(256, 2048 * 256) == 2048 && meta_grid(256, 2047 * 256) == 2047 && meta_grid(256, 2047 * 256 + 1) == 2048, "at the cap");
}

static ts_atom atom(int kind, int col, int lo, int hi, int negate, int group, const uint32_t* set = nullptr, int64_t set_bits = 0) {
    ts_atom a;
    memset(&a, 0, sizeof(a));
    a.kind = kind;
    a.col = col;
    a.lo = lo;
    a.hi = hi;
    a.negate = negate;
    a.group = group;
    a.set = set;
    a.set_bits = set_bits;
    return a;
}

static void refusals() {
    // columns: 0 scalar, 1 list, 2 never set
    const int kinds[3] = {kMetaColScalar, kMetaColList, kMetaColUnset};
    const uint32_t set[2] = {0x5u, 0x1u};
    auto refused = [&](const ts_atom& a, const char* text) {
        const MetaProgram p = meta_plan(kinds, 3, &a, 1);
        return p.invalid && !strcmp(p.invalid, text) && p.bad_atom == 0;
    };
    auto accepted = [&](const ts_atom& a) { return meta_plan(kinds, 3, &a, 1).invalid == nullptr; };
    CHECK(accepted(atom(TS_ATOM_RANGE, 0, 1, 1, 0, 0)) && accepted(atom(TS_ATOM_RANGE, 0, INT32_MIN + 1, INT32_MAX, 1, 0)), "ranges");
    CHECK(accepted(atom(TS_ATOM_IN, 0, 0, 0, 1, 0, set, 33)) && accepted(atom(TS_ATOM_ANY_IN, 1, 0, 0, 0, 0, set, 33)), "sets");
    CHECK(accepted(atom(TS_ATOM_IS_NULL, 0, 0, 0, 1, 0)) && accepted(atom(TS_ATOM_IS_NULL, 0, 5, 1, 0, 0)), "IS_NULL reads neither lo nor hi");
    CHECK(accepted(atom(TS_ATOM_IN, 0, 0, 0, 0, 0, nullptr, 0)), "the empty set needs no words");
    CHECK(refused(atom(-1, 0, 0, 0, 0, 0), "atom kind out of range") && refused(atom(4, 0, 0, 0, 0, 0), "atom kind out of range"), "kind");
    CHECK(refused(atom(TS_ATOM_RANGE, -1, 0, 0, 0, 0), "column out of range") && refused(atom(TS_ATOM_RANGE, 3, 0, 0, 0, 0), "column out of range"), "column");
    CHECK(refused(atom(TS_ATOM_RANGE, 2, 0, 0, 0, 0), "the column was never set") && refused(atom(TS_ATOM_ANY_IN, 2, 0, 0, 0, 0, set, 33), "the column was never set"), "unset");
    CHECK(refused(atom(TS_ATOM_ANY_IN, 0, 0, 0, 0, 0, set, 33), "ANY_IN needs a list column"), "ANY_IN on a scalar column");
    for (int kind : {TS_ATOM_RANGE, TS_ATOM_IN, TS_ATOM_IS_NULL})
        CHECK(refused(atom(kind, 1, 0, 0, 0, 0, set, 33), "RANGE, IN and IS_NULL need a scalar column"), "kind %d on a list column", kind);
    CHECK(refused(atom(TS_ATOM_RANGE, 0, 0, 0, 2, 0), "negate is 0 or 1") && refused(atom(TS_ATOM_RANGE, 0, 0, 0, -1, 0), "negate is 0 or 1"), "negate");
    CHECK(refused(atom(TS_ATOM_ANY_IN, 1, 0, 0, 1, 0, set, 33), "ANY_IN cannot be negated"), "negated ANY_IN");
    CHECK(refused(atom(TS_ATOM_RANGE, 0, 2, 1, 0, 0), "lo > hi"), "lo > hi");
    CHECK(refused(atom(TS_ATOM_IN, 0, 0, 0, 0, 0, nullptr, 33), "the set is missing") && refused(atom(TS_ATOM_ANY_IN, 1, 0, 0, 0, 0, nullptr, 1), "the set is missing"), "no set");
    CHECK(refused(atom(TS_ATOM_IN, 0, 0, 0, 0, 0, set, -1), "set_bits outside [0, INT32_MAX]") &&
          refused(atom(TS_ATOM_IN, 0, 0, 0, 0, 0, set, (int64_t)INT32_MAX + 1), "set_bits outside [0, INT32_MAX]"), "set_bits");
    // the program as a whole
    std::vector<ts_atom> many(33, atom(TS_ATOM_RANGE, 0, 0, 9, 0, 0));
    MetaProgram p = meta_plan(kinds, 3, many.data(), 33);
    CHECK(p.invalid && !strcmp(p.invalid, "a program has at most 32 atoms") && p.bad_atom == -1, "33 atoms");
    CHECK(meta_plan(kinds, 3, many.data(), 32).invalid == nullptr, "32 atoms");
    CHECK(meta_plan(kinds, 3, many.data(), -1).invalid != nullptr, "a negative count");
    p = meta_plan(kinds, 3, nullptr, 1);
    CHECK(p.invalid && !strcmp(p.invalid, "atoms is NULL"), "no atoms");
    for (int i = 0; i < 17; ++i) many[i].group = 100 - i;
    p = meta_plan(kinds, 3, many.data(), 17);
    CHECK(p.invalid && !strcmp(p.invalid, "a program has at most 16 groups") && p.bad_atom == 16, "17 groups");
    CHECK(meta_plan(kinds, 3, many.data(), 16).invalid == nullptr && meta_plan(kinds, 3, many.data(), 16).ngroups == 16, "16 groups");
    // the bad atom is named
    many.assign(5, atom(TS_ATOM_RANGE, 0, 0, 9, 0, 0));
    many[3].lo = 10;
    p = meta_plan(kinds, 3, many.data(), 5);
    CHECK(p.invalid && p.bad_atom == 3, "atom %d", p.bad_atom);
    // the empty program
    p = meta_plan(kinds, 3, nullptr, 0);
    CHECK(!p.invalid && p.natoms == 0 && p.ngroups == 0 && p.set_words == 0 && meta_all_groups(p.ngroups) == 0, "the empty program");
}

static void groups_and_sets() {
    const int kinds[2] = {kMetaColScalar, kMetaColList};
    // the bits past set_bits of a set's last word are not the set's
    const uint32_t a33[2] = {0x80000001u, 0xFFFFFFFFu};      // 33 bits: {0, 31, 32}
    const uint32_t b64[2] = {0x2u, 0x80000000u};             // 64 bits: {1, 63}
    const uint32_t c5[1] = {0xFFu};                           // 5 bits: {0 .. 4}
    const ts_atom atoms[6] = {atom(TS_ATOM_IN, 0, 0, 0, 0, 7, a33, 33),   atom(TS_ATOM_RANGE, 0, 3, 4, 1, -2),
                              atom(TS_ATOM_ANY_IN, 1, 0, 0, 0, 7, b64, 64), atom(TS_ATOM_IS_NULL, 0, 0, 0, 0, 0),
                              atom(TS_ATOM_IN, 0, 0, 0, 1, -2, c5, 5),    atom(TS_ATOM_IN, 0, 0, 0, 0, 0, nullptr, 0)};
    const MetaProgram p = meta_plan(kinds, 2, atoms, 6);
    CHECK(!p.invalid && p.natoms == 6 && p.ngroups == 3, "%d groups", p.ngroups);
    if (p.invalid) return;
    // slots in the order of first appearance: 7 -> 0, -2 -> 1, 0 -> 2
    const int want_slot[6] = {0, 1, 0, 2, 1, 2};
    for (int i = 0; i < 6; ++i) {
        CHECK(p.atom[i].slot == want_slot[i], "atom %d: slot %d", i, p.atom[i].slot);
        CHECK(p.atom[i].kind == atoms[i].kind && p.atom[i].col == atoms[i].col && p.atom[i].lo == atoms[i].lo && p.atom[i].hi == atoms[i].hi &&
              p.atom[i].negate == atoms[i].negate, "atom %d", i);
    }
    CHECK(p.group_of_slot[0] == 7 && p.group_of_slot[1] == -2 && p.group_of_slot[2] == 0, "group values");
    CHECK(meta_all_groups(3) == 7u && meta_all_groups(16) == 0xFFFFu && meta_all_groups(1) == 1u, "verdict bits");
    // sets back to back, whole words each, in atom order; atoms without a set take none
    CHECK(p.atom[0].set_off == 0 && p.atom[2].set_off == 2 && p.atom[4].set_off == 4 && p.set_words == 5, "%lld words", (long long)p.set_words);
    CHECK(p.atom[0].set_bits == 33 && p.atom[2].set_bits == 64 && p.atom[4].set_bits == 5 && p.atom[1].set_bits == 0 && p.atom[5].set_bits == 0, "set_bits");
    CHECK(p.atom[5].set_off == 5, "the empty set lies at the end and has no words");
    std::vector<uint32_t> packed((size_t)p.set_words, 0xDEADBEEFu);
    meta_pack_sets(p, atoms, packed.data());
    const uint32_t want[5] = {0x80000001u, 0x1u, 0x2u, 0x80000000u, 0x1Fu};
    for (int w = 0; w < 5; ++w) CHECK(packed[w] == want[w], "word %d: %08x", w, packed[w]);
    CHECK(set_words_of(0) == 0 && set_words_of(1) == 1 && set_words_of(32) == 1 && set_words_of(33) == 2 && set_words_of(100000) == 3125, "set words");
}

static AlgoInputs batch(int algo, int64_t n, int64_t allowed) {     // 256 queries behind a device mask, on an index the matrix path serves
    AlgoInputs in;
    memset(&in, 0, sizeof(in));
    in.algo = algo;
    in.mfma_ok = true;
    in.n = n;
    in.nq = 256;
    in.k = 10;
    in.mfma_min_rows = 16384;
    in.scan_max_queries = 4;
    in.mask = in.mask_on_device = true;
    in.allowed = allowed;
    return in;
}

static void known_counts() {
    const char* kMask = "the MFMA path serves host masks that keep at least a tenth of the rows, for more than 4 queries";
    const int64_t n = 1000000;
    for (const bool biased : {false, true}) {
        // the plain search decides with choose_algo, the biased one (ts_search_biased_ex) with choose_bias_algo on a served index
        auto choose = [&](AlgoInputs in) {
            in.bias = biased;
            return biased ? choose_bias_algo(in, true) : choose_algo(in);
        };
        for (const int algo : {TS_ALGO_AUTO, TS_ALGO_SCAN, TS_ALGO_MFMA}) {
            // the field at its default: a device mask is decided as before, whatever `allowed` says
            for (const int64_t allowed : {(int64_t)0, n / 10 - 1, n / 10, n}) {
                const AlgoChoice c = choose(batch(algo, n, allowed));
                if (algo == TS_ALGO_MFMA) CHECK(c.unsupported && !strcmp(c.unsupported, kMask), "biased %d allowed %lld", (int)biased, (long long)allowed);
                else CHECK(!c.unsupported && c.algo == TS_ALGO_SCAN, "biased %d algo %d allowed %lld -> %d", (int)biased, algo, (long long)allowed, c.algo);
                CHECK(!mask_wants_count(batch(algo, n, allowed)), "a device mask is never counted on the host");
            }
            // the count known: just below a tenth, at a tenth, all rows, none
            for (const int64_t allowed : {(int64_t)0, n / 10 - 1, n / 10, n}) {
                AlgoInputs in = batch(algo, n, allowed);
                in.allowed_known = true;
                const AlgoChoice c = choose(in);
                const bool dense = allowed * 10 >= n;
                CHECK(!mask_wants_count(in), "nothing to count");
                if (algo == TS_ALGO_SCAN) CHECK(!c.unsupported && c.algo == TS_ALGO_SCAN, "biased %d allowed %lld", (int)biased, (long long)allowed);
                else if (dense) CHECK(!c.unsupported && c.algo == TS_ALGO_MFMA, "biased %d algo %d allowed %lld", (int)biased, algo, (long long)allowed);
                else if (algo == TS_ALGO_MFMA) CHECK(c.unsupported && !strcmp(c.unsupported, kMask), "biased %d allowed %lld", (int)biased, (long long)allowed);
                else CHECK(!c.unsupported && c.algo == TS_ALGO_SCAN, "biased %d allowed %lld -> %d", (int)biased, (long long)allowed, c.algo);
                // exactly what a counted host mask of that density gets
                AlgoInputs host = in;
                host.mask_on_device = host.allowed_known = false;
                const AlgoChoice h = choose(host);
                CHECK((c.unsupported != nullptr) == (h.unsupported != nullptr) && (c.unsupported || c.algo == h.algo), "biased %d algo %d allowed %lld", (int)biased, algo, (long long)allowed);
            }
        }
        // a known count does not make a batch: four queries, a small index, an index without matrix kernels stay on the scan
        AlgoInputs in = batch(TS_ALGO_AUTO, n, n);
        in.allowed_known = true;
        in.nq = 4;
        CHECK(choose(in).algo == TS_ALGO_SCAN && !choose(in).unsupported, "biased %d: 4 queries", (int)biased);
        in.algo = TS_ALGO_MFMA;
        CHECK(choose(in).unsupported != nullptr, "biased %d: algo = mfma, 4 queries", (int)biased);
        in = batch(TS_ALGO_AUTO, 16383, 16383);
        in.allowed_known = true;
        CHECK(choose(in).algo == TS_ALGO_SCAN && !choose(in).unsupported, "biased %d: below TS_MFMA_MIN_ROWS", (int)biased);
    }
    // the field means nothing without a device mask: a host mask is counted as ever, no mask is no mask
    AlgoInputs in = batch(TS_ALGO_AUTO, n, n / 10 - 1);
    in.mask_on_device = false;
    in.allowed_known = true;
    CHECK(mask_wants_count(in) && choose_algo(in).algo == TS_ALGO_SCAN, "a sparse host mask");
    in.mask = false;
    CHECK(choose_algo(in).algo == TS_ALGO_MFMA, "no mask");
    // ts_search_biased (not _ex: choose_algo with bias) keeps the scan behind a row set too
    in = batch(TS_ALGO_AUTO, n, n);
    in.allowed_known = in.bias = true;
    CHECK(choose_algo(in).algo == TS_ALGO_SCAN && !choose_algo(in).unsupported, "the scan-only biased search");
}

int main() {
    mask_shape();
    refusals();
    groups_and_sets();
    known_counts();
    if (g_failed) printf("meta_plan_check: %d checks FAILED\n", g_failed);
    else printf("meta_plan_check: all checks passed\n");
    return g_failed ? 1 : 0;
}
