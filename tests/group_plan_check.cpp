// Stand-alone check of theoremsearch_amd/csrc/group_plan.h, the grouped search's host decisions (tests/test_group_plan_cpu.py
// builds it with the host compiler under -fsanitize=address,undefined and runs it).  Exit 0 = every check held; otherwise each
// failed check is printed.
#include "group_plan.h"

#include <cstdio>
#include <cstring>
#include <random>
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

static bool says(const char* text, const char* part) { return text && strstr(text, part); }

// the depth rule for every k: first = min(256, max(2 k, k + 16))
static void depths() {
    CHECK(group_deep_depth() == TS_MAX_K, "deep = %d", group_deep_depth());
    int prev = 0;
    for (int k = 1; k <= TS_MAX_K; ++k) {
        const int first = group_first_depth(k);
        CHECK(first >= k && first <= TS_MAX_K, "k %d: first %d", k, first);
        CHECK(first >= prev, "k %d: first %d after %d", k, first, prev);
        CHECK((first <= 64) == (k <= 32), "k %d: first %d", k, first);
        CHECK(first == (2 * k > k + 16 ? 2 * k : k + 16) || first == TS_MAX_K, "k %d: first %d", k, first);
        CHECK((first == group_deep_depth()) == (k >= 128), "k %d: first %d", k, first);
        CHECK(group_has_deep_stage(k) == (first < group_deep_depth()), "k %d", k);
        CHECK(first - k >= (k <= 240 ? 16 : TS_MAX_K - k), "k %d: slack %d", k, first - k);
        prev = first;
    }
    CHECK(group_first_depth(1) == 17 && group_first_depth(10) == 26 && group_first_depth(16) == 32 && group_first_depth(17) == 34, "small k");
    CHECK(group_first_depth(32) == 64 && group_first_depth(33) == 66 && group_first_depth(100) == 200, "middle k");
    CHECK(group_first_depth(127) == 254 && group_first_depth(128) == 256 && group_first_depth(256) == 256, "large k");
    CHECK(!group_depth_invalid(1) && !group_depth_invalid(TS_MAX_K), "the ends are valid");
    CHECK(says(group_depth_invalid(0), "k outside") && says(group_depth_invalid(-1), "k outside") && says(group_depth_invalid(TS_MAX_K + 1), "k outside"), "k out of range");
}

static void certificate() {
    for (int k_out = 1; k_out <= TS_MAX_K; k_out += 5)
        for (int found = 0; found <= TS_MAX_K; ++found) {
            CHECK(group_certified(found, k_out, false) == (found >= k_out), "found %d of %d, a full list", found, k_out);
            CHECK(group_certified(found, k_out, true), "found %d of %d, a list with padding", found, k_out);
        }
    CHECK(!group_certified(0, 1, false) && group_certified(0, 1, true) && group_certified(1, 1, false), "k_out = 1");
}

template <class T>
static void membership_of(std::mt19937_64& rng, int count, T lo, T hi) {
    std::uniform_int_distribution<long long> pick((long long)lo, (long long)hi);
    std::vector<T> raw((size_t)count);
    for (T& v : raw) v = (T)pick(rng);
    for (int i = 0; i + 1 < count; i += 3) raw[(size_t)i + 1] = raw[(size_t)i];        // duplicates before sorting
    std::vector<T> list = raw;
    const int n = sort_unique(list.data(), count);
    CHECK(n <= count && (count == 0 || n >= 1), "%d of %d left", n, count);
    for (int i = 0; i + 1 < n; ++i) CHECK(list[(size_t)i] < list[(size_t)i + 1], "position %d not strictly ascending", i);
    auto linear = [&](T v) {
        for (T x : raw)
            if (x == v) return true;
        return false;
    };
    // every member, its neighbours, the ends of the type's range in use, random values
    std::vector<T> probes = {lo, hi, (T)0, (T)-1, (T)1};
    for (T v : raw) { probes.push_back(v); probes.push_back((T)(v - 1)); probes.push_back((T)(v + 1)); }
    for (int i = 0; i < 200; ++i) probes.push_back((T)pick(rng));
    std::vector<T> dup = raw;                   // the sorted list with its duplicates kept is searched the same way
    std::sort(dup.begin(), dup.end());
    for (T v : probes) {
        CHECK(sorted_has(list.data(), n, v) == linear(v), "count %d: value %lld", count, (long long)v);
        CHECK(sorted_has(dup.data(), count, v) == linear(v), "count %d with duplicates: value %lld", count, (long long)v);
    }
    CHECK(!sorted_has((const T*)nullptr, 0, (T)5), "the empty list holds nothing");
}

static void membership() {
    std::mt19937_64 rng(20260101);
    for (int count : {0, 1, 255, 256})
        for (int rep = 0; rep < 4; ++rep) {
            membership_of<int32_t>(rng, count, -40, 40);                                   // dense: many hits, negative codes
            membership_of<int32_t>(rng, count, INT32_MIN + 2, INT32_MAX - 1);               // the whole range
            membership_of<int64_t>(rng, count, 0, 3000);
            membership_of<int64_t>(rng, count, 0, (int64_t)0xFFFFFFF0ll);
        }
}

static void validation() {
    // ts_search_grouped
    CHECK(!grouped_args_invalid(true, true, true, true, true, TS_F32, 0, 1, TS_ALGO_AUTO), "valid");
    CHECK(!grouped_args_invalid(true, true, true, true, true, TS_BF16, 5, TS_MAX_K, TS_ALGO_MFMA), "valid");
    for (int miss = 0; miss < 5; ++miss)
        CHECK(says(grouped_args_invalid(miss != 0, miss != 1, miss != 2, miss != 3, miss != 4, TS_F32, 1, 1, TS_ALGO_AUTO), "NULL argument"), "missing %d", miss);
    CHECK(says(grouped_args_invalid(true, true, true, true, true, 2, 1, 1, TS_ALGO_AUTO), "q_dtype"), "q_dtype");
    CHECK(says(grouped_args_invalid(true, true, true, true, true, -1, 1, 1, TS_ALGO_AUTO), "q_dtype"), "q_dtype");
    CHECK(says(grouped_args_invalid(true, true, true, true, true, TS_F32, -1, 1, TS_ALGO_AUTO), "nq is negative"), "nq");
    CHECK(says(grouped_args_invalid(true, true, true, true, true, TS_F32, 1, 0, TS_ALGO_AUTO), "k outside"), "k");
    CHECK(says(grouped_args_invalid(true, true, true, true, true, TS_F32, 1, TS_MAX_K + 1, TS_ALGO_AUTO), "k outside"), "k");
    CHECK(says(grouped_args_invalid(true, true, true, true, true, TS_F32, 1, 1, 3), "algo"), "algo");
    CHECK(says(grouped_args_invalid(true, true, true, true, true, TS_F32, 1, 1, -1), "algo"), "algo");
    // ts_collapse_topk
    CHECK(!collapse_args_invalid(true, true, true, true, true, 0, 1, 1, 0, 0), "valid");
    CHECK(!collapse_args_invalid(true, true, true, true, true, 300, TS_MAX_K, 100000, 5, 1000000000), "valid: k_out has no upper limit");
    for (int miss = 0; miss < 5; ++miss)
        CHECK(says(collapse_args_invalid(miss != 0, miss != 1, miss != 2, miss != 3, miss != 4, 1, 1, 1, 1, 0), "NULL argument"), "missing %d", miss);
    CHECK(says(collapse_args_invalid(true, true, true, true, true, -1, 1, 1, 1, 0), "nq is negative"), "nq");
    CHECK(says(collapse_args_invalid(true, true, true, true, true, 1, 0, 1, 1, 0), "k_in outside"), "k_in");
    CHECK(says(collapse_args_invalid(true, true, true, true, true, 1, TS_MAX_K + 1, 1, 1, 0), "k_in outside"), "k_in");
    CHECK(says(collapse_args_invalid(true, true, true, true, true, 1, 1, 0, 1, 0), "k_out is less than 1"), "k_out");
    CHECK(says(collapse_args_invalid(true, true, true, true, true, 1, 1, 1, -1, 0), "n is negative"), "n");
    CHECK(says(collapse_args_invalid(true, true, true, true, true, 1, 1, 1, 1, -1), "row_offset is negative"), "row_offset");
    // ts_rowset_exclude
    std::vector<int32_t> codes(kGroupMaxList + 1, 7);
    std::vector<int64_t> rows(kGroupMaxList + 1, 3);
    CHECK(!exclude_args_invalid(true, true, nullptr, 0, nullptr, 0, 0), "valid: nothing excluded");
    CHECK(!exclude_args_invalid(true, true, codes.data(), kGroupMaxList, rows.data(), kGroupMaxList, 4), "valid: full lists, duplicates");
    CHECK(says(exclude_args_invalid(false, true, nullptr, 0, nullptr, 0, 0), "NULL argument"), "meta");
    CHECK(says(exclude_args_invalid(true, false, nullptr, 0, nullptr, 0, 0), "NULL argument"), "out");
    CHECK(says(exclude_args_invalid(true, true, codes.data(), kGroupMaxList + 1, nullptr, 0, 4), "ncodes outside"), "ncodes");
    CHECK(says(exclude_args_invalid(true, true, codes.data(), -1, nullptr, 0, 4), "ncodes outside"), "ncodes");
    CHECK(says(exclude_args_invalid(true, true, nullptr, 0, rows.data(), kGroupMaxList + 1, 4), "nrows outside"), "nrows");
    CHECK(says(exclude_args_invalid(true, true, nullptr, 0, rows.data(), -1, 4), "nrows outside"), "nrows");
    CHECK(says(exclude_args_invalid(true, true, nullptr, 1, nullptr, 0, 4), "codes is NULL"), "codes");
    CHECK(says(exclude_args_invalid(true, true, nullptr, 0, nullptr, 1, 4), "local_rows is NULL"), "rows");
    codes[5] = TS_META_NULL;
    CHECK(says(exclude_args_invalid(true, true, codes.data(), 10, nullptr, 0, 4), "TS_META_NULL is not a code"), "a NULL code");
    CHECK(!exclude_args_invalid(true, true, codes.data(), 5, nullptr, 0, 4), "the NULL lies behind the list");
    codes[5] = INT32_MIN + 1;
    CHECK(!exclude_args_invalid(true, true, codes.data(), 10, nullptr, 0, 4), "negative codes are codes");
    rows[2] = 4;
    CHECK(says(exclude_args_invalid(true, true, nullptr, 0, rows.data(), 3, 4), "outside [0, n)"), "row n");
    rows[2] = -1;
    CHECK(says(exclude_args_invalid(true, true, nullptr, 0, rows.data(), 3, 4), "outside [0, n)"), "row -1");
    CHECK(!exclude_args_invalid(true, true, nullptr, 0, rows.data(), 2, 4), "the bad row lies behind the list");
    CHECK(says(exclude_args_invalid(true, true, nullptr, 0, rows.data(), 1, 0), "outside [0, n)"), "an empty table has no rows");
}

int main() {
    depths();
    certificate();
    membership();
    validation();
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
