// Stand-alone check of theoremsearch_amd/csrc/dev_array.h, the library's one owner of device memory
// (tests/test_dev_array_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it).  The type is
// instantiated over malloc / free with a policy that counts live allocations, records the order of its calls and can be told to
// fail the n-th allocation: a double free, a use after free or a leak is the sanitizers' finding, a wrong order or a wrong
// state a failed CHECK.  Exit 0 = every check held.
#include "dev_array.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>

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

constexpr int kNoMem = 2;       // what the policy answers for a failed allocation (any non-zero code)
constexpr int kZeroFailed = 7;  // ... and for a failed zeroing

struct TestMem {
    static int live, allocs, fail_at, fail_zero;    // fail_at: the allocs-th allocation from now fails (1 = the next), 0 = none
    static std::string log;                         // 'a' alloc, 'x' failed alloc, 'f' free, 'z' zero
    static void start() { allocs = 0; fail_at = 0; fail_zero = 0; log.clear(); }
    static int alloc(void** p, size_t bytes) {
        if (fail_at && ++allocs == fail_at) {
            log += 'x';
            return kNoMem;
        }
        *p = malloc(bytes ? bytes : 1);
        memset(*p, 0xAB, bytes);        // fresh memory is not zero: need_zeroed has to make it so
        ++live;
        log += 'a';
        return 0;
    }
    static void free(void* p) {
        ::free(p);
        --live;
        log += 'f';
    }
    static int zero(void* p, size_t bytes) {
        log += 'z';
        if (fail_zero) return kZeroFailed;
        memset(p, 0, bytes);
        return 0;
    }
};
int TestMem::live = 0, TestMem::allocs = 0, TestMem::fail_at = 0, TestMem::fail_zero = 0;
std::string TestMem::log;

template <class T> using Arr = DevArrayOf<T, TestMem>;
#define LOG_IS(s) CHECK(TestMem::log == (s), "calls '%s'", TestMem::log.c_str())

static void need_keeps_and_grows() {
    TestMem::start();
    {
        Arr<float> a;
        CHECK(!a && a.bytes() == 0, "starts empty");
        CHECK(a.need(64) == 0 && a && a.bytes() == 64, "%zu", a.bytes());
        float* first = a;
        first[15] = 1.0f;
        LOG_IS("a");
        CHECK(a.need(64) == 0 && a.need(8) == 0 && a == first && a.bytes() == 64, "large enough: kept");
        LOG_IS("a");                    // no allocator call
        CHECK(a.need(65) == 0 && a.bytes() == 65, "%zu", a.bytes());
        LOG_IS("afa");                  // the old one is freed BEFORE the new one is allocated
        CHECK(TestMem::live == 1, "%d", TestMem::live);
        a.as<char>()[64] = 1;           // the whole new size is there (the sanitizer watches)
        a.reset();
        CHECK(!a && a.bytes() == 0 && TestMem::live == 0, "%d", TestMem::live);
        a.reset();                      // nothing to free twice
        LOG_IS("afaf");
    }
    CHECK(TestMem::live == 0, "%d", TestMem::live);
}

static void need_fails_empty_and_retries() {
    TestMem::start();
    Arr<int> a;
    CHECK(a.need(16) == 0, "first");
    TestMem::allocs = 0;
    TestMem::fail_at = 1;
    CHECK(a.need(32) == kNoMem, "the policy's code comes back");
    CHECK(!a && a.bytes() == 0 && TestMem::live == 0, "empty, size 0, the old one gone: live %d", TestMem::live);
    LOG_IS("afx");
    TestMem::fail_at = 0;
    CHECK(a.need(32) == 0 && a && a.bytes() == 32, "the next call tries again");
    LOG_IS("afxa");
    // a failure on an empty buffer: still empty
    Arr<int> b;
    TestMem::allocs = 0;
    TestMem::fail_at = 1;
    CHECK(b.need(8) == kNoMem && !b && b.bytes() == 0, "empty stays empty");
    TestMem::fail_at = 0;
}

static void need_zeroed_zeroes_fresh_only() {
    TestMem::start();
    Arr<unsigned char> a;
    bool zeroing = true;
    CHECK(a.need_zeroed(48, &zeroing) == 0 && !zeroing, "fresh");
    LOG_IS("az");
    bool all0 = true;
    for (int i = 0; i < 48; ++i) all0 = all0 && a[i] == 0;
    CHECK(all0, "a fresh allocation is zeroed");
    a[5] = 9;
    CHECK(a.need_zeroed(48) == 0 && a.need_zeroed(4) == 0 && a[5] == 9, "a kept one is not touched");
    LOG_IS("az");
    CHECK(a.need_zeroed(96) == 0 && a.bytes() == 96 && a[5] == 0 && a[95] == 0, "grown: fresh again");
    LOG_IS("azfaz");
    // the allocation fails: not a zeroing failure
    TestMem::allocs = 0;
    TestMem::fail_at = 1;
    zeroing = true;
    CHECK(a.need_zeroed(200, &zeroing) == kNoMem && !zeroing && !a && a.bytes() == 0, "allocation failed");
    TestMem::fail_at = 0;
    // the zeroing fails: the fresh allocation is given back, the buffer is empty
    TestMem::fail_zero = 1;
    CHECK(a.need_zeroed(200, &zeroing) == kZeroFailed && zeroing && !a && a.bytes() == 0 && TestMem::live == 0, "zeroing failed: live %d", TestMem::live);
    TestMem::fail_zero = 0;
    CHECK(a.need_zeroed(200, &zeroing) == 0 && !zeroing && a[199] == 0, "and again");
}

static void remake_releases_all_first() {
    TestMem::start();
    Arr<float> a;
    Arr<long long> b;
    CHECK(a.need(16) == 0 && b.need(32) == 0, "made");
    TestMem::log.clear();
    CHECK(remake(a, 160, b, 320) == 0 && a.bytes() == 160 && b.bytes() == 320, "%zu %zu", a.bytes(), b.bytes());
    LOG_IS("ffaa");                     // every member released before any is allocated
    CHECK(TestMem::live == 2, "%d", TestMem::live);
    // a buffer that would have sufficed is re-made too: the group is sized together
    TestMem::log.clear();
    CHECK(remake(a, 8, b, 8) == 0 && a.bytes() == 8 && b.bytes() == 8, "%zu %zu", a.bytes(), b.bytes());
    LOG_IS("ffaa");
    // the second member fails: all members empty, nothing leaks
    TestMem::log.clear();
    TestMem::allocs = 0;
    TestMem::fail_at = 2;
    CHECK(remake(a, 64, b, 64) == kNoMem, "the code of the failed member");
    CHECK(!a && !b && a.bytes() == 0 && b.bytes() == 0 && TestMem::live == 0, "live %d", TestMem::live);
    LOG_IS("ffaxf");
    // the first member fails: the second is not tried
    TestMem::log.clear();
    TestMem::allocs = 0;
    TestMem::fail_at = 1;
    CHECK(remake(a, 64, b, 64) == kNoMem && !a && !b && TestMem::live == 0, "live %d", TestMem::live);
    LOG_IS("x");
    TestMem::fail_at = 0;
    CHECK(remake(a, 64, b, 64) == 0 && a && b, "and again");
}

static void borrowed_is_never_freed() {
    TestMem::start();
    float mine[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    {
        Arr<float> a;
        a.borrow(mine, sizeof(mine));
        CHECK(a == mine && a.bytes() == sizeof(mine), "held");
        a.reset();
        CHECK(!a && a.bytes() == 0, "forgotten");
        LOG_IS("");
        a.borrow(mine, sizeof(mine));
        // a later need: never the borrowed memory, however large - a fresh allocation that the array owns
        CHECK(a.need(8) == 0 && a != mine && a.bytes() == 8 && TestMem::live == 1, "live %d", TestMem::live);
        LOG_IS("a");
        a.borrow(mine, sizeof(mine));   // borrowing gives up what was owned
        LOG_IS("af");
        CHECK(TestMem::live == 0, "%d", TestMem::live);
        Arr<float> moved(std::move(a));     // a moved borrow is still a borrow
        CHECK(!a && moved == mine, "moved");
    }                                   // the destructors: nothing to free
    LOG_IS("af");
    CHECK(mine[0] == 1 && mine[7] == 8, "untouched");
}

static void moves_transfer_ownership() {
    TestMem::start();
    {
        Arr<int> a;
        CHECK(a.need(40) == 0, "made");
        int* p = a;
        Arr<int> b(std::move(a));
        CHECK(!a && a.bytes() == 0 && b == p && b.bytes() == 40, "move construction");
        LOG_IS("a");
        Arr<int> c;
        CHECK(c.need(24) == 0, "made");
        c = std::move(b);
        CHECK(!b && b.bytes() == 0 && c == p && c.bytes() == 40, "move assignment");
        LOG_IS("aaf");                  // the target's old memory freed, once
        CHECK(TestMem::live == 1, "%d", TestMem::live);
        Arr<int>& same = c;
        c = std::move(same);            // to itself: kept
        CHECK(c == p && TestMem::live == 1, "%d", TestMem::live);
        CHECK(a.need(8) == 0, "a moved-from array is an empty one");
    }
    LOG_IS("aafaff");
    CHECK(TestMem::live == 0, "%d", TestMem::live);
}

// the index handle in miniature: several arrays in a struct, some never made, one borrowed, one pair re-made
struct Handle {
    Arr<void> rows;
    Arr<float> scores;
    Arr<long long> ids;
    Arr<unsigned> never;
    Arr<void> view;
};

static void struct_of_arrays_frees_everything() {
    TestMem::start();
    char parent[32];
    {
        Handle h;
        CHECK(h.rows.need(1024) == 0 && h.scores.need_zeroed(40) == 0, "made");
        CHECK(remake(h.scores, 400, h.ids, 800) == 0, "re-made");
        h.view.borrow(parent, sizeof(parent));
        CHECK(TestMem::live == 3, "%d", TestMem::live);
        Handle* heap = new Handle();
        CHECK(heap->rows.need(64) == 0 && heap->ids.need(64) == 0, "made");
        heap->rows = std::move(h.rows);
        delete heap;
        CHECK(TestMem::live == 2, "%d", TestMem::live);
    }
    CHECK(TestMem::live == 0, "%d", TestMem::live);
}

int main() {
    need_keeps_and_grows();
    need_fails_empty_and_retries();
    need_zeroed_zeroes_fresh_only();
    remake_releases_all_first();
    borrowed_is_never_freed();
    moves_transfer_ownership();
    struct_of_arrays_frees_everything();
    CHECK(TestMem::live == 0, "%d", TestMem::live);
    if (g_failed) printf("dev_array_check: %d checks FAILED\n", g_failed);
    else printf("dev_array_check: all checks passed\n");
    return g_failed ? 1 : 0;
}
