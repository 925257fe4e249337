// devbuf_host.cpp - bk::DevBuf (biokanga_amd/csrc/bk_devbuf.h, as it stands) on the host: bk::dev_malloc_bytes and bk::free_dev are defined
// here over malloc / free.  They count the live allocations, refuse a free of anything that is not live (a double free, a pointer that
// never came from the allocator), hold the live count under a limit the checks set, and can fail the k-th allocation.
// Built and run by tests/test_host_devbuf.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <type_traits>
#include <utility>

#include "bk_devbuf.h"

static std::set<void *> g_live;
static size_t g_max_live = ~(size_t)0;      // more live allocations than this at once: a failure
static long g_allocs = 0, g_frees = 0;      // calls of the wrappers (free: with a pointer)
static long g_fail_at = -1;                 // the allocation call of this number fails with hipErrorOutOfMemory
static size_t g_last_bytes = 0;
static int g_failed = 0;

#define CHECK(cond, what)                                                         \
    do {                                                                          \
        if (!(cond)) { printf("FAIL [%s] %s (line %d)\n", what, #cond, __LINE__); g_failed++; } \
    } while (0)

namespace bk {
hipError_t dev_malloc_bytes(void **p, size_t bytes)
{
    g_allocs++;
    if (g_allocs == g_fail_at) return hipErrorOutOfMemory;
    CHECK(g_live.size() < g_max_live, "allocator: the old memory goes before the new is asked for");
    void *q = malloc(bytes ? bytes : 1);
    if (!q) return hipErrorOutOfMemory;
    memset(q, 0xA5, bytes);
    g_live.insert(q);
    g_last_bytes = bytes;
    *p = q;
    return hipSuccess;
}

void free_dev(void *p)
{
    if (!p) return;
    g_frees++;
    if (g_live.erase(p) != 1) {
        printf("FAIL [allocator] free of %p, which is not a live allocation\n", p);
        g_failed++;
        return;
    }
    free(p);
}
}  // namespace bk

using bk::DevBuf;

static_assert(!std::is_copy_constructible<DevBuf<uint32_t>>::value && !std::is_copy_assignable<DevBuf<uint32_t>>::value, "DevBuf is not copyable");
static_assert(std::is_nothrow_move_constructible<DevBuf<uint32_t>>::value && std::is_nothrow_move_assignable<DevBuf<uint32_t>>::value, "DevBuf is movable");

// 1: an ensure that fits calls nothing and keeps the pointer
static void check_fitting_ensure()
{
    const char *w = "1 fitting ensure";
    DevBuf<uint32_t> b;
    CHECK(b.get() == nullptr && b.cap() == 0, w);
    CHECK(b.ensure(0) == hipSuccess && g_allocs == 0 && b.get() == nullptr, w);
    CHECK(b.ensure(10) == hipSuccess && b.cap() == 10 && b.get() != nullptr, w);
    uint32_t *p = b.get();
    const long a0 = g_allocs, f0 = g_frees;
    for (size_t n : {10u, 9u, 1u, 0u}) CHECK(b.ensure(n) == hipSuccess && b.get() == p && b.cap() == 10, w);
    CHECK(g_allocs == a0 && g_frees == f0, w);
    p[9] = 1;                                   // (the last element is ours: the sanitizers look)
}

// 2: growing frees first, then allocates exactly n elements
static void check_growing_ensure()
{
    const char *w = "2 growing ensure";
    CHECK(g_live.empty(), w);
    g_max_live = 1;
    {
        DevBuf<uint64_t> b;
        CHECK(b.ensure(10) == hipSuccess && g_last_bytes == 10 * sizeof(uint64_t), w);
        const long a0 = g_allocs, f0 = g_frees;
        CHECK(b.ensure(25) == hipSuccess, w);
        CHECK(b.cap() == 25 && g_last_bytes == 25 * sizeof(uint64_t), w);
        CHECK(g_allocs == a0 + 1 && g_frees == f0 + 1 && g_live.size() == 1, w);
        b.get()[24] = 1;
        CHECK(b.ensure(26) == hipSuccess && b.cap() == 26 && g_last_bytes == 26 * sizeof(uint64_t), w);       // (no growth factor)
        b.reset();
        CHECK(b.get() == nullptr && b.cap() == 0 && g_live.empty(), w);
        b.reset();                              // (of an empty buffer: nothing)
        CHECK(g_frees == f0 + 3, w);
        CHECK(b.ensure(3) == hipSuccess && b.cap() == 3, w);
    }
    CHECK(g_live.empty(), w);
    g_max_live = ~(size_t)0;
}

// 3: a failed ensure leaves the buffer empty, frees nothing twice, and a later ensure works
static void check_failed_ensure()
{
    const char *w = "3 failed ensure";
    DevBuf<uint32_t> b;
    CHECK(b.ensure(10) == hipSuccess, w);
    const long f0 = g_frees;
    g_fail_at = g_allocs + 1;
    CHECK(b.ensure(20) == hipErrorOutOfMemory, w);
    CHECK(b.get() == nullptr && b.cap() == 0, w);
    CHECK(g_live.empty() && g_frees == f0 + 1, w);
    b.reset();
    CHECK(g_frees == f0 + 1, w);
    CHECK(b.ensure(5) == hipSuccess && b.cap() == 5 && b.get() != nullptr && g_live.size() == 1, w);
    g_fail_at = g_allocs + 1;                   // .. and of an empty buffer
    DevBuf<uint32_t> e;
    CHECK(e.ensure(7) == hipErrorOutOfMemory && e.get() == nullptr && e.cap() == 0, w);
    g_fail_at = -1;
}

// 4: moves leave the source empty; the destination frees once; assigning over a buffer frees what it held
static void check_moves()
{
    const char *w = "4 moves";
    CHECK(g_live.empty(), w);
    {
        DevBuf<uint32_t> a;
        CHECK(a.ensure(8) == hipSuccess, w);
        uint32_t *pa = a.get();
        const long a0 = g_allocs, f0 = g_frees;
        DevBuf<uint32_t> b(std::move(a));
        CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == 8, w);
        CHECK(g_allocs == a0 && g_frees == f0 && g_live.size() == 1, w);
        DevBuf<uint32_t> c;
        CHECK(c.ensure(4) == hipSuccess && g_live.size() == 2, w);
        uint32_t *pc = c.get();
        c = std::move(b);
        CHECK(b.get() == nullptr && b.cap() == 0 && c.get() == pa && c.cap() == 8, w);
        CHECK(g_frees == f0 + 1 && g_live.size() == 1 && g_live.count(pc) == 0 && g_live.count(pa) == 1, w);
        c = DevBuf<uint32_t>{};                 // (how a struct of buffers is released: assigned from an empty one)
        CHECK(c.get() == nullptr && c.cap() == 0 && g_live.empty() && g_frees == f0 + 2, w);
        CHECK(a.ensure(2) == hipSuccess && a.cap() == 2, w);      // a moved-from buffer is an empty one
    }
    CHECK(g_live.empty(), w);
    {
        struct Group { DevBuf<uint32_t> x, y[2]; } g;
        CHECK(g.x.ensure(1) == hipSuccess && g.y[0].ensure(2) == hipSuccess && g.y[1].ensure(3) == hipSuccess && g_live.size() == 3, w);
        g = Group{};
        CHECK(g_live.empty() && g.y[1].get() == nullptr, w);
    }
}

int main()
{
    check_fitting_ensure();
    CHECK(g_live.empty(), "the destructor frees");
    check_growing_ensure();
    check_failed_ensure();
    CHECK(g_live.empty(), "the destructor frees");
    check_moves();
    // 5: nothing is left, and every free was of a live allocation (the free wrapper has checked each)
    CHECK(g_live.empty(), "5 live count at exit");
    CHECK(g_frees > 0 && g_allocs > g_frees, "5 the wrappers were used");
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("ok\n");
    return 0;
}
