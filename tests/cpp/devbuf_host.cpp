// devbuf_host.cpp - bk::DevBuf and bk::PinBuf (biokanga_amd/csrc/bk_devbuf.h, as it stands) on the host: bk::dev_malloc_bytes / bk::free_dev
// and bk::pin_malloc_bytes / bk::free_pin are defined here over malloc / free, each pair with a pool of its own.  A pool counts its live
// allocations, refuses a free of anything that is not live in it (a double free, a pointer that never came from its allocator - a
// DevBuf's memory handed to the pinned free, or the reverse), holds the live count under a limit the checks set, and can fail the k-th
// allocation.  Every check runs once per owner type.  Built and run by tests/test_host_devbuf.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <type_traits>
#include <utility>

#include "bk_devbuf.h"

static int g_failed = 0;

#define CHECK(cond, what)                                                         \
    do {                                                                          \
        if (!(cond)) { printf("FAIL [%s] %s (line %d)\n", what, #cond, __LINE__); g_failed++; } \
    } while (0)

struct Pool {
    const char *name;
    std::set<void *> live;
    size_t max_live = ~(size_t)0;           // more live allocations than this at once: a failure
    long allocs = 0, frees = 0;             // calls of the wrappers (free: with a pointer)
    long fail_at = -1;                      // the allocation call of this number fails with hipErrorOutOfMemory
    size_t last_bytes = 0;

    hipError_t alloc(void **p, size_t bytes)
    {
        allocs++;
        if (allocs == fail_at) return hipErrorOutOfMemory;
        CHECK(live.size() < max_live, "allocator: the old memory goes before the new is asked for");
        void *q = malloc(bytes ? bytes : 1);
        if (!q) return hipErrorOutOfMemory;
        memset(q, 0xA5, bytes);
        live.insert(q);
        last_bytes = bytes;
        *p = q;
        return hipSuccess;
    }
    void release(void *p)
    {
        if (!p) return;
        frees++;
        if (live.erase(p) != 1) {
            printf("FAIL [%s allocator] free of %p, which is not a live allocation of this pool\n", name, p);
            g_failed++;
            return;
        }
        free(p);
    }
};
static Pool g_dev{"device"}, g_pin{"pinned"};

namespace bk {
hipError_t dev_malloc_bytes(void **p, size_t bytes) { return g_dev.alloc(p, bytes); }
void free_dev(void *p) { g_dev.release(p); }
hipError_t pin_malloc_bytes(void **p, size_t bytes) { return g_pin.alloc(p, bytes); }
void free_pin(void *p) { g_pin.release(p); }
}  // namespace bk

using bk::DevBuf;
using bk::PinBuf;

static_assert(!std::is_copy_constructible<DevBuf<uint32_t>>::value && !std::is_copy_assignable<DevBuf<uint32_t>>::value, "DevBuf is not copyable");
static_assert(std::is_nothrow_move_constructible<DevBuf<uint32_t>>::value && std::is_nothrow_move_assignable<DevBuf<uint32_t>>::value, "DevBuf is movable");
static_assert(!std::is_copy_constructible<PinBuf<uint32_t>>::value && !std::is_copy_assignable<PinBuf<uint32_t>>::value, "PinBuf is not copyable");
static_assert(std::is_nothrow_move_constructible<PinBuf<uint32_t>>::value && std::is_nothrow_move_assignable<PinBuf<uint32_t>>::value, "PinBuf is movable");
static_assert(!std::is_convertible<DevBuf<uint32_t>, PinBuf<uint32_t>>::value && !std::is_convertible<PinBuf<uint32_t>, DevBuf<uint32_t>>::value &&
              !std::is_assignable<DevBuf<uint32_t> &, PinBuf<uint32_t>>::value && !std::is_assignable<PinBuf<uint32_t> &, DevBuf<uint32_t>>::value,
              "memory of one kind is never handed to an owner of the other");

// 1: an ensure that fits calls nothing and keeps the pointer
template <template <class> class Buf> static void check_fitting_ensure(Pool &g, const Pool &o)
{
    const char *w = "1 fitting ensure";
    const long o_calls = o.allocs + o.frees;
    const long a00 = g.allocs;
    Buf<uint32_t> b;
    CHECK(b.get() == nullptr && b.cap() == 0, w);
    CHECK(b.ensure(0) == hipSuccess && g.allocs == a00 && b.get() == nullptr, w);
    CHECK(b.ensure(10) == hipSuccess && b.cap() == 10 && b.get() != nullptr, w);
    uint32_t *p = b.get();
    const long a0 = g.allocs, f0 = g.frees;
    for (size_t n : {10u, 9u, 1u, 0u}) CHECK(b.ensure(n) == hipSuccess && b.get() == p && b.cap() == 10, w);
    CHECK(g.allocs == a0 && g.frees == f0, w);
    p[9] = 1;                                   // (the last element is ours: the sanitizers look)
    CHECK(o.allocs + o.frees == o_calls, w);      // (the other pool saw none of it)
}

// 2: growing frees first, then allocates exactly n elements
template <template <class> class Buf> static void check_growing_ensure(Pool &g, const Pool &o)
{
    const char *w = "2 growing ensure";
    const long o_calls = o.allocs + o.frees;
    CHECK(g.live.empty(), w);
    g.max_live = 1;
    {
        Buf<uint64_t> b;
        CHECK(b.ensure(10) == hipSuccess && g.last_bytes == 10 * sizeof(uint64_t), w);
        const long a0 = g.allocs, f0 = g.frees;
        CHECK(b.ensure(25) == hipSuccess, w);
        CHECK(b.cap() == 25 && g.last_bytes == 25 * sizeof(uint64_t), w);
        CHECK(g.allocs == a0 + 1 && g.frees == f0 + 1 && g.live.size() == 1, w);
        b.get()[24] = 1;
        CHECK(b.ensure(26) == hipSuccess && b.cap() == 26 && g.last_bytes == 26 * sizeof(uint64_t), w);       // (no growth factor)
        b.reset();
        CHECK(b.get() == nullptr && b.cap() == 0 && g.live.empty(), w);
        b.reset();                              // (of an empty buffer: nothing)
        CHECK(g.frees == f0 + 3, w);
        CHECK(b.ensure(3) == hipSuccess && b.cap() == 3, w);
    }
    CHECK(g.live.empty(), w);
    g.max_live = ~(size_t)0;
    CHECK(o.allocs + o.frees == o_calls, w);      // (the other pool saw none of it)
}

// 3: a failed ensure leaves the buffer empty, frees nothing twice, and a later ensure works
template <template <class> class Buf> static void check_failed_ensure(Pool &g, const Pool &o)
{
    const char *w = "3 failed ensure";
    const long o_calls = o.allocs + o.frees;
    Buf<uint32_t> b;
    CHECK(b.ensure(10) == hipSuccess, w);
    const long f0 = g.frees;
    g.fail_at = g.allocs + 1;
    CHECK(b.ensure(20) == hipErrorOutOfMemory, w);
    CHECK(b.get() == nullptr && b.cap() == 0, w);
    CHECK(g.live.empty() && g.frees == f0 + 1, w);
    b.reset();
    CHECK(g.frees == f0 + 1, w);
    CHECK(b.ensure(5) == hipSuccess && b.cap() == 5 && b.get() != nullptr && g.live.size() == 1, w);
    g.fail_at = g.allocs + 1;                   // .. and of an empty buffer
    Buf<uint32_t> e;
    CHECK(e.ensure(7) == hipErrorOutOfMemory && e.get() == nullptr && e.cap() == 0, w);
    g.fail_at = -1;
    CHECK(o.allocs + o.frees == o_calls, w);      // (the other pool saw none of it)
}

// 4: moves leave the source empty; the destination frees once; assigning over a buffer frees what it held
template <template <class> class Buf> static void check_moves(Pool &g, const Pool &o)
{
    const char *w = "4 moves";
    const long o_calls = o.allocs + o.frees;
    CHECK(g.live.empty(), w);
    {
        Buf<uint32_t> a;
        CHECK(a.ensure(8) == hipSuccess, w);
        uint32_t *pa = a.get();
        const long a0 = g.allocs, f0 = g.frees;
        Buf<uint32_t> b(std::move(a));
        CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == 8, w);
        CHECK(g.allocs == a0 && g.frees == f0 && g.live.size() == 1, w);
        Buf<uint32_t> c;
        CHECK(c.ensure(4) == hipSuccess && g.live.size() == 2, w);
        uint32_t *pc = c.get();
        c = std::move(b);
        CHECK(b.get() == nullptr && b.cap() == 0 && c.get() == pa && c.cap() == 8, w);
        CHECK(g.frees == f0 + 1 && g.live.size() == 1 && g.live.count(pc) == 0 && g.live.count(pa) == 1, w);
        c = Buf<uint32_t>{};                 // (how a struct of buffers is released: assigned from an empty one)
        CHECK(c.get() == nullptr && c.cap() == 0 && g.live.empty() && g.frees == f0 + 2, w);
        CHECK(a.ensure(2) == hipSuccess && a.cap() == 2, w);      // a moved-from buffer is an empty one
    }
    CHECK(g.live.empty(), w);
    {
        struct Group { Buf<uint32_t> x, y[2]; } grp;
        CHECK(grp.x.ensure(1) == hipSuccess && grp.y[0].ensure(2) == hipSuccess && grp.y[1].ensure(3) == hipSuccess && g.live.size() == 3, w);
        grp = Group{};
        CHECK(g.live.empty() && grp.y[1].get() == nullptr, w);
    }
    CHECK(o.allocs + o.frees == o_calls, w);      // (the other pool saw none of it)
}

template <template <class> class Buf> static void check_all(Pool &g, const Pool &o)
{
    check_fitting_ensure<Buf>(g, o);
    CHECK(g.live.empty(), "the destructor frees");
    check_growing_ensure<Buf>(g, o);
    check_failed_ensure<Buf>(g, o);
    CHECK(g.live.empty(), "the destructor frees");
    check_moves<Buf>(g, o);
    // 5: nothing is left, and every free was of a live allocation of the owner's own pool (the free wrapper has checked each)
    CHECK(g.live.empty(), "5 live count at exit");
    CHECK(g.frees > 0 && g.allocs > g.frees, "5 the wrappers were used");
}

int main()
{
    check_all<DevBuf>(g_dev, g_pin);
    check_all<PinBuf>(g_pin, g_dev);
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("ok\n");
    return 0;
}
