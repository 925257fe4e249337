// bk_dev_group.h - the grouping table of the request passes that collect requests with equal keys (bk_dups.hip, bk_junctions.hip): open
// addressing in HBM, linear probing, a lane per request, no sort.  A slot is any 16-byte struct with a `uint32_t owner`: the index of the
// request that claimed it, whose key is the slot's (requests are not written during a call, so the owner's may be read as soon as its
// index has been seen).  Slots only ever go from empty to owned, and all lanes of a group walk the same probe sequence: the first slot of
// it that is not another group's is claimed by exactly one of them and joined by the rest, so a group has one slot whatever the scheduling.
// Every probe loop ends after `slots` steps: with slots >= n an empty slot or the group is always met before that, so running out is a
// bug - the caller raises its error word and the call returns BK_ERR_INTERNAL instead of hanging.  The device half is checked on the CPU
// beside a stand-in for bk_dev_util.h (tests/test_host_dev_group.py).
#pragma once
#include "bk_dev_util.h"

namespace bk {

constexpr int kGroupBlock = 256;                                     // threads per block of the clear kernel
constexpr uint32_t kGroupEmpty = 0xFFFFFFFFu;                        // `owner` of a slot nobody has claimed (no request has this index: n < 2^32 - 1)

// the hash of a key given as two words; the probe sequence starts at hash & mask
__device__ __forceinline__ uint64_t group_hash(uint64_t a, uint64_t b)
{
    uint64_t h = a * 0x9E3779B97F4A7C15ULL;
    h ^= b + 0xD6E8FEB86659FD93ULL + (h << 6) + (h >> 2);
    h ^= h >> 33; h *= 0xFF51AFD7ED558CCDULL;
    h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ULL;
    h ^= h >> 33;
    return h;
}

// Request j finds or claims its group's slot (mask = slots - 1; same(o): request o's full key equals j's).  Returns the slot, or ~0
// after mask + 1 steps.
template <class Slot, class Same> __device__ __forceinline__ uint64_t group_claim(Slot *table, uint64_t mask, uint64_t hash, uint32_t j, Same same)
{
    uint64_t slot = hash & mask;
    for (uint64_t step = 0; step <= mask; step++, slot = (slot + 1) & mask) {
        uint32_t *ow = &table[slot].owner;
        // (relaxed: a stale "empty" only sends the lane into the compare-and-swap, which answers with the owner there is)
        uint32_t o = __hip_atomic_load(ow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (o == kGroupEmpty) {
            o = atomicCAS(ow, kGroupEmpty, j);
            if (o == kGroupEmpty) o = j;
        }
        if (o == j || same(o)) return slot;                          // (o < n: only requests of this call claim slots)
    }
    return ~0ULL;
}

// a slot as one 16-byte load (read field by field, the fields behind `owner` are fetched only once the probe loop is over: one more trip
// to memory, 6 % of k_dup_verdict)
typedef uint4 __attribute__((may_alias)) group_slot_words;
template <class Slot> __device__ __forceinline__ Slot group_load(const Slot *p)
{
    const uint4 w = *reinterpret_cast<const group_slot_words *>(p);
    Slot s;
    __builtin_memcpy(&s, &w, sizeof(Slot));
    return s;
}

// behind the kernel boundary: the slot of request j's group as the claims left it, with its contents in `found`, or ~0 when there is
// none (which the claims rule out)
template <class Slot, class Same> __device__ __forceinline__ uint64_t group_find(const Slot *table, uint64_t mask, uint64_t hash, uint32_t j, Same same, Slot &found)
{
    uint64_t slot = hash & mask;
    for (uint64_t step = 0; step <= mask; step++, slot = (slot + 1) & mask) {
        found = group_load(table + slot);
        if (found.owner == kGroupEmpty) break;
        if (found.owner == j || same(found.owner)) return slot;
    }
    return ~0ULL;
}

template <class Slot> __global__ void __launch_bounds__(kGroupBlock) k_group_clear(Slot *__restrict__ table, uint64_t slots, Slot empty)
{
    static_assert(sizeof(Slot) == 16 && alignof(Slot) == 16, "a slot is one 16-byte store");
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x) table[i] = empty;
}

}  // namespace bk

#if defined(__HIPCC__)
// ---- the host side: how a call of a grouping pass begins (it launches the clear kernel, so it is here) ----
#include <algorithm>
#include "bk_ctx_int.h"
#include "bk_wait.h"

namespace bk {

struct GroupCall { uint64_t slots = 0; double t_start = 0, t_alloc = 0, t_up = 0; };       // the call's table; BK_TIMING's "buffers" ends at t_alloc, "clear + upload" at t_up

// table_slots: the stage's knob - 0: 1024 doubled up to 2n; else a power of two >= n.  The requests', the table's and the totals' buffers
// are made, the pass's own by more_buffers() (0, or a BK_ERR_ code); the totals are zeroed, the table cleared to `empty`, the requests uploaded, the stream waited for.
template <class Req, class Slot, class More>
int group_begin(bk_ctx *c, uint64_t table_slots, const Req *reqs, uint64_t n, DevBuf<Req> &d_reqs, DevBuf<Slot> &table, DevBuf<unsigned long long> &tot, size_t tot_words,
                Slot empty, More more_buffers, GroupCall &g)
{
    g.slots = table_slots ? table_slots : 1024;
    if (table_slots && ((g.slots & (g.slots - 1)) || g.slots < n)) return BK_ERR_PARAMS;
    while (!table_slots && g.slots < 2 * n) g.slots <<= 1;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    g.t_start = now_s();
    HIP_TRY(d_reqs.ensure(n));
    HIP_TRY(table.ensure(g.slots));
    HIP_TRY(tot.ensure(tot_words));
    if (const int rc = more_buffers()) return rc;
    g.t_alloc = now_s();
    HIP_TRY(hipMemsetAsync(tot.get(), 0, tot_words * 8, s));
    const uint32_t clear_blocks = (uint32_t)std::min<uint64_t>((g.slots + kGroupBlock - 1) / kGroupBlock, 1u << 16);
    hipLaunchKernelGGL(k_group_clear<Slot>, dim3(clear_blocks), dim3(kGroupBlock), 0, s, table.get(), g.slots, empty);
    HIP_TRY(hipGetLastError());
    if (upload_host(d_reqs.get(), reqs, (size_t)n * sizeof(Req), c->device)) return BK_ERR_INTERNAL;
    HIP_TRY(hipStreamSynchronize(s));
    g.t_up = now_s();
    return BK_OK;
}

}  // namespace bk
#endif
