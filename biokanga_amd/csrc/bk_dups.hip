// bk_dups.hip - duplicate marking (bk_mark_duplicates of include/biokanga_amd.h, where THE RULE is stated: templates with equal keys -
// sequence, unclipped 5' position(s), strand(s) - form a group, the template with the highest score stays, the earlier request among equal
// scores, every other one is a duplicate).  No sort: the grouping table of bk_dev_group.h with bk::DupSlot (owner, best, count), a lane per
// request, two kernels.  k_dup_group: the lane finds or claims its group's slot; on it the lane raises `best` to
// score << 32 | (0xFFFFFFFF - index) by an atomic maximum and counts itself: a group has one slot whatever the scheduling, and the maximum
// makes the keeper independent of it too.  k_dup_verdict, behind the kernel boundary: the lane finds its slot again; it is kept iff the
// low word of `best` names it.  Groups (= owners), the largest count and the flagged requests are reduced over the block before they
// reach the totals.  A lane that runs out of slots raises the error word (bk_dev_group.h says why that is a bug).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_dev_group.h"
#include "bk_env.h"

namespace {
using namespace bk;

constexpr int kDupBlock = 256;                                       // threads per block of every kernel here
constexpr uint32_t kDupWaves = kDupBlock / 64;
enum { kDupGroups = 0, kDupMaxGroup = 1, kDupFlagged = 2, kDupError = 3, kDupTotWords = 4 };

// a template's key with the ends of a pair in canonical order: (a, strand bit 0) <= (b, strand bit 1), '+' < '-'; bit 2: a pair
struct DupKey {
    uint32_t chrom;
    int32_t a, b;
    uint32_t s;
};

// q: a bk_dup_req as one 16-byte load - chrom_id, pos5, pos5_mate, strand | strand_mate << 8 | score << 16
__device__ __forceinline__ DupKey dup_key(const uint4 q)
{
    DupKey k;
    k.chrom = q.x;
    const int32_t p = (int32_t)q.y, pm = (int32_t)q.z;
    const uint32_t sm = (q.w >> 8) & 0xffu;
    const uint32_t s = (q.w & 0xffu) == '-' ? 1u : 0u, m = sm == '-' ? 1u : 0u;
    if (!sm) { k.a = p; k.b = 0; k.s = s; return k; }                 // a fragment: pos5_mate is not looked at
    const bool swap = pm < p || (pm == p && m < s);
    k.a = swap ? pm : p;
    k.b = swap ? p : pm;
    k.s = (swap ? m : s) | ((swap ? s : m) << 1) | 4u;
    return k;
}

__device__ __forceinline__ bool dup_same(const DupKey &x, const DupKey &y) { return x.chrom == y.chrom && x.a == y.a && x.b == y.b && x.s == y.s; }

__device__ __forceinline__ uint64_t dup_hash(const DupKey &k) { return group_hash((uint64_t)k.chrom << 32 | (uint32_t)k.a, (uint64_t)k.s << 32 | (uint32_t)k.b); }

__device__ __forceinline__ bool dup_valid(const DevIndex &ix, const uint4 q)
{
    const uint32_t e = q.x <= ix.max_id ? ix.id2idx[q.x] : 0xffffffffu;
    const uint32_t st = q.w & 0xffu, sm = (q.w >> 8) & 0xffu;
    return e < ix.n_ent && (st == '+' || st == '-') && (sm == 0 || sm == '+' || sm == '-');
}

// pass 1: request j finds or claims its group's slot, offers itself as the keeper and is counted (mask = slots - 1)
__global__ void __launch_bounds__(kDupBlock) k_dup_group(DevIndex ix, const uint4 *__restrict__ reqs, uint64_t n, DupSlot *table, uint64_t mask, unsigned long long *tot)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint4 q = reqs[j];
    if (!dup_valid(ix, q)) return;
    const DupKey k = dup_key(q);
    const uint64_t slot = group_claim(table, mask, dup_hash(k), (uint32_t)j, [&](uint32_t o) { return dup_same(k, dup_key(reqs[o])); });
    if (slot == ~0ULL) { atomicOr(&tot[kDupError], 1ULL); return; }
    atomicMax(&table[slot].best, (unsigned long long)(q.w >> 16) << 32 | (kGroupEmpty - (uint32_t)j));
    atomicAdd(&table[slot].count, 1u);
}

// pass 2: out[j] = 0 kept, 1 duplicate, 2 flagged; tot: groups, largest group, flagged
__global__ void __launch_bounds__(kDupBlock) k_dup_verdict(DevIndex ix, const uint4 *__restrict__ reqs, uint64_t n, const DupSlot *__restrict__ table, uint64_t mask,
                                                           uint8_t *__restrict__ out, unsigned long long *__restrict__ tot)
{
    __shared__ uint32_t s_groups[kDupWaves], s_flagged[kDupWaves], s_max[kDupWaves], s_lost[kDupWaves];
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    bool owner = false, flagged = false, lost = false;
    uint32_t cnt = 0;
    if (j < n) {
        const uint4 q = reqs[j];
        flagged = !dup_valid(ix, q);
        uint8_t answer = 2;
        if (!flagged) {
            const DupKey k = dup_key(q);
            DupSlot t;
            lost = group_find(table, mask, dup_hash(k), (uint32_t)j, [&](uint32_t o) { return dup_same(k, dup_key(reqs[o])); }, t) == ~0ULL;       // (pass 1 left this request in no slot)
            if (!lost) {
                answer = (uint32_t)t.best == kGroupEmpty - (uint32_t)j ? 0 : 1;
                owner = t.owner == (uint32_t)j;
                cnt = owner ? t.count : 0u;
            }
        }
        out[j] = answer;
    }
    const uint32_t ng = (uint32_t)__popcll(__ballot(owner)), nf = (uint32_t)__popcll(__ballot(flagged)), nl = (uint32_t)__popcll(__ballot(lost));
#pragma unroll
    for (int d = 32; d; d >>= 1) cnt = max(cnt, (uint32_t)__shfl_xor((int)cnt, d));
    if (lane == 0) { s_groups[wv] = ng; s_flagged[wv] = nf; s_max[wv] = cnt; s_lost[wv] = nl; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long g = 0, f = 0, x = 0, l = 0;
        for (uint32_t w = 0; w < kDupWaves; w++) { g += s_groups[w]; f += s_flagged[w]; x = max(x, (unsigned long long)s_max[w]); l += s_lost[w]; }
        if (g) { atomicAdd(&tot[kDupGroups], g); atomicMax(&tot[kDupMaxGroup], x); }
        if (f) atomicAdd(&tot[kDupFlagged], f);
        if (l) atomicOr(&tot[kDupError], 2ULL);
    }
}

}  // namespace

extern "C" int bk_mark_duplicates(bk_ctx *c, const bk_dup_req *reqs, uint64_t n, uint8_t *out, bk_dup_totals *totals)
{
    if (!c || (n && (!reqs || !out)) || n >= bk::kGroupEmpty) return BK_ERR_PARAMS;
    if (totals) *totals = bk_dup_totals{};
    if (!n) return BK_OK;
    if (c->entries.empty() || !c->ix.id2idx) return BK_ERR_PARAMS;
    bk::DupStage &B = c->dup;
    bk::GroupCall g;
    if (const int rc = bk::group_begin(c, B.table_slots, reqs, n, B.reqs, B.table, B.tot, kDupTotWords, bk::DupSlot{0ULL, bk::kGroupEmpty, 0u}, [&]() -> int { HIP_TRY(B.out.ensure(n)); return BK_OK; }, g)) return rc;
    const uint64_t slots = g.slots;
    hipStream_t s = c->stream;
    const bool timing = bk::env::timing();
    const uint32_t blocks = (uint32_t)((n + kDupBlock - 1) / kDupBlock);
    const uint4 *d_reqs = reinterpret_cast<const uint4 *>(B.reqs.get());
    hipLaunchKernelGGL(k_dup_group, dim3(blocks), dim3(kDupBlock), 0, s, c->ix, d_reqs, n, B.table.get(), slots - 1, B.tot.get());
    HIP_TRY(hipGetLastError());
    if (timing) HIP_TRY(hipStreamSynchronize(s));
    const double t_group = bk::now_s();
    hipLaunchKernelGGL(k_dup_verdict, dim3(blocks), dim3(kDupBlock), 0, s, c->ix, d_reqs, n, B.table.get(), slots - 1, B.out.get(), B.tot.get());
    HIP_TRY(hipGetLastError());
    if (timing) HIP_TRY(hipStreamSynchronize(s));
    const double t_verdict = bk::now_s();
    unsigned long long tot[kDupTotWords] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(out, B.out.get(), (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(tot, B.tot.get(), sizeof(tot), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (tot[kDupError]) {
        fprintf(stderr, "biokanga_amd: bk_mark_duplicates: a request found no slot among %llu (error word %llu)\n", (unsigned long long)slots, tot[kDupError]);
        return BK_ERR_INTERNAL;
    }
    if (totals) {
        totals->templates = n; totals->groups = tot[kDupGroups]; totals->max_group = tot[kDupMaxGroup]; totals->flagged = tot[kDupFlagged];
        totals->duplicates = n - tot[kDupFlagged] - tot[kDupGroups];
    }
    if (timing)
        fprintf(stderr, "bk timing: mark duplicates: %llu requests, %llu slots (%.1f MB of requests and answers, %.1f MB of table): buffers %.2f, clear + upload %.2f, k_dup_group %.2f, k_dup_verdict %.2f, "
                        "answers back %.2f, whole call %.1f ms\n",
                (unsigned long long)n, (unsigned long long)slots, 1e-6 * (double)(n * 17), 1e-6 * (double)(slots * sizeof(bk::DupSlot)), 1e3 * (g.t_alloc - g.t_start), 1e3 * (g.t_up - g.t_alloc), 1e3 * (t_group - g.t_up),
                1e3 * (t_verdict - t_group), 1e3 * (bk::now_s() - t_verdict), 1e3 * (bk::now_s() - g.t_start));
    return BK_OK;
}
