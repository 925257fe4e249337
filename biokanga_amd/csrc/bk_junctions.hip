// bk_junctions.hip - the junction table and the transcript strand of spliced records (bk_junctions of include/biokanga_amd.h, where THE RULE
// is stated: requests with equal (sequence, start, end) are one junction; its motif - and with it its strand - is read from the two target
// bases at each end of the gap, in the sequence as indexed).  The grouping table is that of bk_dev_group.h with bk::JctSlot (owner, count,
// overhang, motif), a lane per request, the request one 16-byte load.  k_jct_group: the lane finds or claims its junction's slot; there
// it counts itself and raises the overhang by an atomic maximum.  k_jct_classify, behind the kernel boundary:
// the lane finds its slot again, and only the owner goes on - the target is gathered once per junction, not once per read: two dinucleotides
// out of DevIndex::tgt4 (one may lie across two of its 64-bit words), the motif into the slot, the bk_junction and its two sort keys into the
// emit arrays at a place taken from one counter per wave.  k_jct_answer: every request reads its slot's strand; junctions, the largest
// count, the motifs and the flagged requests are reduced over the block before they reach the totals.  The emitted junctions are then
// ordered by two stable radix sorts of (key, place) - on `end`, then on entry index << 32 | start - and gathered; the requests are never
// sorted.  A lane that runs out of slots raises the error word (bk_dev_group.h says why that is a bug).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_dev_group.h"
#include "bk_env.h"
#include "bk_prim.h"

namespace {
using namespace bk;

constexpr int kJctBlock = 256;                                       // threads per block of every kernel here
constexpr uint32_t kJctWaves = kJctBlock / 64;
constexpr uint32_t kJctNoEntry = 0xFFFFFFFFu;
enum { kJctJunctions = 0, kJctMaxReads = 1, kJctFlagged = 2, kJctError = 3, kJctEmitted = 4, kJctMotif0 = 5, kJctTotWords = 12 };
static_assert(sizeof(bk_junction_req) == 16 && sizeof(bk_junction) == 20 && sizeof(JctSlot) == 16, "record layout");

// q: a bk_junction_req as one 16-byte load - chrom_id, start, end, overhang | reserved << 16
__device__ __forceinline__ bool jct_same(const uint4 a, const uint4 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

__device__ __forceinline__ uint64_t jct_hash(const uint4 q) { return group_hash((uint64_t)q.x << 32 | q.y, (uint64_t)q.z); }

// the entry index of the request's sequence, or kJctNoEntry for a request that is flagged
__device__ __forceinline__ uint32_t jct_entry(const DevIndex &ix, const uint4 q)
{
    const uint32_t e = q.x <= ix.max_id ? ix.id2idx[q.x] : kJctNoEntry;
    if (e >= ix.n_ent) return kJctNoEntry;
    const uint64_t len = ix.ent_end[e] - ix.ent_start[e] + 1;
    if (q.y == 0 || q.z <= q.y || (uint64_t)q.z >= len || (q.w & 0xffffu) == 0) return kJctNoEntry;
    return e;
}

// the codes (nibble & 7: a c g t n) of the bases at g and g + 1 of the concatenated target, first << 4 | second
__device__ __forceinline__ uint32_t jct_dinuc(const uint64_t *__restrict__ tgt4, uint64_t g)
{
    const uint64_t w = tgt4[g >> 4];
    const uint32_t at = (uint32_t)(g & 15);
    if (at < 15) return (uint32_t)(w >> (56 - 4 * at)) & 0x77u;
    return ((uint32_t)w & 7u) << 4 | ((uint32_t)(tgt4[(g >> 4) + 1] >> 60) & 7u);       // the pair lies across two words
}

// motif 0..6 of the donor and acceptor pairs (codes a0 c1 g2 t3; any n, or anything else: 0)
__device__ __forceinline__ uint32_t jct_motif(uint32_t d, uint32_t a)
{
    const uint32_t k = d << 8 | a;
    switch (k) {
    case 0x2302: return 1;          // GT..AG
    case 0x1301: return 2;          // CT..AC
    case 0x2102: return 3;          // GC..AG
    case 0x1321: return 4;          // CT..GC
    case 0x0301: return 5;          // AT..AC
    case 0x2303: return 6;          // GT..AT
    }
    return 0;
}

// pass 1: request j finds or claims its junction's slot, is counted there and offers its overhang (mask = slots - 1)
__global__ void __launch_bounds__(kJctBlock) k_jct_group(DevIndex ix, const uint4 *__restrict__ reqs, uint64_t n, JctSlot *table, uint64_t mask, unsigned long long *tot)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint4 q = reqs[j];
    if (jct_entry(ix, q) == kJctNoEntry) return;
    const uint64_t slot = group_claim(table, mask, jct_hash(q), (uint32_t)j, [&](uint32_t o) { return jct_same(q, reqs[o]); });
    if (slot == ~0ULL) { atomicOr(&tot[kJctError], 1ULL); return; }
    atomicAdd(&table[slot].count, 1u);
    atomicMax(&table[slot].overhang, q.w & 0xffffu);
}

// the slot of request j's junction as pass 1 left it and what it holds, or ~0 when there is none (which pass 1 rules out)
__device__ __forceinline__ uint64_t jct_find(const uint4 *__restrict__ reqs, const JctSlot *table, uint64_t mask, uint64_t j, const uint4 q, JctSlot &t)
{
    return group_find(table, mask, jct_hash(q), (uint32_t)j, [&](uint32_t o) { return jct_same(q, reqs[o]); }, t);
}

// pass 2: the owner of every slot reads its junction's motif from the target, writes it into the slot and emits the junction: jct[p],
// key_end[p] = end, key_hi[p] = entry index << 32 | start, place[p] = p, with p from the emit counter (one addition per wave)
__global__ void __launch_bounds__(kJctBlock) k_jct_classify(DevIndex ix, const uint4 *__restrict__ reqs, uint64_t n, JctSlot *table, uint64_t mask, uint32_t *__restrict__ jct,
                                                            uint32_t *__restrict__ key_end, unsigned long long *__restrict__ key_hi, uint32_t *__restrict__ place,
                                                            unsigned long long *tot)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    bool owner = false, lost = false;
    uint4 q = make_uint4(0, 0, 0, 0);
    uint32_t e = kJctNoEntry, word = 0, count = 0, overhang = 0;
    if (j < n) {
        q = reqs[j];
        e = jct_entry(ix, q);
        if (e != kJctNoEntry) {
            JctSlot t;
            const uint64_t slot = jct_find(reqs, table, mask, j, q, t);
            lost = slot == ~0ULL;
            if (!lost && t.owner == (uint32_t)j) {
                owner = true;
                const uint64_t g0 = ix.ent_start[e];
                uint32_t motif = 0;
                if (q.z - q.y >= 4) motif = jct_motif(jct_dinuc(ix.tgt4, g0 + q.y), jct_dinuc(ix.tgt4, g0 + q.z - 2));
                const uint32_t strand = motif == 0 ? (uint32_t)'.' : ((motif & 1u) ? (uint32_t)'+' : (uint32_t)'-');
                word = motif | strand << 8;
                table[slot].motif = word;
                count = t.count;
                overhang = t.overhang;
            }
        }
    }
    // (all lanes of the wave are here: none has returned)
    const uint64_t owners = __ballot(owner);
    if (__ballot(lost) && lane == 0) atomicOr(&tot[kJctError], 2ULL);
    if (!owners) return;
    const int leader = __ffsll((unsigned long long)owners) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(&tot[kJctEmitted], (unsigned long long)__popcll(owners));
    base = ((unsigned long long)(uint32_t)__shfl((int)(base >> 32), leader) << 32) | (uint32_t)__shfl((int)(uint32_t)base, leader);
    if (!owner) return;
    const uint64_t p = base + (uint64_t)__popcll(owners & ((1ULL << lane) - 1));          // (p < n: there are no more owners than requests)
    uint32_t *w = jct + 5 * p;
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = count;
    w[4] = (overhang & 0xffffu) | (word & 0xffu) << 16 | (word >> 8 & 0xffu) << 24;        // max_overhang, motif, strand
    key_end[p] = q.z;
    key_hi[p] = (unsigned long long)e << 32 | q.y;
    place[p] = (uint32_t)p;
}

// pass 3: strand_out[j] = '+', '-' or 0; tot: junctions, largest count, junctions by motif, flagged requests
__global__ void __launch_bounds__(kJctBlock) k_jct_answer(DevIndex ix, const uint4 *__restrict__ reqs, uint64_t n, const JctSlot *__restrict__ table, uint64_t mask,
                                                          uint8_t *__restrict__ strand_out, unsigned long long *__restrict__ tot)
{
    __shared__ uint32_t s_flagged[kJctWaves], s_max[kJctWaves], s_lost[kJctWaves], s_motif[kJctWaves][7];
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    bool owner = false, flagged = false, lost = false;
    uint32_t cnt = 0, motif = 0;
    if (j < n) {
        const uint4 q = reqs[j];
        flagged = jct_entry(ix, q) == kJctNoEntry;
        uint8_t answer = 0;
        if (!flagged) {
            JctSlot t;
            lost = jct_find(reqs, table, mask, j, q, t) == ~0ULL;
            if (!lost) {
                motif = t.motif & 0xffu;
                const uint32_t s = t.motif >> 8 & 0xffu;
                answer = s == '.' ? (uint8_t)0 : (uint8_t)s;
                owner = t.owner == (uint32_t)j;
                cnt = owner ? t.count : 0u;
            }
        }
        strand_out[j] = answer;
    }
    const uint32_t nf = (uint32_t)__popcll(__ballot(flagged)), nl = (uint32_t)__popcll(__ballot(lost));
#pragma unroll
    for (int m = 0; m < 7; m++) {
        const uint32_t nm = (uint32_t)__popcll(__ballot(owner && motif == (uint32_t)m));
        if (lane == 0) s_motif[wv][m] = nm;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) cnt = max(cnt, (uint32_t)__shfl_xor((int)cnt, d));
    if (lane == 0) { s_flagged[wv] = nf; s_max[wv] = cnt; s_lost[wv] = nl; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long g = 0, f = 0, x = 0, l = 0;
        for (uint32_t w = 0; w < kJctWaves; w++) { f += s_flagged[w]; x = max(x, (unsigned long long)s_max[w]); l += s_lost[w]; }
        for (int m = 0; m < 7; m++) {
            unsigned long long k = 0;
            for (uint32_t w = 0; w < kJctWaves; w++) k += s_motif[w][m];
            if (k) atomicAdd(&tot[kJctMotif0 + m], k);
            g += k;
        }
        if (g) { atomicAdd(&tot[kJctJunctions], g); atomicMax(&tot[kJctMaxReads], x); }
        if (f) atomicAdd(&tot[kJctFlagged], f);
        if (l) atomicOr(&tot[kJctError], 4ULL);
    }
}

// between the two sorts: the second key of every junction in the order the first sort left
__global__ void __launch_bounds__(kJctBlock) k_jct_second_keys(const unsigned long long *__restrict__ key_hi, const uint32_t *__restrict__ place, uint64_t n,
                                                               unsigned long long *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = key_hi[place[i]];
}

// behind them: the junctions in their final order (five words each)
__global__ void __launch_bounds__(kJctBlock) k_jct_gather(const uint32_t *__restrict__ jct, const uint32_t *__restrict__ place, uint64_t n, uint32_t *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *s = jct + 5 * (uint64_t)place[i];
    uint32_t *w = out + 5 * i;
    w[0] = s[0]; w[1] = s[1]; w[2] = s[2]; w[3] = s[3]; w[4] = s[4];
}

}  // namespace

extern "C" int bk_junctions(bk_ctx *c, const bk_junction_req *reqs, uint64_t n, uint8_t *strand_out, bk_junction *out, uint64_t cap, uint64_t *n_junctions,
                            bk_junction_totals *totals)
{
    if (!c || (n && !reqs) || n >= bk::kGroupEmpty || (!out && cap)) return BK_ERR_PARAMS;
    if (!n) {
        if (n_junctions) *n_junctions = 0;
        if (totals) *totals = bk_junction_totals{};
        return BK_OK;
    }
    if (c->entries.empty() || !c->ix.id2idx || !c->ix.tgt4) return BK_ERR_PARAMS;
    bk::JunctionStage &B = c->jct;
    auto more_buffers = [&]() -> int {
        HIP_TRY(B.strand.ensure(n)); HIP_TRY(B.jct.ensure(n)); HIP_TRY(B.key_end[0].ensure(n)); HIP_TRY(B.key_hi[0].ensure(n)); HIP_TRY(B.place[0].ensure(n));
        return BK_OK;
    };
    bk::GroupCall g;
    if (const int rc = bk::group_begin(c, B.table_slots, reqs, n, B.reqs, B.table, B.tot, kJctTotWords, bk::JctSlot{bk::kGroupEmpty, 0u, 0u, 0u}, more_buffers, g)) return rc;
    const uint64_t slots = g.slots;
    hipStream_t s = c->stream;
    const bool timing = bk::env::timing();
    const uint32_t blocks = (uint32_t)((n + kJctBlock - 1) / kJctBlock);
    const uint4 *d_reqs = reinterpret_cast<const uint4 *>(B.reqs.get());
    uint32_t *d_jct = reinterpret_cast<uint32_t *>(B.jct.get());
    hipLaunchKernelGGL(k_jct_group, dim3(blocks), dim3(kJctBlock), 0, s, c->ix, d_reqs, n, B.table.get(), slots - 1, B.tot.get());
    HIP_TRY(hipGetLastError());
    if (timing) HIP_TRY(hipStreamSynchronize(s));
    const double t_group = bk::now_s();
    hipLaunchKernelGGL(k_jct_classify, dim3(blocks), dim3(kJctBlock), 0, s, c->ix, d_reqs, n, B.table.get(), slots - 1, d_jct, B.key_end[0].get(), B.key_hi[0].get(),
                       B.place[0].get(), B.tot.get());
    HIP_TRY(hipGetLastError());
    if (timing) HIP_TRY(hipStreamSynchronize(s));
    const double t_classify = bk::now_s();
    hipLaunchKernelGGL(k_jct_answer, dim3(blocks), dim3(kJctBlock), 0, s, c->ix, d_reqs, n, B.table.get(), slots - 1, B.strand.get(), B.tot.get());
    HIP_TRY(hipGetLastError());
    unsigned long long tot[kJctTotWords] = {0};
    HIP_TRY(hipMemcpyAsync(tot, B.tot.get(), sizeof(tot), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const double t_answer = bk::now_s();
    if (tot[kJctError] || tot[kJctEmitted] != tot[kJctJunctions] || tot[kJctJunctions] > n) {
        fprintf(stderr, "biokanga_amd: bk_junctions: a request found no slot among %llu (error word %llu; %llu junctions emitted, %llu counted)\n", (unsigned long long)slots,
                tot[kJctError], tot[kJctEmitted], tot[kJctJunctions]);
        return BK_ERR_INTERNAL;
    }
    const uint64_t nj = tot[kJctJunctions];
    if (n_junctions) *n_junctions = nj;
    if (out && nj > cap) return BK_ERR_MEM;
    if (out && nj) {
        // two stable passes, the less significant key first: `end`, then entry index << 32 | start; the places travel as the values
        int hi_bits = 33;
        while (hi_bits < 64 && ((uint64_t)c->ix.n_ent >> (hi_bits - 32))) hi_bits++;
        HIP_TRY(B.key_end[1].ensure(nj));
        HIP_TRY(B.key_hi[1].ensure(nj));
        HIP_TRY(B.key_hi[2].ensure(nj));
        HIP_TRY(B.place[1].ensure(nj));
        HIP_TRY(B.place[2].ensure(nj));
        HIP_TRY(B.sorted.ensure(nj));
        size_t tb1 = 0, tb2 = 0;
        HIP_TRY(bk::prim::sort_pairs(nullptr, tb1, B.key_end[0].get(), B.key_end[1].get(), B.place[0].get(), B.place[1].get(), (size_t)nj, 0, 32, s));
        HIP_TRY(bk::prim::sort_pairs(nullptr, tb2, B.key_hi[1].get(), B.key_hi[2].get(), B.place[1].get(), B.place[2].get(), (size_t)nj, 0, hi_bits, s));
        HIP_TRY(B.tmp.ensure(std::max(tb1, tb2) + 256));
        const uint32_t jblocks = (uint32_t)((nj + kJctBlock - 1) / kJctBlock);
        size_t tb = B.tmp.cap();
        HIP_TRY(bk::prim::sort_pairs(B.tmp.get(), tb, B.key_end[0].get(), B.key_end[1].get(), B.place[0].get(), B.place[1].get(), (size_t)nj, 0, 32, s));
        hipLaunchKernelGGL(k_jct_second_keys, dim3(jblocks), dim3(kJctBlock), 0, s, B.key_hi[0].get(), B.place[1].get(), nj, B.key_hi[1].get());
        HIP_TRY(hipGetLastError());
        tb = B.tmp.cap();
        HIP_TRY(bk::prim::sort_pairs(B.tmp.get(), tb, B.key_hi[1].get(), B.key_hi[2].get(), B.place[1].get(), B.place[2].get(), (size_t)nj, 0, hi_bits, s));
        hipLaunchKernelGGL(k_jct_gather, dim3(jblocks), dim3(kJctBlock), 0, s, d_jct, B.place[2].get(), nj, reinterpret_cast<uint32_t *>(B.sorted.get()));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, B.sorted.get(), (size_t)nj * sizeof(bk_junction), hipMemcpyDeviceToHost, s));
    }
    if (strand_out) HIP_TRY(hipMemcpyAsync(strand_out, B.strand.get(), (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (totals) {
        totals->requests = n; totals->junctions = nj; totals->flagged = tot[kJctFlagged]; totals->max_reads = tot[kJctMaxReads];
        for (int m = 0; m < 7; m++) totals->by_motif[m] = tot[kJctMotif0 + m];
    }
    if (timing)
        fprintf(stderr, "bk timing: junctions: %llu requests, %llu slots, %llu junctions (%.1f MB of requests, answers and emitted junctions, %.1f MB of table): buffers %.2f, "
                        "clear + upload %.2f, k_jct_group %.2f, k_jct_classify %.2f, k_jct_answer + totals back %.2f, sort + answers back %.2f, whole call %.1f ms\n",
                (unsigned long long)n, (unsigned long long)slots, (unsigned long long)nj, 1e-6 * (double)(n * (16 + 1 + 20 + 4 + 8 + 4)), 1e-6 * (double)(slots * sizeof(bk::JctSlot)),
                1e3 * (g.t_alloc - g.t_start), 1e3 * (g.t_up - g.t_alloc), 1e3 * (t_group - g.t_up), 1e3 * (t_classify - t_group), 1e3 * (t_answer - t_classify),
                1e3 * (bk::now_s() - t_answer), 1e3 * (bk::now_s() - g.t_start));
    return BK_OK;
}
