// bk_search.hip - LocateFirstExact (SfxArrayV2.cpp:7765-7876) + the extent of the matching run for every core of a phase (gfx950):
//   k_search          one pass over suffix array + target (indexes without second-level keys)
//   k_search_a_ilp    pass A: k-mer table + small buckets out of the second-level keys
//   k_search_b        pass B: bisection of the big buckets, work list grouped by bucket
//   k_search_deep     pass B's tails in a launch of their own ("search_split"): suffix array + target behind the key levels, full searches
#include <algorithm>

#include "bk_dev_search_a.h"
#include "bk_dev_prof.h"
#include "bk_plan_table.h"

namespace bk {

// ------------------------------------------------------------------------------------------------
// K1: SA interval search, one lane per (active read, strand, core)

// With `lazy` set (register-window path), a core whose k-mer table bucket holds <= kLazyBucket suffixes
// is NOT bisected/verified here: the bucket is handed on as is (bit 31 of iv_n set) and the extend
// kernels keep only the members whose core bases are clean in the window they evaluate anyway -
// same candidates in the same SA order, two dependent HBM round trips fewer per probe.

template <bool WIDE>
__global__ void __launch_bounds__(256) k_search(DevIndex ix, DevAlignCfg cfg, DevBatch b, const uint32_t *__restrict__ act,
                                                uint32_t n_act, int phase, int cmax, int nstr, int lazy)
{
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t per_read = (uint32_t)(nstr * cmax);
    uint64_t a = tid / per_read;
    if (a >= n_act) return;
    uint32_t rem = (uint32_t)(tid - a * per_read);
    int si = (int)(rem / (uint32_t)cmax), c = (int)(rem % (uint32_t)cmax);
    uint32_t r = act[a];
    const uint32_t meta = b.rmeta[r];
    int len = (int)(meta & kReadLenMask);
    ReadPlan p = make_plan(len, cfg);
    int mm, cl, cd;
    phase_params(p, cfg, phase, mm, cl, cd);
    // offset of core c by the sliding rule
    int cur = cd, o = 0, n = 0, my_ofs = -1;
    while (n < p.max_slides && o <= len - cl && cur > cl / 3) {
        if (o + cl + cur > len) cur = len - (o + cl);
        if (n == c) my_ofs = o;
        n++;
        o += cur;
    }
    if (my_ofs < 0 || n > kMaxCoresFast) return;
    int strand = cfg.align_strand == 2 ? 1 : si;
    const RdRow rdw = read_row(b, r, strand, (meta & kReadHasN) != 0);
    uint64_t first, count;
    uint64_t slot = iv_slot(b, (uint32_t)a, r, strand, c);
    if (lazy && ix.k > 0 && cl >= ix.k) {
        uint64_t p0 = rdw.nib16(my_ofs) & top_mask(cl);
        uint64_t lo, hi;
        core_range(ix, p0, cl, lo, hi);
        if (hi - lo <= kLazyBucket && !(lo == 0 && hi == ix.n)) {
            iv_put(b, slot, lo, (uint32_t)(hi - lo) | (hi > lo ? kLazyFlag : 0u));
            return;
        }
    }
    search_core<WIDE>(ix, rdw, my_ofs, cl, ~0ULL >> 1, first, count);     // exact run length
    iv_put(b, slot, first, count > 0x7FFFFFFFULL ? 0x7FFFFFFFu : (uint32_t)count);
}

// Pass A with ILP searches per lane, written stage by stage so that the loads of a stage (read row, k-mer table, second-level
// keys) of all ILP searches are in flight together: item u of a lane is search number tid + u * (lanes of the grid), i.e. every u
// maps neighbouring lanes to neighbouring searches.  Same records and work list for every ILP (order aside).
// What a read's cores look like in this phase comes from the plan table (bk_plan_table.h): the phase's row is staged in LDS when the
// block starts - at most kMaxReadLenAbs + 1 entries, 16 KB, beside a few words of static LDS, so every batch's row fits and no lane goes
// to memory for it.  An item's (read, strand, core) comes from the block's cursor and reciprocals the launch passes (item_decode): no
// lane divides by a runtime number.

template <int ILP>
__global__ void __launch_bounds__(256) k_search_a_ilp(DevIndex ix, DevAlignCfg cfg, DevBatch b, const uint32_t *__restrict__ act,
                                                      const uint32_t *__restrict__ p_n_act, int phase, int cmax, int nstr, int lazy,
                                                      StripeSet out, ItemGeo ig)
{
    __shared__ uint32_t s_cnt, s_base;
    extern __shared__ uint2 s_plan[];                       // this phase's row of the plan table: b.plan_n entries
    plan_stage(s_plan, b, phase, threadIdx.x, 256);         // (the first tile's barrier stands between these stores and the look-ups)
#if defined(BK_PROF) && BK_PROF == 2
    PROF_BEGIN;
#endif
    // the length of the active list lives in device memory (PhaseCtl); a block takes tiles of 256 * ILP searches until the list is done
    const uint32_t n_act = *p_n_act;
    const uint32_t per_read = (uint32_t)(nstr * cmax);
    const uint64_t total = (uint64_t)n_act * per_read;
    constexpr uint64_t stride = 256;                        // item u of a lane: tile start + lane + 256 u - neighbouring lanes, neighbouring searches
    const int k = ix.k;
    ItemCursor cur = item_cursor((uint64_t)blockIdx.x * (256 * ILP), per_read);       // (block-uniform; ig's step is the grid's stride below)
  for (uint64_t tile0 = (uint64_t)blockIdx.x * (256 * ILP); tile0 < total; tile0 += (uint64_t)gridDim.x * (256 * ILP), item_advance(cur, ig)) {
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    PassACore pa[ILP];                  // the items of this lane, stage by stage (bk_dev_search_a.h)
    uint64_t slot[ILP];
    // The core at offset 0 of phases 0, 1, 2 .. begins with the same k + 15 bases whenever it is that long, so the interval those bases
    // select is looked up once: phase 0 leaves it in iv32 (here, or pass B after its key bisection), the later phases' offset-0 lanes
    // take it from there instead of fetching a k-mer table line and a key line each (a quarter of the searches at C2).
    uint32_t cix[ILP];                  // entry of iv32 this lane reads (phase > 0) or writes (phase 0); kNoIv32 = neither
    // stage 1: the item, its read row
#pragma unroll
    for (int u = 0; u < ILP; u++) {
        pass_a_clear(pa[u]);
        slot[u] = 0;
        cix[u] = kNoIv32;
        uint64_t a;
        int si, c;
        item_decode(cur, threadIdx.x + (uint32_t)u * (uint32_t)stride, ig, a, si, c);
        if (a < n_act) {                                    // (the item's number is below n_act * per_read)
            const uint32_t r = act[a];
            const uint32_t meta = b.rmeta[r];
            const int len = (int)(meta & kReadLenMask);
            const int strand_c = cfg.align_strand == 2 ? 1 : si;
            if (b.iv32 != nullptr && c == 0 && phase > 0) pa[u].cv = b.iv32[(uint32_t)strand_c * b.n_reads + r];     // (requested with the length)
            const PlanGeo g = plan_lookup(s_plan, b.plan_n, len);
            const int cd = g.cd, nc = g.nc;
            pa[u].cl = g.cl;
            if (c < nc && nc <= kMaxCoresFast) {
                pa[u].on = true;
                if (b.iv32 != nullptr && c == 0 && pa[u].cl >= k + kK2Bases) {
                    cix[u] = (uint32_t)strand_c * b.n_reads + r;
                    // (a plain count, or the record of a bucket of one suffix handed on as it is - kElemFlag: the same bucket, the same suffix,
                    // whatever the core's length - where unverified buckets may be handed on at all)
                    pa[u].cached = phase > 0 && pa[u].cv.y != kNoIv32 && (pa[u].cv.y < (1u << kKindShift) || (lazy && (pa[u].cv.y & kIvFlags) == kIvFlags));
                }
                const int my_ofs = c * cd < len - pa[u].cl ? c * cd : len - pa[u].cl;
                const int strand = cfg.align_strand == 2 ? 1 : si;
                slot[u] = iv_slot(b, (uint32_t)a, r, strand, c);
                if (b.rd2 != nullptr && !(meta & kReadHasN)) {
                    // 32 bases from the core's start out of the 2-bit row: the k-mer code's bases and the 16 that follow them
                    const uint64_t *row = b.rd2 + ((uint64_t)r * 2 + strand) * (b.nw / 2);
                    const uint64_t x = bits64_2(row, my_ofs);
                    pa[u].p0 = spread2to4((uint32_t)(x >> 32)) & top_mask(pa[u].cl);
                    pa[u].q2raw = k == 16 ? (uint32_t)x : (uint32_t)(bits64_2(row, my_ofs + k) >> 32);
                } else {
                    const uint64_t *rdw = b.rd4 + ((uint64_t)r * 2 + strand) * b.wpr;
                    pa[u].p0 = nib16(rdw, my_ofs) & top_mask(pa[u].cl);
                    const uint64_t q4 = nib16(rdw, my_ofs + k);
                    pa[u].q2raw = squeeze2(q4);
                    // an N among the core's bases behind the k-mer cannot be put to the 2-bit keys: the full search takes the core
                    const int rem2 = pa[u].cl - k;
                    if (rem2 > 0 && (q4 & 0x4444444444444444ULL & top_mask(rem2 < kK2Bases ? rem2 : kK2Bases))) pa[u].p0 |= 0x4000000000000000ULL;
                }
            }
        }
    }
    PROFS(0);
    // stage 2: k-mer table
#pragma unroll
    for (int u = 0; u < ILP; u++) pass_a_table(ix, k, pa[u]);
    PROFS(1);
    // stage 3: small buckets from the key array
#pragma unroll
    for (int u = 0; u < ILP; u++) pass_a_keys(ix, k, lazy, pa[u]);
    PROFS(2);
    // stage 4: results
#pragma unroll
    for (int u = 0; u < ILP; u++) {
        pass_a_result(k, lazy, pa[u]);
        if (phase == 0 && cix[u] != kNoIv32) b.iv32[cix[u]] = pa[u].leave;
    }
    PROFS(3);
    // work-list appends, one global atomic per block.  The interval records are stored after them: the barriers of the append
    // wait for every store the wave has issued.  Every slot of a core the read has is stored, an empty result as a zero count:
    // nothing clears the records in front of this kernel, and what a slot held (the previous phase's longer list, the previous
    // batch) must not reach a consumer.  A lane that appends its slot to pass B's list stores the work item (bucket and kind) in
    // it, and pass B stores the result over that on every path it has.  Slots of cores a read does not have stay as they were:
    // every consumer looks at the cores below the read's own count only.
    const int lane = threadIdx.x & 63;
    uint32_t my_off[ILP];
#pragma unroll
    for (int u = 0; u < ILP; u++) {
        my_off[u] = 0;
        const uint64_t m = __ballot(pa[u].push);
        if (m) {
            uint32_t w = 0;
            if (lane == 0) w = atomicAdd(&s_cnt, (uint32_t)__popcll(m));
            w = __builtin_amdgcn_readfirstlane(w);
            my_off[u] = w + (uint32_t)__popcll(m & ((1ULL << lane) - 1));
        }
    }
    PROFS(4);
    __syncthreads();
    const uint64_t tile = tile0 / (256 * ILP);
    if (threadIdx.x == 0 && s_cnt) s_base = stripe_reserve_tile(out, 0, s_cnt, tile);
    __syncthreads();
    PROFS(5);
#pragma unroll
    for (int u = 0; u < ILP; u++) {
        if (pa[u].push) stripe_put_tile(out, 0, s_base + my_off[u], (uint32_t)slot[u], tile);
        if (pa[u].on) iv_put(b, slot[u], pa[u].first, pa[u].nval);
    }
    __syncthreads();                                        // (s_cnt / s_base are the next tile's, too)
  }
#if defined(BK_PROF) && BK_PROF == 2
    PROFS(6);
    PROF_END;
#endif
}

// -DBK_DIAG_B builds also count how full pass B's waves are where they load: at every load site the lanes that issue the load add one
// each to `used`, and one of them adds 64 for the wave to `offered` (a line's worth of lanes was there to be used).  Summed per phase in
// g_diag_b (phases 0 .. 7: word 2p used, word 2p + 1 offered), read with bk_debug_prof() by tools/search_b_diag.py.
#ifdef BK_DIAG_B
static __device__ unsigned long long g_diag_b[64 * 16];
#define BK_B_TRIP() do { const unsigned long long m_ = __ballot(1); d_used += 1; if ((int)(threadIdx.x & 63) == __ffsll((long long)m_) - 1) d_off += 64; } while (0)
// (k2_count_range's line counter carries the wave's share above bit 20: bk_dev_k2.h, BK_K2_LINE)
#define BK_B_LINES(l) do { d_used += (l) & 0xFFFFFULL; d_off += 64 * ((l) >> 20); (l) &= 0xFFFFFULL; } while (0)
#define BK_B_FLUSH(phase) do { if ((phase) < 8) { if (d_used) atomicAdd(&g_diag_b[(blockIdx.x & 63) * 16 + 2 * (phase)], d_used); \
                                                   if (d_off) atomicAdd(&g_diag_b[(blockIdx.x & 63) * 16 + 2 * (phase) + 1], d_off); } } while (0)
#else
#define BK_B_TRIP() (void)0
#define BK_B_LINES(l) (void)0
#define BK_B_FLUSH(phase) (void)0
#endif

// Pass B.  SPLIT = false: a lane carries its work item from the second-level keys to the final record.  SPLIT = true ("search_split"): the
// lane runs the key levels only; an item they do not settle - and every kKindFull item - is left in its slot as a continuation (the
// narrowed interval with kind kKindDeep; the kKindFull record as it is) and the slot is appended to the striped list `deep`, which
// k_search_deep finishes in a launch of its own, dense in lanes that all have the same kind of work: the bisection over suffix array and
// target is ten times the dependent trips of an item that ends behind the second-level keys, and one such item keeps its whole wave.
template <bool WIDE, bool SPLIT>
__global__ void __launch_bounds__(256) k_search_b(DevIndex ix, DevAlignCfg cfg, DevBatch b, int phase, int lazy,
                                                  const uint32_t *__restrict__ list, const uint32_t *__restrict__ sorted, uint32_t n_sorted,
                                                  const uint32_t *__restrict__ p_n_list, SlotGeo sg, StripeSet deep)
{
    // the work list's length lives in device memory; its first min(length, n_sorted) items are taken from `sorted` (the grouped copy:
    // the launch had to size the sort before the length was known), the others from the list as pass A left it - the order of the
    // items never changes a result
    __shared__ uint64_t s_lv[kK2Levels + 1];                // where the sampled levels of the keys start (k2s_start)
    extern __shared__ uint2 s_plan[];                       // this phase's row of the plan table, as in pass A: every batch's row fits in LDS
    plan_stage(s_plan, b, phase, threadIdx.x, 256);
    if (threadIdx.x <= (unsigned)kK2Levels) s_lv[threadIdx.x] = threadIdx.x ? k2s_start(ix.n, (int)threadIdx.x) : 0;
    __syncthreads();
    const uint32_t n_list = *p_n_list;
    const uint32_t n_grouped = sorted != nullptr ? (n_list < n_sorted ? n_list : n_sorted) : 0u;
#ifdef BK_DIAG_B
    unsigned long long d_used = 0, d_off = 0;
#endif
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_list; i += gridDim.x * blockDim.x) {
    uint32_t slot32 = 0;
    // the item's key levels; true: the item is not settled and goes on the deep list (SPLIT only)
    const bool push = [&]() -> bool {
#ifdef BK_DIAG_B
    // counted per item kind, low word items, high word 64-byte lines: counter 5 = the bisections over the second- and the third-level
    // keys (items of both added up), counter 6 = what is left for suffix array + target after them
    unsigned long long d_k2 = 0, d_deep = 0, d_sa = 0;
    struct Fin { unsigned long long &a, &b, &c; DevBatch &bb; __device__ ~Fin() { if (a + b) atomicAdd(&bb.ctr[ctr_stripe() + 5], a + b); if (c) atomicAdd(&bb.ctr[ctr_stripe() + 6], c); } } fin{d_k2, d_deep, d_sa, b};
#endif
    BK_B_TRIP();
    slot32 = i < n_grouped ? sorted[i] : list[i];
    const uint64_t slot = slot32;
    uint32_t a;
    int strand, c;
    slot_decode(slot32, sg, a, strand, c);                  // (reciprocals of iv_stride and iv_cores from the launch)
    if (!b.iv_by_read) BK_B_TRIP();
    const uint32_t r = iv_index_read(b.iv_by_read, a, b.act);      // (slots that go by read decode straight to it: no trip to the list)
    BK_B_TRIP();
    const uint32_t meta = b.rmeta[r];
    const int len = (int)(meta & kReadLenMask);
    const PlanGeo g = plan_lookup(s_plan, b.plan_n, len);
    const int cl = g.cl, cd = g.cd;
    const int my_ofs = c * cd < len - cl ? c * cd : len - cl;
    const RdRow rdw = read_row(b, r, strand, (meta & kReadHasN) != 0);
    uint64_t first;
    uint32_t raw;
    iv_get(b, slot, first, raw);
    const uint32_t kind = raw >> kKindShift;
    uint64_t cnt = raw & ((1u << kKindShift) - 1);
    const int k = ix.k;
    if (kind == kKindFull) {
        if (SPLIT) return true;                             // (the record stays as pass A left it)
        BK_B_TRIP();
        search_core<WIDE>(ix, rdw, my_ofs, cl, ~0ULL >> 1, first, cnt);
        iv_put(b, slot, first, cnt > 0x7FFFFFFFULL ? 0x7FFFFFFFu : (uint32_t)cnt);
        return false;
    }
    if (kind == kKindK2) {
        const uint32_t m = k2_mask(cl - k);
        BK_B_TRIP();
        const uint32_t q2 = squeeze2(rdw.nib16(my_ofs + k)) & m;
        // lower and upper bound through the sampled levels: a line per level and bound (bk_dev_k2.h)
        uint64_t l1, l2;
        unsigned long long k2_lines = 0;                    // (counted by -DBK_DIAG_B builds only)
        k2_bounds(ix.k2, s_lv, first, cnt, m, q2, l1, l2, k2_lines);
        BK_B_LINES(k2_lines);
#ifdef BK_DIAG_B
        d_k2 += 1 + (k2_lines << 32);                       // (low word: items of this kind; high word: their lines)
#endif
        // keys of the N kind at the end of the run of equal keys may be there for their fill only: the target decides
        {
            const int upto = cl < k + kK2Bases ? cl : k + kK2Bases;
            while (l2 > l1) {
                BK_B_TRIP();
                const uint32_t kv = ix.k2[l2 - 1];
                if (!k2_nkind(kv) || cmp_core_from(rdw, my_ofs, upto, k, ix.tgt4, sa_get<WIDE>(ix, l2 - 1)) == 0) break;
                l2--;
            }
        }
        first = l1;
        cnt = l2 - l1;
        if (!WIDE && b.iv32 != nullptr && phase == 0 && c == 0 && cl >= k + kK2Bases)       // see k_search_a_ilp
            b.iv32[(uint32_t)strand * b.n_reads + r] = make_uint2((uint32_t)first, (uint32_t)cnt);
        if (cnt == 0 || cl <= k + kK2Bases) {
            iv_put(b, slot, first, cnt > 0x7FFFFFFFULL ? 0x7FFFFFFFu : (uint32_t)cnt);
            return false;
        }
    }
    // [first, first+cnt) agrees with the core on its first k+15 bases
    if (lazy && cnt <= kLazyBucket) {
        iv_put(b, slot, first, (uint32_t)cnt | kLazyFlag);
        return false;
    }
    int start = k + kK2Bases;
    // the next 15 bases from the third-level keys and the 15 after those from the fourth-level keys, the way the second-level keys gave
    // theirs (an N among them in the read: not expressible in 2 bits, the suffix array and the target take over there)
    bool settled = false;
    for (int lv = 0; lv < kMoreKeys && ix.kx[lv] != nullptr; lv++) {
        const uint32_t *__restrict__ kx = ix.kx[lv];
        BK_B_TRIP();
        const uint64_t p3 = rdw.nib16(my_ofs + start);
        if (p3 & 0x4444444444444444ULL & top_mask(cl - start < kK2Bases ? cl - start : kK2Bases)) break;
        const uint32_t m3 = k2_mask(cl - start);
        const uint32_t q3 = squeeze2(p3) & m3;
        uint64_t l1, l2;
        unsigned long long k3_lines = 0;
        k2_bounds(kx, s_lv, first, cnt, m3, q3, l1, l2, k3_lines);
        BK_B_LINES(k3_lines);
#ifdef BK_DIAG_B
        d_deep += 1 + (k3_lines << 32);                     // (low word: items that consult the third-level keys; high word: their lines)
#endif
        {
            const int upto = cl < start + kK2Bases ? cl : start + kK2Bases;
            while (l2 > l1) {
                BK_B_TRIP();
                const uint32_t kv = kx[l2 - 1];
                if (!k2_nkind(kv) || cmp_core_from(rdw, my_ofs, upto, start, ix.tgt4, sa_get<WIDE>(ix, l2 - 1)) == 0) break;
                l2--;
            }
        }
        first = l1;
        cnt = l2 - l1;
        start += kK2Bases;
        if (cnt == 0 || cl <= start) {
            iv_put(b, slot, first, cnt > 0x7FFFFFFFULL ? 0x7FFFFFFFu : (uint32_t)cnt);
            settled = true;
            break;
        }
        if (lazy && cnt <= kLazyBucket) {
            iv_put(b, slot, first, (uint32_t)cnt | kLazyFlag);
            settled = true;
            break;
        }
    }
    if (settled) return false;
    if (SPLIT) {
        // the continuation: what the key levels left of the interval (never wider than the item's own: below 2^kKindShift).  How many
        // bases they covered is not stored - k_search_deep works it out from the read as the loop above did
        iv_put(b, slot, first, (uint32_t)cnt | (kKindDeep << kKindShift));
        return true;
    }
    {
        uint64_t l1 = first, h1 = first + cnt, l2 = first, h2 = first + cnt;
        while (l1 < h1 || l2 < h2) {
            const bool a1 = l1 < h1, a2 = l2 < h2;
            const uint64_t m1 = l1 + ((h1 - l1) >> 1), m2 = l2 + ((h2 - l2) >> 1);
#ifdef BK_DIAG_B
            d_sa += (2ULL << 32) * (a1 + (a2 && m1 != m2));            // (an element of the suffix array and a window of the target per probe)
#endif
            BK_B_TRIP();
            const uint64_t s1 = a1 ? sa_get<WIDE>(ix, m1) : 0, s2 = a2 ? sa_get<WIDE>(ix, m2) : 0;
            BK_B_TRIP();
            const int c1 = a1 ? cmp_core_from(rdw, my_ofs, cl, start, ix.tgt4, s1) : 0;
            const int c2 = a2 ? cmp_core_from(rdw, my_ofs, cl, start, ix.tgt4, s2) : 0;
            if (a1) { if (c1 > 0) l1 = m1 + 1; else h1 = m1; }
            if (a2) { if (c2 >= 0) l2 = m2 + 1; else h2 = m2; }
        }
        first = l1;
#ifdef BK_DIAG_B
        d_sa += 1;
#endif
        cnt = l2 - l1;
    }
    iv_put(b, slot, first, cnt > 0x7FFFFFFFULL ? 0x7FFFFFFFu : (uint32_t)cnt);
    return false;
    }();
    if (SPLIT && push) {
        // the lanes of the wave that hand their item on take places in the tile's stripe together: one atomic a wave, on one of
        // kListStripes lines (tile = the 256 items this block has in hand; a tile appends at most 256 slots: stripe_cap)
        const uint64_t m = __ballot(1);
        const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
        const uint64_t tile = i >> 8;
        uint32_t w = 0;
        if (lane == leader) w = stripe_reserve_tile(deep, 0, (uint32_t)__popcll(m), tile);
        w = __shfl(w, leader);
        stripe_put_tile(deep, 0, w + (uint32_t)__popcll(m & ((1ULL << lane) - 1)), slot32, tile);
    }
  }
    BK_B_FLUSH(phase);
}

// cmp_core_from with the core's first kTailWords 16-base words behind `start` held in registers (masked to the core's length): the tail's
// bisection compares the same bases of the read a dozen times or two, and in a launch where every lane does so the rows of the resident
// waves no longer fit the caches - every step fetched them again
constexpr int kTailWords = 4;
template <typename Row>
__device__ __forceinline__ int cmp_tail(const uint64_t (&pw)[kTailWords], const Row &rdw, int ofs, int cl, int start,
                                        const uint64_t *__restrict__ tgt, uint64_t pos)
{
#pragma unroll
    for (int j = 0; j < kTailWords; j++) {
        const int i = start + 16 * j;
        if (i >= cl) return 0;
        const uint64_t t = nib16(tgt, pos + i) & top_mask(cl - i);
        if (pw[j] != t) return pw[j] < t ? -1 : 1;
    }
    return cmp_core_from(rdw, ofs, cl, start + 16 * kTailWords, tgt, pos);
}

// The tails of pass B's items ("search_split"), a lane per slot of the deep list: the bisection over suffix array and target from the first
// base no key level covered (kKindDeep, the interval k_search_b narrowed), the full search (kKindFull).  It stores the slot's final
// record, as the unsplit pass B does.  How many bases the key levels covered comes from the read alone: k + 15, and 15 more for every key
// array the index has, up to the first whose 15 bases hold an N in the read - the rule of k_search_b's loop, which hands an item on only
// where the core is longer than that.
template <bool WIDE>
__global__ void __launch_bounds__(256) k_search_deep(DevIndex ix, DevBatch b, int phase, const uint32_t *__restrict__ list,
                                                     const uint32_t *__restrict__ p_n_list, SlotGeo sg)
{
    extern __shared__ uint2 s_plan[];
    plan_stage(s_plan, b, phase, threadIdx.x, 256);
    __syncthreads();
    const uint32_t n_list = *p_n_list;
#ifdef BK_DIAG_B
    unsigned long long d_used = 0, d_off = 0;
#endif
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_list; i += gridDim.x * blockDim.x) {
#ifdef BK_DIAG_B
    unsigned long long d_sa = 0;                            // counter 6, as in k_search_b
    struct Fin { unsigned long long &c; DevBatch &bb; __device__ ~Fin() { if (c) atomicAdd(&bb.ctr[ctr_stripe() + 6], c); } } fin{d_sa, b};
#endif
    BK_B_TRIP();
    const uint32_t slot32 = list[i];
    const uint64_t slot = slot32;
    uint32_t a;
    int strand, c;
    slot_decode(slot32, sg, a, strand, c);
    if (!b.iv_by_read) BK_B_TRIP();
    const uint32_t r = iv_index_read(b.iv_by_read, a, b.act);      // (slots that go by read decode straight to it: no trip to the list)
    BK_B_TRIP();
    const uint32_t meta = b.rmeta[r];
    const int len = (int)(meta & kReadLenMask);
    const PlanGeo g = plan_lookup(s_plan, b.plan_n, len);
    const int cl = g.cl, cd = g.cd;
    const int my_ofs = c * cd < len - cl ? c * cd : len - cl;
    const RdRow rdw = read_row(b, r, strand, (meta & kReadHasN) != 0);
    uint64_t first;
    uint32_t raw;
    iv_get(b, slot, first, raw);
    uint64_t cnt = raw & ((1u << kKindShift) - 1);
    if ((raw >> kKindShift) == kKindFull) {
        BK_B_TRIP();
        search_core<WIDE>(ix, rdw, my_ofs, cl, ~0ULL >> 1, first, cnt);
        iv_put(b, slot, first, cnt > 0x7FFFFFFFULL ? 0x7FFFFFFFu : (uint32_t)cnt);
        continue;
    }
    int start = ix.k + kK2Bases;
    for (int lv = 0; lv < kMoreKeys && ix.kx[lv] != nullptr && cl > start; lv++) {
        BK_B_TRIP();
        const uint64_t p3 = rdw.nib16(my_ofs + start);
        if (p3 & 0x4444444444444444ULL & top_mask(cl - start < kK2Bases ? cl - start : kK2Bases)) break;
        start += kK2Bases;
    }
    uint64_t pw[kTailWords];
#pragma unroll
    for (int j = 0; j < kTailWords; j++) {
        const int at = start + 16 * j;
        pw[j] = at < cl ? rdw.nib16(my_ofs + at) & top_mask(cl - at) : 0;
    }
    uint64_t l1 = first, h1 = first + cnt, l2 = first, h2 = first + cnt;
    while (l1 < h1 || l2 < h2) {
        const bool a1 = l1 < h1, a2 = l2 < h2;
        const uint64_t m1 = l1 + ((h1 - l1) >> 1), m2 = l2 + ((h2 - l2) >> 1);
#ifdef BK_DIAG_B
        d_sa += (2ULL << 32) * (a1 + (a2 && m1 != m2));
#endif
        BK_B_TRIP();
        const uint64_t s1 = a1 ? sa_get<WIDE>(ix, m1) : 0, s2 = a2 ? sa_get<WIDE>(ix, m2) : 0;
        BK_B_TRIP();
        const int c1 = a1 ? cmp_tail(pw, rdw, my_ofs, cl, start, ix.tgt4, s1) : 0;
        const int c2 = a2 ? cmp_tail(pw, rdw, my_ofs, cl, start, ix.tgt4, s2) : 0;
        if (a1) { if (c1 > 0) l1 = m1 + 1; else h1 = m1; }
        if (a2) { if (c2 >= 0) l2 = m2 + 1; else h2 = m2; }
    }
#ifdef BK_DIAG_B
    d_sa += 1;
#endif
    cnt = l2 - l1;
    iv_put(b, slot, l1, cnt > 0x7FFFFFFFULL ? 0x7FFFFFFFu : (uint32_t)cnt);
  }
    BK_B_FLUSH(phase);
}

void launch_search(const DevIndex &ix, const DevAlignCfg &cfg, const DevBatch &b, const uint32_t *act, uint32_t n_act,
                   int phase, int cmax, int nstr, int lazy, hipStream_t s)
{
    uint64_t threads = (uint64_t)n_act * (uint64_t)(cmax * nstr);
    unsigned blocks = (unsigned)((threads + 255) / 256);
    if (ix.sa_hi) hipLaunchKernelGGL(k_search<true>, dim3(blocks), dim3(256), 0, s, ix, cfg, b, act, n_act, phase, cmax, nstr, lazy);
    else hipLaunchKernelGGL(k_search<false>, dim3(blocks), dim3(256), 0, s, ix, cfg, b, act, n_act, phase, cmax, nstr, lazy);
}

// keys for grouping work items that touch the same part of the index (see bk_engine.cpp, sort_work):
// search items by the start of their k-mer bucket, wave items by the start of their longest core interval
__global__ void __launch_bounds__(256) k_keys_search(DevBatch b, const uint32_t *__restrict__ list, const uint32_t *__restrict__ p_n, uint32_t n_sort, int shift,
                                                     uint32_t *__restrict__ keys)
{
    // keys of the first min(*p_n, n_sort) items; what the sort was sized for beyond the list's real length sorts to the end
    const uint32_t n = *p_n;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_sort; i += gridDim.x * blockDim.x)
        keys[i] = i < n ? (uint32_t)(iv_start(b, list[i]) >> shift) : 0xFFFFFFFFu;
}

void launch_keys_search(const DevBatch &b, const PhaseLists &l, const PhaseCtl *cur, uint32_t n_sort, int shift, uint32_t *keys, hipStream_t s)
{
    if (!n_sort) return;
    unsigned blocks = (n_sort + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(k_keys_search, dim3(blocks), dim3(256), 0, s, b, l.slist, &cur->n_slist, n_sort, shift, keys);
}

// l.slist_stage: at least n_act * cmax * nstr + (kListStripes + 2) * 1024 entries; l.stripe_cnt: kListStripes * 16 words, zero between launches
// n_act_bound: no more reads than this are on the active list (its length is cur->n_act, in device memory)
void launch_search_a(const DevIndex &ix, const DevAlignCfg &cfg, const DevBatch &b, const PhaseLists &l, PhaseCtl *cur, uint32_t n_act_bound, int phase, int cmax, int nstr, int lazy, hipStream_t s)
{
    uint32_t *list = l.slist, *list_cnt = &cur->n_slist;
    uint64_t threads = (uint64_t)n_act_bound * (uint64_t)(cmax * nstr);
    if (!threads) return;
    lazy &= 0xff;
    constexpr int ilp = 2;                             // searches per lane: 1, 2, 4 measured (45.5 / 42.7 / 43.6 ms of search per C2 step, round 2)
    const uint64_t per = (uint64_t)256 * (uint64_t)ilp;
    const uint64_t tiles = (threads + per - 1) / per;
    const unsigned blocks = (unsigned)std::min<uint64_t>(tiles, 16384);       // (a block takes tiles until the list is done)
    StripeSet out;
    out.cnt = l.stripe_cnt;
    out.stage[0] = out.stage[1] = out.stage[2] = l.slist_stage;
    out.cap = stripe_cap((unsigned)tiles, (unsigned)per);             // (stripes go by tile number)
    static_assert(256 * ilp <= (int)kItemMaxLaneOfs, "a lane's offset within a tile must stay in item_decode's range");
    const ItemGeo ig = item_geo_make((uint32_t)(cmax * nstr), (uint32_t)cmax, (uint64_t)blocks * per);
    const size_t lds = (size_t)b.plan_n * sizeof(uint2);           // the phase's row of the plan table
    hipLaunchKernelGGL(k_search_a_ilp<ilp>, dim3(blocks), dim3(256), lds, s, ix, cfg, b, l.act_in, &cur->n_act, phase, cmax, nstr, lazy, out, ig);
    launch_compact(out, &list, &list_cnt, 1, nullptr, s);
}

// l.slist: the work items as pass A left them (cur->n_slist of them, at most n_bound); sorted / n_sorted: the grouped copy of the first n_sorted (or null)
// split false: a lane carries its item to the end.  Else ("search_split") the items the key levels do not settle are finished by a second
// launch: their slots go through the stripes of l.slist_stage (at least n_bound + (kListStripes + 2) * 1024 entries; l.stripe_cnt as for
// pass A) back into l.slist, which nobody reads once k_search_b has ended, and their number is added to cur->n_deep, zero since the chunk
// began.  k_search_deep is sized by n_bound as well: blocks beyond the count leave at once, none at all does nothing.
void launch_search_b(const DevIndex &ix, const DevAlignCfg &cfg, const DevBatch &b, const PhaseLists &l, PhaseCtl *cur, int phase, int lazy, const uint32_t *sorted, uint32_t n_sorted, uint64_t n_bound, bool split, hipStream_t s)
{
    if (!n_bound) return;
    const uint32_t *list = l.slist, *p_n_list = &cur->n_slist;
    uint32_t *deep_list = l.slist, *deep_cnt = &cur->n_deep;
    const uint64_t tiles = (n_bound + 255) / 256;
    unsigned blocks = (unsigned)std::min<uint64_t>(tiles, 32768);
    const SlotGeo sg = slot_geo_make(b.iv_stride, b.iv_cores);
    const size_t lds = (size_t)b.plan_n * sizeof(uint2);
    StripeSet deep;
    deep.cnt = l.stripe_cnt;
    deep.stage[0] = deep.stage[1] = deep.stage[2] = l.slist_stage;
    deep.cap = stripe_cap((unsigned)tiles, 256);                      // (stripes go by tile number)
    if (!split) {
        if (ix.sa_hi) hipLaunchKernelGGL((k_search_b<true, false>), dim3(blocks), dim3(256), lds, s, ix, cfg, b, phase, lazy, list, sorted, n_sorted, p_n_list, sg, deep);
        else hipLaunchKernelGGL((k_search_b<false, false>), dim3(blocks), dim3(256), lds, s, ix, cfg, b, phase, lazy, list, sorted, n_sorted, p_n_list, sg, deep);
        return;
    }
    if (ix.sa_hi) hipLaunchKernelGGL((k_search_b<true, true>), dim3(blocks), dim3(256), lds, s, ix, cfg, b, phase, lazy, list, sorted, n_sorted, p_n_list, sg, deep);
    else hipLaunchKernelGGL((k_search_b<false, true>), dim3(blocks), dim3(256), lds, s, ix, cfg, b, phase, lazy, list, sorted, n_sorted, p_n_list, sg, deep);
    launch_compact(deep, &deep_list, &deep_cnt, 1, nullptr, s);
    blocks = (unsigned)std::min<uint64_t>(tiles, 8192);
    if (ix.sa_hi) hipLaunchKernelGGL(k_search_deep<true>, dim3(blocks), dim3(256), lds, s, ix, b, phase, deep_list, deep_cnt, sg);
    else hipLaunchKernelGGL(k_search_deep<false>, dim3(blocks), dim3(256), lds, s, ix, b, phase, deep_list, deep_cnt, sg);
}

// the interval records of the slots a phase can use - [strand][core][position in the active list] for every core below cmax - set
// to one word (0: cleared).  Pass A and pass B store every slot they own, so the phase loop does not launch this; "iv_poison" (bk_ctx_tune)
// fills the records with ones in front of the search, which makes any slot a consumer reads without its having been written in
// that phase show in the results.
__global__ void __launch_bounds__(256) k_clear_iv(DevBatch b, const uint32_t *__restrict__ p_n_act, int cmax, int st0, int st1, uint32_t word)
{
    const uint32_t n_act = b.iv_by_read ? b.n_reads : *p_n_act;       // (slots by read: every read's, the list may not exist yet)
    const uint64_t per_strand = (uint64_t)cmax * n_act, total = per_strand * (uint64_t)(st1 - st0 + 1);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const int st = st0 + (int)(i / per_strand);
        const uint64_t q = i % per_strand;
        const uint64_t slot = iv_slot(b, (uint32_t)(q % n_act), (uint32_t)(q % n_act), st, (int)(q / n_act));
        if (b.iv2) b.iv2[slot] = make_uint2(word, word);
        else { b.iv_first[slot] = word ? ~0ULL : 0ULL; b.iv_n[slot] = word; }
    }
}

void launch_clear_iv(const DevBatch &b, const PhaseCtl *cur, uint32_t n_act_bound, int cmax, int st0, int st1, uint32_t word, hipStream_t s)
{
    const uint64_t total = (uint64_t)n_act_bound * (uint64_t)cmax * (uint64_t)(st1 - st0 + 1);
    if (!total) return;
    const unsigned blocks = (unsigned)std::min<uint64_t>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(k_clear_iv, dim3(blocks), dim3(256), 0, s, b, cur ? &cur->n_act : nullptr, cmax, st0, st1, word);      // (cur null: slots by read, nobody reads the count)
}

}  // namespace bk

// in-kernel section timers (bk_dev_prof.h): BK_PROF == 1 reads k_flat's, 2 pass A's; a -DBK_DIAG_B build reads pass B's lane use
namespace bk { int prof_read_flat(unsigned long long *out16); }
extern "C" int bk_debug_prof(unsigned long long *out16)
{
#if defined(BK_PROF) && BK_PROF == 2
    return bk::prof_read(out16);
#elif defined(BK_DIAG_B)
    // lane use of pass B since the library was loaded: phase p's lane-trips used in word 2p, offered in word 2p + 1 (p < 8)
    unsigned long long h[64 * 16];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(bk::g_diag_b), sizeof(h)) != hipSuccess) return 1;
    for (int k = 0; k < 16; k++) { out16[k] = 0; for (int s0 = 0; s0 < 64; s0++) out16[k] += h[s0 * 16 + k]; }
    return 0;
#elif defined(BK_PROF)
    return bk::prof_read_flat(out16);
#else
    (void)out16;
    return 1;
#endif
}
