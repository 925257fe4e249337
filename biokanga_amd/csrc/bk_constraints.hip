// bk_constraints.hip - loci base constraints of `align -5` against finished alignments (gfx950; CAligner::AcceptLociConstraints and
// AcceptBaseConstraint, Aligner.cpp:2480-2595).  A join of the records of a run - tens of millions - against at most 6400 ranges: only
// the records that lie over a range need their bases.  So two kernels per chunk of requests: k_constraint_touch sees geometry alone,
// answers most requests and lists the rest; the host gathers the listed reads' bases and uploads those alone; k_constraint_check walks
// them.  Which records are asked about and what becomes of the answers is host policy above the boundary (host/loci_constraints.h).
#include "bk_device.h"

namespace bk {

// The constraints stay in HBM (100 KB at most, shared by every lane: they live in L2): sorted by (sequence, start, end), a slice per
// constrained sequence, and in every entry the running maximum of `end` inside its slice.  The constraints that can overlap the loci
// s .. e of a sequence are then tab[lo .. hi): hi = the first one whose start lies behind e, lo = the first one whose running maximum
// reaches s - both by bisection, the running maximum never decreases.  lo < hi exactly when one of them overlaps s .. e: tab[hi - 1]'s
// running maximum is the `end` of a constraint that starts no later than tab[hi - 1] does, so at or before e, and ends at or behind s.
__device__ __forceinline__ void overlap_range(const DevConstraint *__restrict__ tab, uint32_t first, uint32_t count, uint32_t s, uint32_t e, uint32_t &lo, uint32_t &hi)
{
    uint32_t a = first, b = first + count;
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (tab[mid].start <= e) a = mid + 1;
        else b = mid;
    }
    hi = a;
    a = first;
    b = hi;
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if (tab[mid].max_end < s) a = mid + 1;
        else b = mid;
    }
    lo = a;
}

struct ConstraintReq {           // a bk_constraint_req out of the two 16-byte loads it is read with
    uint64_t read_ofs;
    uint32_t chrom_id, read_len, strand, n_segs;
    uint32_t start[2], len[2], idx[2];
};
__device__ __forceinline__ ConstraintReq load_req(const bk_constraint_req *__restrict__ reqs, uint64_t i)
{
    const uint4 *w = reinterpret_cast<const uint4 *>(reqs) + 2 * i;
    const uint4 r0 = w[0], r1 = w[1];
    ConstraintReq q;
    q.read_ofs = ((uint64_t)r0.y << 32) | r0.x;
    q.chrom_id = r0.z;
    q.read_len = r0.w & 0xffffu; q.strand = (r0.w >> 16) & 0xffu; q.n_segs = r0.w >> 24;
    q.start[0] = r1.x; q.len[0] = r1.y & 0xffffu; q.idx[0] = r1.y >> 16;
    q.start[1] = r1.z; q.len[1] = r1.w & 0xffffu; q.idx[1] = r1.w >> 16;
    return q;
}

// One lane per request, geometry only.  A request is served when its sequence exists, its strand is '+' or '-', it has one or two
// segments, every segment lies inside the sequence (in 64 bits) and inside the read, and the read inside the `n_bases` bytes the caller
// holds; anything else is answered BK_CONSTRAINT_BAD and reads neither the entry arrays nor the constraints.  Served requests are
// UNTOUCHED unless a segment overlaps a constraint of their sequence: those are TOUCHED, and appended to `list` (room for every
// request) with the range of constraints per segment - the wave's touched lanes take consecutive places behind one atomic of its first
// lane.  Waves take 64 requests a round and every lane stays in the loop until its wave's last round: the ballot needs them all.
__global__ void __launch_bounds__(256) k_constraint_touch(DevIndex ix, DevConstraints cs, const bk_constraint_req *__restrict__ reqs, uint32_t n, uint64_t n_bases,
                                                          uint8_t *__restrict__ status, ConstraintHit *__restrict__ list, uint32_t *__restrict__ list_cnt)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint64_t at = (uint64_t)wave * 64; at < n; at += (uint64_t)n_waves * 64) {
        const uint64_t i = at + lane;
        bool touched = false;
        ConstraintHit hit = {(uint32_t)i, {0, 0}, {0, 0}};
        if (i < n) {
            const ConstraintReq q = load_req(reqs, i);
            uint32_t st = BK_CONSTRAINT_BAD;
            const uint32_t e = q.chrom_id <= ix.max_id ? ix.id2idx[q.chrom_id] : 0xffffffffu;
            if (e < ix.n_ent && (q.strand == '+' || q.strand == '-') && (q.n_segs == 1 || q.n_segs == 2) && q.read_ofs <= n_bases && q.read_len <= n_bases - q.read_ofs) {
                const uint64_t chrom_len = ix.ent_end[e] - ix.ent_start[e] + 1;
                bool ok = true;
                for (uint32_t s = 0; s < q.n_segs; s++) ok = ok && (uint64_t)q.start[s] + q.len[s] <= chrom_len && q.idx[s] + q.len[s] <= q.read_len;
                if (ok) {
                    st = BK_CONSTRAINT_UNTOUCHED;
                    // the sequence's slice: the directory is sorted by chrom_id
                    uint32_t a = 0, b = cs.n_dir;
                    while (a < b) {
                        const uint32_t mid = (a + b) >> 1;
                        if (cs.dir[mid].chrom_id < q.chrom_id) a = mid + 1;
                        else b = mid;
                    }
                    if (a < cs.n_dir && cs.dir[a].chrom_id == q.chrom_id) {
                        const uint32_t first = cs.dir[a].first, count = cs.dir[a].count;
                        for (uint32_t s = 0; s < q.n_segs; s++) {
                            if (!q.len[s]) continue;
                            uint32_t lo, hi;
                            overlap_range(cs.tab, first, count, q.start[s], q.start[s] + q.len[s] - 1, lo, hi);
                            if (lo < hi) { hit.lo[s] = (uint16_t)lo; hit.hi[s] = (uint16_t)hi; touched = true; }
                        }
                        if (touched) st = BK_CONSTRAINT_TOUCHED;
                    }
                }
            }
            status[i] = (uint8_t)st;
        }
        const unsigned long long m = __ballot(touched);
        if (m) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(list_cnt, (uint32_t)__popcll(m));
            base = __shfl(base, 0);
            if (touched) list[base + (uint32_t)__popcll(m & ((1ULL << lane) - 1ULL))] = hit;
        }
    }
}

// One wave per listed request - which k_constraint_touch served, so nothing is checked again.  `gbases` holds the listed reads' bases
// back to back, read t from gofs[t] on.  Lanes take the loci of both segments with stride 64: the base of the read as aligned (for '-'
// the read reversed, codes below 4 complemented: index len - 1 - j of the read as loaded), then every constraint of the segment's
// range that covers the locus - allowed by the base's bit, or with R by equality with the target's nibble `& 7`, fetched once per
// locus and only where an R constraint asks.  One lane's violation is the wave's: its first lane writes BK_CONSTRAINT_VIOLATED.
__global__ void __launch_bounds__(256) k_constraint_check(DevIndex ix, DevConstraints cs, const bk_constraint_req *__restrict__ reqs, const ConstraintHit *__restrict__ list,
                                                          uint32_t n_list, const uint8_t *__restrict__ gbases, const uint64_t *__restrict__ gofs, uint8_t *__restrict__ status)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t t = wave; t < n_list; t += n_waves) {
        const ConstraintHit h = list[t];
        const ConstraintReq q = load_req(reqs, h.req);
        const uint64_t g0 = ix.ent_start[ix.id2idx[q.chrom_id]];
        const uint8_t *__restrict__ b = gbases + gofs[t];
        const bool rev = q.strand == '-';
        bool viol = false;
        for (uint32_t s = 0; s < q.n_segs; s++) {
            const uint32_t lo = h.lo[s], hi = h.hi[s];
            if (lo >= hi) continue;
            for (uint32_t j = lane; j < q.len[s]; j += 64) {
                const uint32_t locus = q.start[s] + j, ridx = q.idx[s] + j;
                uint32_t base = b[rev ? q.read_len - 1 - ridx : ridx] & 7u;
                if (rev && base < 4u) base = 3u - base;
                int tgt = -1;
                for (uint32_t k = lo; k < hi; k++) {
                    const DevConstraint c = cs.tab[k];
                    if (c.start > locus || c.end < locus) continue;
                    bool ok = base < 4u && ((c.mask >> base) & 1u);
                    if (!ok && (c.mask & BK_CONSTRAINT_R)) {
                        if (tgt < 0) { const uint64_t p = g0 + locus; tgt = (int)((ix.tgt4[p >> 4] >> (60 - 4 * (p & 15))) & 7u); }
                        ok = (uint32_t)tgt == base;
                    }
                    viol = viol || !ok;
                }
            }
        }
        if (__any(viol) && lane == 0) status[h.req] = (uint8_t)BK_CONSTRAINT_VIOLATED;
    }
}

void launch_constraint_touch(const DevIndex &ix, const DevConstraints &cs, const bk_constraint_req *reqs, uint32_t n, uint64_t n_bases, uint8_t *status,
                             ConstraintHit *list, uint32_t *list_cnt, hipStream_t s)
{
    if (!n) return;
    uint64_t blocks = ((uint64_t)n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_constraint_touch, dim3((unsigned)blocks), dim3(256), 0, s, ix, cs, reqs, n, n_bases, status, list, list_cnt);
}

void launch_constraint_check(const DevIndex &ix, const DevConstraints &cs, const bk_constraint_req *reqs, const ConstraintHit *list, uint32_t n_list,
                             const uint8_t *gbases, const uint64_t *gofs, uint8_t *status, hipStream_t s)
{
    if (!n_list) return;
    uint64_t blocks = ((uint64_t)n_list + 3) / 4;      // four waves a block
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_constraint_check, dim3((unsigned)blocks), dim3(256), 0, s, ix, cs, reqs, list, n_list, gbases, gofs, status);
}

}  // namespace bk
