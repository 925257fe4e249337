// bk_sites.hip - start-site octamers of finished alignments (gfx950; CAligner::ProcessSiteProbabilites, Aligner.cpp:8121-8172): the eight
// target bases at each alignment's start site, gathered from the 4-bit target in HBM.  The sequential half of that routine (the carried
// buffer, PrevLoci, the counts, the scaling) is host policy above the boundary (host/site_prefs.h).
#include "bk_dev_util.h"

namespace bk {

// One lane per alignment.  The arithmetic is the reference's `UINT32 HitLoci`, wraps included: its `HitLoci < 0` test cannot fire, so
// there is no clamp to 0, and a site that wrapped past the sequence's end is what its GetSeq answers with nothing (SfxArrayV2.cpp:2327) -
// bit 31 of the result, and no target word is touched.  A fetched window lies inside its sequence (site + 8 <= chrom_len), so the two
// words nib16 loads are inside the padded target.  Two dependent loads per lane (entry table, target words); requests are read and
// results written as whole records by consecutive lanes.
__global__ void __launch_bounds__(256) k_site_octamers(DevIndex ix, const bk_site_req *__restrict__ reqs, uint64_t n, int32_t rel_ofs,
                                                       bk_site_res *__restrict__ out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const bk_site_req rq = reqs[i];
        const uint32_t e = rq.chrom_id <= ix.max_id ? ix.id2idx[rq.chrom_id] : 0xffffffffu;
        if (e >= ix.n_ent) {                                                 // (no such sequence: the entry points refuse it; a device caller's slip reads nothing)
            reinterpret_cast<uint2 *>(out)[i] = make_uint2(0x80000000u, 0u);
            continue;
        }
        const uint64_t g0 = ix.ent_start[e];
        const uint32_t chrom_len = (uint32_t)(ix.ent_end[e] - g0 + 1);
        const bool rev = rq.strand == '-';
        uint32_t site = rq.match_loci;
        if (!rev) site += (uint32_t)rel_ofs;                                 // :8133-8140
        else site = site + rq.match_len - 1u - (uint32_t)rel_ofs - 7u;
        if ((uint32_t)(site + 8u) >= chrom_len) site = chrom_len - 9u;       // :8145-8146
        uint32_t codes = 0x80000000u;
        if (site < chrom_len && chrom_len - site >= 8u) {                    // (the second test cannot fail behind the clamp: it is the load's own bound)
            const uint32_t w = (uint32_t)(nib16(ix.tgt4, g0 + site) >> 32) & 0x77777777u;      // eight nibbles, first base on top, each & 7
            codes = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                // buffer position k: target base k, or for '-' the complement (codes 0..3 only) of target base 7 - k (SeqTrans.cpp:458-512)
                uint32_t b = (w >> (rev ? 4 * k : 28 - 4 * k)) & 7u;
                if (rev && b < 4u) b = 3u - b;
                codes |= b << (21 - 3 * k);
            }
        }
        reinterpret_cast<uint2 *>(out)[i] = make_uint2(codes, site);        // {codes, site}: one 8-byte store per lane
    }
}

void launch_site_octamers(const DevIndex &ix, const bk_site_req *reqs, uint64_t n, int32_t rel_ofs, bk_site_res *out, hipStream_t s)
{
    if (!n) return;
    uint64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_site_octamers, dim3((unsigned)blocks), dim3(256), 0, s, ix, reqs, n, rel_ofs, out);
}

}  // namespace bk
