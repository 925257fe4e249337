// bk_primer.hip - 5' primer artefact correction of finished alignments (gfx950; CAligner::PCR5PrimerCorrect, Aligner.cpp:1996-2107): the
// first twelve bases of a read against the target it aligned to, gathered from the 4-bit target in HBM, and the reference's two loops
// over them.  Which records are asked about, the patching of the read store and the counts are host policy above the boundary
// (host/primer_correct.h).
#include "bk_dev_util.h"

namespace bk {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // a bk_primer_res as the one 16-byte store it is written with

// One lane per request.  The window - the first twelve bases of the match for '+', its last twelve for '-' - lies inside the match, and
// a request is only served when the match lies inside its sequence (match_len >= 12, match_loci + match_len <= the sequence's length,
// in 64 bits), so the two words nib16 loads are inside the padded target.  Anything else - no such sequence included - reads nothing
// and comes back BK_PRIMER_BAD.  The target's nibbles inside a sequence are 0..4: the indexer clears the lower-case flag
// (SfxArrayV2.cpp:1235) and GetSeq answers `& 0x0f` (:2343), so `& 7` of the nibble is what the reference compares the read's `& 7`
// against; a read N (4) never equals a base and is corrected to it, a target N is written into the read as N.  Two dependent loads per
// lane (entry table, target words); requests are read (three 8-byte loads) and results written (one 16-byte store) as whole records by
// consecutive lanes.
__global__ void __launch_bounds__(256) k_primer_correct(DevIndex ix, const bk_primer_req *__restrict__ reqs, uint64_t n, u32x4 *__restrict__ out)      // (out: bk_primer_res records, 16 bytes each)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        // (the 24-byte record as three 8-byte loads, its fields taken from the registers)
        const uint2 *rw = reinterpret_cast<const uint2 *>(reqs) + 3 * i;
        const uint2 r0 = rw[0], r1 = rw[1], r2 = rw[2];
        struct { uint32_t chrom_id, match_loci, match_len, strand, low_mm, max_mms; } rq = {r1.x, r1.y, r2.x & 0xffffu, (r2.x >> 16) & 0xffu, r2.x >> 24, r2.y & 0xffu};
        uint64_t codes = ((uint64_t)(r0.y & 0xfu) << 32) | r0.x;
        uint32_t mask = 0, status = BK_PRIMER_BAD, n_fix = 0;
        int cur = (int)rq.low_mm;
        const int max_mms = (int)rq.max_mms;
        const uint32_t e = rq.chrom_id <= ix.max_id ? ix.id2idx[rq.chrom_id] : 0xffffffffu;
        if (e < ix.n_ent && (rq.strand == '+' || rq.strand == '-') && rq.match_len >= BK_PRIMER_KLEN) {
            const uint64_t g0 = ix.ent_start[e];
            const uint64_t chrom_len = ix.ent_end[e] - g0 + 1;
            if ((uint64_t)rq.match_loci + rq.match_len <= chrom_len) {
                const bool rev = rq.strand == '-';
                const uint64_t at = g0 + rq.match_loci + (rev ? (uint64_t)rq.match_len - BK_PRIMER_KLEN : 0u);
                const uint64_t w = nib16(ix.tgt4, at);                     // twelve nibbles, first base on top
                // window position k: target base k, or for '-' the complement (codes 0..3 only) of target base 11 - k (SeqTrans.cpp:458-512)
                uint64_t tgt = 0;
#pragma unroll
                for (int k = 0; k < BK_PRIMER_KLEN; k++) {
                    uint32_t b = (uint32_t)(w >> (rev ? 16 + 4 * k : 60 - 4 * k)) & 7u;
                    if (rev && b < 4u) b = 3u - b;
                    tgt |= (uint64_t)b << (33 - 3 * k);
                }
                status = BK_PRIMER_UNTOUCHED;
                if (cur > max_mms) {                                       // :2049
                    // would correcting 5' mismatches left to right get the read there?  (:2064-2071)
                    int c1 = cur;
#pragma unroll
                    for (int k = 0; k < BK_PRIMER_KLEN; k++)
                        if (c1 > max_mms && ((codes ^ tgt) >> (33 - 3 * k) & 7u)) c1--;
                    if (c1 <= max_mms) {                                   // :2072-2090: exactly those bases, stopping at the one that gets there
#pragma unroll
                        for (int k = 0; k < BK_PRIMER_KLEN; k++) {
                            const int sh = 33 - 3 * k;
                            const uint32_t fix = (cur > max_mms && ((codes ^ tgt) >> sh & 7u)) ? 1u : 0u;      // (selects, no branch per base)
                            const uint64_t m = fix ? 7ULL << sh : 0ULL;
                            codes = (codes & ~m) | (tgt & m);
                            mask |= fix << k;
                            n_fix += fix;
                            cur -= (int)fix;
                        }
                        status = BK_PRIMER_CORRECTED;
                    } else
                        status = BK_PRIMER_REJECTED;
                }
            }
        }
        // {codes, mask | status << 16 | mismatches << 24, n_corrected}: one 16-byte store per lane
        const uint32_t w2 = mask | (status << 16) | ((uint32_t)(uint8_t)cur << 24);
        out[i] = u32x4{(uint32_t)codes, (uint32_t)(codes >> 32), w2, n_fix};
    }
}

void launch_primer_correct(const DevIndex &ix, const bk_primer_req *reqs, uint64_t n, bk_primer_res *out, hipStream_t s)
{
    if (!n) return;
    uint64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_primer_correct, dim3((unsigned)blocks), dim3(256), 0, s, ix, reqs, n, reinterpret_cast<u32x4 *>(out));
}

}  // namespace bk
