// primer_correct.h - 5' primer artefact correction of `biokanga align -6 <n>`: host side of CAligner::PCR5PrimerCorrect
// (biokanga/Aligner.cpp:1996-2107).  With -6 the reads are aligned at min(s + n, 15) substitutions per 100 bases; this pass then brings
// every accepted read back under the user's -s by overwriting mismatching bases among its first twelve with the target's, or drops
// it.  The compare against the target runs on the GPU (bk_primer_correct); here: which records are asked about (:2040-2053), the
// request of one, and what its answer does to the record and to the read as loaded (:2072-2093).
#pragma once
#include <cstdint>

#include "../../../include/biokanga_amd.h"

namespace bk {

constexpr int kMaxAllowedSubs = 15;                // cMaxAllowedSubs: the cap of the initial rate (Aligner.cpp:211)
constexpr int kMaxPrimerSubs = 5;                  // cPCRPrimerSubs: -6 0..5 (kanga.cpp:785)

inline int primer_initial_subs(int max_subs, int primer_subs)                // m_InitalAlignSubs (Aligner.cpp:210-213)
{
    return primer_subs > 0 ? (max_subs + primer_subs < kMaxAllowedSubs ? max_subs + primer_subs : kMaxAllowedSubs) : max_subs;
}

inline int primer_max_mms(int rate, uint32_t read_len) { return (int)(((uint32_t)rate * read_len + 50) / 100); }            // :2043

struct PrimerStats {                               // the three counts of the "Completed PCR 5' primer correction" line
    uint64_t reads = 0, bases = 0, rejected = 0;
};

// the reads PCR5PrimerCorrect goes on with: accepted, one segment, not yet inside the rate, matched over their whole length
inline bool primer_selects(const bk_hit &h, bool two_segments, uint32_t read_len, int rate)
{
    if (h.nar != BK_NAR_ACCEPTED || two_segments) return false;
    if ((int)h.low_mm <= primer_max_mms(rate, read_len)) return false;
    return h.match_len == read_len && read_len >= BK_PRIMER_KLEN;
}

// `read`: the read's bases as loaded, a byte each (code in the low three bits)
inline bk_primer_req primer_request(const bk_hit &h, const uint8_t *read, uint32_t read_len, int rate)
{
    bk_primer_req q{};
    for (int k = 0; k < BK_PRIMER_KLEN; k++) q.codes |= (uint64_t)(read[k] & 7u) << (33 - 3 * k);
    q.chrom_id = h.chrom_id;
    q.match_loci = h.match_loci;
    q.match_len = h.match_len;
    q.strand = h.strand;
    q.low_mm = (uint8_t)h.low_mm;
    q.max_mms = (uint8_t)primer_max_mms(rate, read_len);
    return q;
}

// the answer of one request: corrected bases take the target's code and keep their byte's high bits; LowMMCnt and Seg[0].Mismatches
// take the new count - or the read goes (NumHits 0, eNARNoHit).  0, or -1 for an answer the device flagged
inline int primer_apply(const bk_primer_res &r, bk_hit &h, uint8_t *read, PrimerStats &st)
{
    if (r.status == BK_PRIMER_CORRECTED) {
        for (int k = 0; k < BK_PRIMER_KLEN; k++)
            if (r.mask >> k & 1) read[k] = (uint8_t)((read[k] & 0xf8u) | (uint8_t)((r.codes >> (33 - 3 * k)) & 7u));
        h.low_mm = (int8_t)r.mismatches;
        h.mismatches = r.mismatches;
        st.reads++;
        st.bases += r.n_corrected;
    } else if (r.status == BK_PRIMER_REJECTED) {
        h.num_hits = 0;
        h.nar = BK_NAR_NOHIT;
        st.rejected++;
    } else if (r.status != BK_PRIMER_UNTOUCHED)
        return -1;
    return 0;
}

}  // namespace bk
