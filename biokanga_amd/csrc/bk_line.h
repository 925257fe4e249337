// bk_line.h - the line as written: the CIGAR shape [c5 S] m M [c3 S] [gap N|I|D m2 M] of an accepted record and its POS, from the hit, its
// flank trims (read orientation) and the read's second segment (CAligner::ReportBAMread, Aligner.cpp:5960-6033).  Everybody takes these
// numbers from here: the host's writers and its NM / MD, coverage, duplicate and junction requests (bk::RecordSet::line of
// host/post_filters.h) and the device formatter (sam_rec_ext of bk_sam.hip).  Nothing of HIP here but the qualifiers: the rule is checked
// on the CPU (tests/test_host_line.py).
#pragma once
#include <cstdint>
#include "../../include/biokanga_amd.h"

#if defined(__HIPCC__)
#define BK_LINE_HD __host__ __device__
#else
#define BK_LINE_HD
#endif

namespace bk {
// the op a second segment (flags & 5: FlgInDel or FlgSplice) is written with: a splice junction N; a microInDel I (bit 1) or D
BK_LINE_HD inline char seg2_op(const bk_seg2 &g) { return (g.flags & 4) ? 'N' : ((g.flags & 2) ? 'I' : 'D'); }

struct Line {
    uint32_t pos, m;          // AdjStartLoci (POS - 1), AdjHitLen
    uint32_t c5, c3;          // soft clips in target order: the trims as they are for '+', swapped for '-'
    char gop;                 // 'N', 'I', 'D'; 0: one segment (m2 and gap are 0 then)
    uint32_t m2;
    long gap;                 // target bases the op consumes: N the distance d between the segments as it is (a negative one too), D |d|, I none
    uint32_t seg_bases;       // read bases of both segments, the first untrimmed
    // the number written in front of the op: an I's is what the two segments leave of the read
    BK_LINE_HD long gap_written(uint32_t read_len) const { return gop == 'I' ? (long)read_len - (long)seg_bases : gap; }
};

// tl, tr: the record's trims; g: its read's second segment, or one with no flag of the two set
BK_LINE_HD inline Line line_of(const bk_hit &h, uint32_t tl, uint32_t tr, const bk_seg2 &g)
{
    const bool plus = h.strand == '+';
    Line L{h.match_loci + (plus ? tl : tr), (uint32_t)h.match_len - tl - tr, plus ? tl : tr, plus ? tr : tl, 0, 0u, 0L, h.match_len};
    if (g.flags & 5) {
        const long d = (long)g.match_loci - ((long)h.match_loci + h.match_len);
        L.gop = seg2_op(g);
        L.m2 = g.match_len;
        L.gap = L.gop == 'N' ? d : (L.gop == 'I' ? 0L : (d < 0 ? -d : d));
        L.seg_bases += g.match_len;
    }
    return L;
}
}  // namespace bk
