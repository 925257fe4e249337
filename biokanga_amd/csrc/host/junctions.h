// junctions.h - `align --junctions <file>` / `--splice-strand`: the junction table of the spliced records and their transcript strand
// (XS:A), both from one call of bk_junctions on the first device (include/biokanga_amd.h, where the rule is stated).  The requests are made
// of the lines as written (bk::RecordSet::line, bk_line.h) of the final record set: one per accepted record whose line has an N.
#pragma once
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "post_filters.h"

namespace bkcli {

// the request of accepted record i when its line is [c5 S] m M [c3 S] gap N m2 M; false: the line has no N, or no gap a request can carry
inline bool junction_request(const bk::RecordSet &recs, size_t i, bk_junction_req &q)
{
    const bk::Line L = recs.line(i);
    if (L.gop != 'N') return false;                            // one segment, I or D
    const uint64_t m = L.m, m2 = L.m2;
    const uint64_t start = (uint64_t)L.pos + m;               // POS - 1 + m
    if (L.gap <= 0 || start + (uint64_t)L.gap > 0xFFFFFFFFull) return false;
    q = bk_junction_req{recs.hits[i].chrom_id, (uint32_t)start, (uint32_t)(start + (uint64_t)L.gap), (uint16_t)std::min<uint64_t>(std::min(m, m2), 0xffffu), 0};
    return true;
}

inline bool junction_participant(const bk_hit &h) { return h.nar == BK_NAR_ACCEPTED && (h.strand == '+' || h.strand == '-'); }

// the requests of the record set in record order: reqs[t] and rec_of[t], its record
inline void junction_requests(const bk::RecordSet &recs, std::vector<bk_junction_req> &reqs, std::vector<uint32_t> &rec_of)
{
    reqs.clear(); rec_of.clear();
    for (size_t i = 0; i < recs.size(); i++) {
        bk_junction_req q;
        if (!junction_participant(recs.hits[i]) || !junction_request(recs, i, q)) continue;
        reqs.push_back(q);
        rec_of.push_back((uint32_t)i);
    }
}

// the strand answers of bk_junctions onto the records: recs.xs[i] = '+' / '-' for the record of such a request, 0 for every other record.
// Returns the records that carry a strand.
inline long junction_apply_strands(bk::RecordSet &recs, const std::vector<uint32_t> &rec_of, const std::vector<uint8_t> &strands)
{
    recs.xs.assign(recs.size(), 0);
    long n = 0;
    for (size_t t = 0; t < rec_of.size(); t++)
        if (strands[t] == '+' || strands[t] == '-') { recs.xs[rec_of[t]] = strands[t]; n++; }
    return n;
}

// one line of the table, STAR's SJ.out.tab layout: name, start + 1, end, strand 0 / 1 / 2, motif, 0 (no annotation), reads, 0 (multi-mapping
// reads are not separated), largest overhang
inline void junction_line(const bk_junction &j, const char *name, std::string &out)
{
    char ln[256];
    const int m = snprintf(ln, sizeof(ln), "%s\t%u\t%u\t%d\t%u\t0\t%u\t0\t%u\n", name, j.start + 1, j.end, j.strand == '+' ? 1 : (j.strand == '-' ? 2 : 0), (unsigned)j.motif, j.reads,
                           (unsigned)j.max_overhang);
    out.append(ln, (size_t)m);
}

}  // namespace bkcli
