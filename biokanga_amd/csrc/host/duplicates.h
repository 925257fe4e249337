// duplicates.h - `align --mark-duplicates`: FLAG 0x400 on the records of duplicate templates, grouped on the first device
// (bk_mark_duplicates of include/biokanga_amd.h, where the rule is stated).  The requests are made of the lines as written
// (bk::RecordSet::line, bk_line.h) of the final record set, one per template, in load order: the library's tie-break (the earlier request
// among equal scores) is then the rule's (the read loaded first).
#pragma once
#include <algorithm>
#include <vector>

#include "post_filters.h"

namespace bkcli {

// one end of a template: the unclipped 5' position of accepted record i and the M bases of its line
struct DupEnd {
    int32_t pos5;
    uint32_t m_bases;
};

inline DupEnd duplicate_end(const bk::RecordSet &recs, size_t i)
{
    const bk::Line L = recs.line(i);
    const long span = (long)L.m + L.gap + (long)L.m2;          // target bases of the line (an I takes none)
    return DupEnd{(int32_t)(recs.hits[i].strand == '+' ? (long)L.pos - (long)L.c5 : (long)L.pos + span - 1 + (long)L.c3), L.m + L.m2};
}

// the request of the template of record i - a fragment - or of records i and mate - a pair, i the end that is handed over first
inline bk_dup_req duplicate_request(const bk::RecordSet &recs, size_t i, long mate = -1)
{
    const DupEnd e = duplicate_end(recs, i);
    bk_dup_req q{};
    q.chrom_id = recs.hits[i].chrom_id; q.pos5 = e.pos5; q.strand = recs.hits[i].strand;
    uint32_t score = e.m_bases;
    if (mate >= 0) {
        const DupEnd f = duplicate_end(recs, (size_t)mate);
        q.pos5_mate = f.pos5; q.strand_mate = recs.hits[(size_t)mate].strand;
        score += f.m_bases;
    }
    q.score = (uint16_t)std::min<uint32_t>(score, 0xffffu);
    return q;
}

inline bool duplicate_participant(const bk_hit &h) { return h.nar == BK_NAR_ACCEPTED && (h.strand == '+' || h.strand == '-'); }

// The templates of the record set in load order: reqs[t] and first[t], the (first) record of template t; a request with a
// strand_mate is the pair first[t], first[t] + 1.  paired: the records are interleaved PE1, PE2 and carry bk_pair_batch's flags.
inline void duplicate_templates(const bk::RecordSet &recs, bool paired, std::vector<bk_dup_req> &reqs, std::vector<uint32_t> &first)
{
    const size_t nr = recs.size();
    reqs.clear(); first.clear();
    reqs.reserve(nr); first.reserve(nr);
    for (size_t i = 0; i < nr; i++) {
        const bk_hit &h = recs.hits[i];
        if (paired && !(i & 1) && i + 1 < nr) {
            const bk_hit &m = recs.hits[i + 1];
            if (duplicate_participant(h) && duplicate_participant(m) && (h.flags & 0x80) && (m.flags & 0x80)) {
                reqs.push_back(duplicate_request(recs, i, (long)i + 1));
                first.push_back((uint32_t)i);
                i++;
                continue;
            }
        }
        if (!duplicate_participant(h)) continue;
        reqs.push_back(duplicate_request(recs, i));
        first.push_back((uint32_t)i);
    }
}

// the answers of bk_mark_duplicates onto the records: recs.dup[i] = 1 for every record of a duplicate template, 0 for all others.
// Returns the records marked, or -1 when an answer is neither "kept" nor "duplicate".
inline long duplicate_apply(bk::RecordSet &recs, const std::vector<bk_dup_req> &reqs, const std::vector<uint32_t> &first, const std::vector<uint8_t> &answers)
{
    recs.dup.assign(recs.size(), 0);
    long n = 0;
    for (size_t t = 0; t < reqs.size(); t++) {
        if (answers[t] > 1) return -1;
        if (!answers[t]) continue;
        recs.dup[first[t]] = 1; n++;
        if (reqs[t].strand_mate) { recs.dup[(size_t)first[t] + 1] = 1; n++; }
    }
    return n;
}

}  // namespace bkcli
