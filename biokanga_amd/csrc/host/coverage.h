// coverage.h - `align --coverage <file>`: the per-base depth of the accepted records as a bedGraph, made on the first device
// (bk_coverage_text of include/biokanga_amd.h, where the rule is stated).  The requests are the M runs of the lines as written
// (bk::RecordSet::line, bk_line.h) of the final record set in output order, whatever the output format.
#pragma once
#include <string>
#include <vector>

#include "report.h"

namespace bkcli {

// the request of accepted record i; false: its numbers are no walk the request can carry
inline bool coverage_request(const bk::RecordSet &recs, size_t i, bk_cov_req &q)
{
    const bk::Line L = recs.line(i);                           // (an I's second M run starts where the first ended: gap 0)
    if (L.m > 0xffffu || L.m2 > 0xffffu || L.gap > 0x7fffffffL || L.gap < -0x7fffffffL) return false;
    q = bk_cov_req{recs.hits[i].chrom_id, L.pos, (uint16_t)L.m, (uint16_t)L.m2, (int32_t)L.gap};
    return true;
}

// 0, or 1 after a fatal message
inline int write_coverage(Report &R, const std::string &path)
{
    const bk::RecordSet &recs = R.rec;
    if (R.ctx == nullptr) { diag("Fatal: '--coverage' needs a device context"); return 1; }
    diag("Processing for per-base coverage into '%s'...", path.c_str());
    std::vector<bk_cov_req> reqs;
    for (const uint32_t i : R.order) {
        const bk_hit &h = recs.hits[i];
        if (h.nar != BK_NAR_ACCEPTED || (h.strand != '+' && h.strand != '-')) continue;
        bk_cov_req q;
        if (!coverage_request(recs, i, q)) { diag("Fatal: the alignment of read '%s' is no walk a coverage request can carry", R.rs.name(recs.RD(i))); return 1; }
        reqs.push_back(q);
    }
    OutBuf out;
    out.open(path.c_str());
    if (out.fd < 0) { diag("Fatal: unable to create '%s'", path.c_str()); return 1; }
    bk_cov_totals tot{};
    const int rc = bk_coverage_text(R.ctx, reqs.data(), reqs.size(), [](void *user, const char *text, uint64_t n, uint64_t) -> int {
        OutBuf &o = *static_cast<OutBuf *>(user);
        o.put(text, (size_t)n);
        return o.failed ? 1 : 0;
    }, &out, &tot);
    out.close();
    if (rc != BK_OK) { diag("Fatal: the coverage could not be made on the device: %s", bk_strerror(rc)); return 1; }
    if (out.failed) { diag("Fatal error: unable to write the coverage to '%s'", path.c_str()); return 1; }
    if (tot.flagged) { diag("Fatal: the coverage pass turned %llu of %zu requests down", (unsigned long long)tot.flagged, reqs.size()); return 1; }
    diag("Coverage: %llu bases covered, mean depth %.2f over covered bases, largest depth %llu, %llu runs", (unsigned long long)tot.covered,
         tot.covered ? (double)tot.depth_sum / (double)tot.covered : 0.0, (unsigned long long)tot.max_depth, (unsigned long long)tot.runs);
    return 0;
}

}  // namespace bkcli
