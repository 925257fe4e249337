// site_prefs.h - start-site octamer preferences of `biokanga align -8 <file> [-9 <ofs>]`: host side of CAligner::ProcessSiteProbabilites,
// WriteSitePrefs and Octamer2Txt (biokanga/Aligner.cpp:8073-8309).  The eight target bases at every alignment's start site come from the
// GPU (bk_site_octamers); here: the sequential pass over them in the reference's sorted order (the carried buffer, PrevLoci, the counts
// per strand, each read's SiteIdx), the scaling to the mean of the top 64 octamers, the CSV writer and the score the BED / CSV
// writers take from the table (:6447).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/biokanga_amd.h"
#include "mtqsort.h"

namespace bk {

constexpr int kNumOctamers = 0x10000;              // cNumOctamers

struct OctSitePref {                               // tsOctSitePrefs
    int octamer, num_sites, num_occs;
    double rel_scale;
};

struct SitePrefs {
    std::vector<OctSitePref> tab[2];               // [0] '+', [1] '-'; by octamer
    // tsReadHit.SiteIdx by record: the reference keeps it in a UINT8 (Aligner.h:201), so the writers look the score up under the
    // octamer's low 8 bits - and under 0 for reads the pass skipped
    std::vector<uint8_t> site_idx;
    long tot_occs = 0, tot_sites = 0;

    // the score column of a record's BED / CSV line (:6447)
    int score(uint8_t strand, size_t rec) const
    {
        const double v = 999 * tab[strand == '+' ? 0 : 1][site_idx[rec]].rel_scale;
        return (int)std::min(1000.0, v);
    }
};

// The loop of :8114-8185 behind the gather.  reqs / res: the visited reads - accepted, no InDel or splice second segment - in
// SortReadHits(eRSMHitMatch) order, and what bk_site_octamers answered for them; rec_of[k]: the record visited read k belongs to.
inline void site_prefs_pass(const bk_site_req *reqs, const bk_site_res *res, const uint32_t *rec_of, size_t n, size_t n_records, SitePrefs &sp)
{
    for (int s = 0; s < 2; s++) {
        sp.tab[s].assign(kNumOctamers, OctSitePref{0, 0, 0, 0.0});
        for (int o = 0; o < kNumOctamers; o++) sp.tab[s][(size_t)o].octamer = o;
    }
    sp.site_idx.assign(n_records, 0);
    sp.tot_occs = sp.tot_sites = 0;
    uint32_t prev_entry = 0, prev_loci = 0xffffffffu;
    uint8_t buf[8];                                // AssembSeq[0..7] as the previous visited read left it
    bool have_buf = false;
    for (size_t k = 0; k < n; k++) {
        const bk_site_req &rq = reqs[k];
        if (rq.chrom_id != prev_entry) { prev_entry = rq.chrom_id; prev_loci = 0xffffffffu; }
        const bool rev = rq.strand == '-';
        if (!(res[k].codes & 0x80000000u)) {
            for (int j = 0; j < 8; j++) buf[j] = (uint8_t)((res[k].codes >> (21 - 3 * j)) & 7u);      // (strand handling done by the device)
            have_buf = true;
        } else {
            // GetSeq returned nothing: the reference goes on with what its buffer held - the previous visited read's eight codes, reverse-
            // complemented once more for a '-' read.  On the very first visited read that buffer is uninitialised stack memory, so
            // the reference's outcome is undefined there: the read is skipped.
            if (!have_buf) continue;
            if (rev) {
                std::reverse(buf, buf + 8);
                for (int j = 0; j < 8; j++) if (buf[j] < 4) buf[j] = (uint8_t)(3 - buf[j]);
            }
        }
        int idx = 0, j = 0;
        for (; j < 8; j++) {
            if (buf[j] > 3) break;
            idx = (idx << 2) | buf[j];
        }
        if (j != 8) continue;                      // (before PrevLoci is looked at)
        sp.site_idx[rec_of[k]] = (uint8_t)idx;
        OctSitePref &p = sp.tab[rev ? 1 : 0][(size_t)idx];
        p.num_occs++;
        sp.tot_occs++;
        if (res[k].site != prev_loci) { p.num_sites++; prev_loci = res[k].site; sp.tot_sites++; }
    }
}

// :8187-8236.  The comparators look at one field and leave ties to the sort, so which of many equal octamers make the top 64 is the
// reference sort's own tie order (mtqsort.h)
inline void site_prefs_scale(SitePrefs &sp)
{
    auto by_scale = [](const OctSitePref &a, const OctSitePref &b) -> int { return a.rel_scale < b.rel_scale ? -1 : (a.rel_scale > b.rel_scale ? 1 : 0); };
    auto by_octamer = [](const OctSitePref &a, const OctSitePref &b) -> int { return a.octamer < b.octamer ? -1 : (a.octamer > b.octamer ? 1 : 0); };
    constexpr int kTop = 0xffc0;
    for (int s = 0; s < 2; s++) {
        std::vector<OctSitePref> &t = sp.tab[s];
        for (OctSitePref &p : t) p.rel_scale = p.num_sites >= 1 ? (double)p.num_occs / p.num_sites : 0.0;
        ref_order_sort(t.data(), (int64_t)kNumOctamers, by_scale);
        double top_mean = 0.0;
        for (int i = kTop; i < kNumOctamers; i++) { top_mean += t[(size_t)i].rel_scale; t[(size_t)i].rel_scale = 1.0; }
        top_mean /= 64;
        for (int i = 0; i < kTop; i++)
            if (t[(size_t)i].rel_scale > 0.0) t[(size_t)i].rel_scale = std::max(0.0001, t[(size_t)i].rel_scale / top_mean);
        ref_order_sort(t.data(), (int64_t)kNumOctamers, by_octamer);
    }
}

// WriteSitePrefs (:8275-8309): 0xffff rows per strand - the reference stops one short of tttttttt
inline void site_prefs_csv(const SitePrefs &sp, std::string &out)
{
    out = "\"Id\",\"Strand\",\"Octamer\",\"TotalHits\",\"UniqueLoci\",\"RelScale\"\n";
    char line[128], oct[9];
    oct[8] = '\0';
    for (int s = 0; s < 2; s++)
        for (int i = 0; i < 0xffff; i++) {
            const OctSitePref &p = sp.tab[s][(size_t)i];
            for (int j = 0, o = p.octamer; j < 8; j++, o >>= 2) oct[7 - j] = "acgt"[o & 3];      // Octamer2Txt
            const int m = snprintf(line, sizeof(line), "%d,\"%c\",\"%s\",%d,%d,%1.3f\n", i + 1, s ? '-' : '+', oct, p.num_occs, p.num_sites, p.rel_scale);
            out.append(line, (size_t)m);
        }
}

}  // namespace bk
