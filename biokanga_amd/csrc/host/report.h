// report.h - output side of `biokanga align`: SAM / BAM / CSV / BED writers, -O statistics, -j / -J read subsets, .jct / .ind files
// (CAligner::WriteBAMReadHits, ReportBAMread, WriteReadHits, WriteBasicCountStats, ReportNoneAligned / ReportMultiAlign).
#pragma once
#include <functional>
#include "../../../include/biokanga_amd.h"
#include "cli_common.h"
#include "post_filters.h"
#include "site_prefs.h"

namespace bkcli {

// ---------------------------------------------------------------------------------------------
// Everything the reporting functions need about one `align` run (references into its AlignRun; the records and their accessors: rec)
struct Report {
    const Args &a;
    ReadStore &rs;
    const bk::RecordSet &rec;                     // one record per read, or per reported locus in -r5 (post_filters.h)
    const std::vector<bk_entry_info> &ents;
    const std::string &species;
    uint32_t n_ent;
    const std::vector<int> &multi_dist;
    const std::vector<uint32_t> &order;           // records in the reference's output order
    int pe_mode, ml_mode, max_ml, fmt, nthreads, micro_indel, splice_len, max_rpt_sam_seqs;
    bk_ctx *ctx = nullptr;                        // a context whose device formats plain SAM records (bk_sam_format); may be null
    uint32_t sam_tags = 0;                        // --sam-tags: BK_SAMTAG_NM | BK_SAMTAG_MD behind QUAL of accepted SAM / BAM records (made on ctx's device)
    const bk::SitePrefs *site_prefs = nullptr;    // -8: the table the BED / CSV score column is taken from (null: the column is 0)
    SamPrealloc *pre = nullptr;                   // SAM text: the output file, created early and being preallocated; may be null
    bk_sam_prep *sam_prep = nullptr;              // the device formatter's head start (bk_sam_prepare), consumed or freed by report_text / report_bam
    // the reads in the packed form the alignment was fed from, as the head start was given them (bk_sam_job.pk_*); the arrays themselves
    // may be gone once the head start has taken them to the device
    // .. and the read store's bases too, when nothing but the host's own formatter could still want them: restore_reads() brings them
    // back (null: they never left)
    std::function<int()> restore_reads;
    const uint32_t *pk_words = nullptr;
    uint64_t n_pk_words = 0;
    const uint16_t *pk_lens16 = nullptr;
    const bk_nbase *pk_exc = nullptr;
    uint64_t n_pk_exc = 0;

    int score(const bk_hit &h, size_t i) const { return site_prefs ? site_prefs->score(h.strand, i) : 0; }                // Aligner.cpp:6447
};

void report_read_subset(Report &R, const char *opt, const char *tag, bool (*want)(uint8_t));
void report_stats(Report &R);
void report_jct_for_sam(Report &R);
int report_bam(Report &R, const std::string &opath);       // 0, or 1 after a fatal message
int report_text(Report &R);

}  // namespace bkcli
