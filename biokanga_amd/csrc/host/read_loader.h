// read_loader.h - the read store's loaders of `biokanga align`: CAligner::LoadRawReads' acceptance rules (biokanga/Aligner.cpp:10724-11427)
// over single-end files and over the mate files of a paired run.  Plain and bgzip'd files are parsed whole (fasta.h) and accepted by
// all threads; the record-by-record loops take everything else, and decide what is said about a file that does not parse.
#pragma once
#include <string>
#include <vector>

#include "cli_common.h"

namespace bkcli {

extern int g_qual_mode;    // -g: FASTQ scores 0 Sanger, 1 Illumina 1.3+, 2 Solexa, 3 ignored (fasta.h)
extern int g_sample_nth;   // -#: every Nth raw read (or pair) of each file is processed, starting with the first (Aligner.cpp:10943,11027-11033)

extern int g_whole_file_loads;   // files that went through the whole-file parse and the all-thread acceptance (the tests' question)

// Contaminant (adaptor) trimming at load, `-H` (Aligner.cpp:11036-11119,11283-11322): behind the -# sampling every raw read is matched against
// the contaminants of its ends, what overlaps counts with the fixed trims in the -l / -L rules and is cut with them (scores too: they share
// the bases' bytes).  The loaders only know this interface; `biokanga align` puts the device matcher (bk_contam_match) behind it.
struct ContamMatcher {
    virtual ~ContamMatcher() = default;
    // `n` reads lying back to back from `bases` on, all PE2 reads or none: out[2i] / out[2i+1] = bases to cut from the 5' / 3' end of read i
    // beyond the fixed trims.  0, or a negative code after the message.
    virtual int match(const uint8_t *bases, const uint32_t *lens, size_t n, bool pe2, int trim5, int trim3, uint16_t *out) = 0;
};
struct ContamTrimming {
    ContamMatcher *matcher = nullptr;       // nullptr: `trims` of an earlier load of the same files are used again, nothing is matched
    bool keep = false;                      // record `trims` (a load that may have to be repeated)
    // per matched read, in the order the files hold them (mates alternate PE1, PE2): 5' and 3' cut
    std::vector<uint16_t> trims;
    size_t replay_at = 0;
};

// 0, or a negative teBSFrsltCodes value after the reference's message
int load_reads(const std::vector<std::string> &files, int trim5, int trim3, int min_len, int max_len, int nthreads, ReadStore &rs,
               ContamTrimming *ct = nullptr);
// mates in lockstep, both must pass the length rules (Aligner.cpp:11080-11130); stored PE1, PE2, PE1, PE2 ..
int load_reads_pe(const std::vector<std::string> &f1, const std::vector<std::string> &f2, int trim5, int trim3, int min_len, int max_len,
                  int nthreads, ReadStore &rs, ContamTrimming *ct = nullptr);

}  // namespace bkcli
