// biokanga_main.cpp - host front end: `biokanga index` and `biokanga align` (C++ above the C ABI).
//
// Keeps the reference's option letters and defaults for the subset that reaches the hot path
// (biokanga/kanga.cpp:194-294, biokanga/kangax.cpp:95-116), the .sfx index format and the SAM text
// the reference writes (libbiokanga/SAMfile.cpp:1521,1573-1575,1766,2110-2283).  The alignment
// itself is ONLY available through libbiokanga_amd (HIP kernels); there is no host fallback.
//
//   biokanga index -i genome.fa[.gz] [-i more.fa] -o genome.sfx -r name [-l minseqlen] [-d descr] [-t title] [-T threads] [--device n]
//   biokanga align -i reads.fa[.gz] -I genome.sfx -o out.sam [-s subs] [-e 1|2] [-Q 0|1|2] [-m 0..3]
//                  [-n maxNs] [-l minlen] [-L maxlen] [-y trim5] [-Y trim3] [-H contaminants.fa] [-M 0|5|6] [-O stats.csv]
//                  [-U 1..4 -u mates.fa -d minins -D maxins [-E]] [-8 siteprefs.csv [-9 ofs]] [-6 0..5] [-5 lociconstraints.csv] [-T host threads] [-F logfile] [--device n | --devices 0-7]
//                  [--sam-tags NM,MD] [--coverage depth.bedgraph] [--mark-duplicates] [--junctions sj.tab] [--splice-strand]
//   (reads: FASTA / FASTQ, plain, gzip'd or bgzip'd, also through a FIFO; -o: a file, a name ending in .gz or .bam, or a FIFO)
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <unistd.h>
#include <regex.h>
#include <zlib.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cctype>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <memory>
#include <ctime>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/biokanga_amd.h"
#include "../sfx_file.h"
#include "../bk_env.h"
#include "bam_writer.h"
#include "fasta.h"
#include "genome_loader.h"
#include "glibc_rand.h"
#include "mtqsort.h"
#include "multi_assign.h"
#include "post_filters.h"
#include "snp.h"
#include "site_prefs.h"
#include "primer_correct.h"
#include "loci_constraints.h"
#include "read_loader.h"
#include "contaminants.h"
#include "report.h"
#include "coverage.h"
#include "duplicates.h"
#include "junctions.h"

namespace {
using namespace bkcli;

// long_no_val: keys of long-only options that take no value (every other key of more than one character takes one)
bool parse_args(int argc, char **argv, int first, const std::map<std::string, std::string> &longnames,
                const std::string &flags_with_val, const std::string &flags_no_val, Args &out, std::string &err, const std::set<std::string> &long_no_val = {})
{
    for (int i = first; i < argc; i++) {
        std::string a = argv[i];
        if (a.size() >= 2 && a[0] == '-' && a[1] == '-') {
            std::string name = a.substr(2), val;
            bool hasval = false;
            size_t eq = name.find('=');
            if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); hasval = true; }
            auto it = longnames.find(name);
            if (it == longnames.end()) { err = "unknown option --" + name; return false; }
            std::string key = it->second;
            bool wants = flags_with_val.find(key) != std::string::npos || key.size() > 1;
            if (flags_no_val.find(key) != std::string::npos && key.size() == 1) wants = false;
            if (long_no_val.count(key)) {
                if (hasval) { err = "option --" + name + " takes no value"; return false; }
                wants = false;
            }
            if (wants && !hasval) {
                if (i + 1 >= argc) { err = "option --" + name + " needs a value"; return false; }
                val = argv[++i];
            }
            out.v[key].push_back(wants ? val : "1");
        } else if (a.size() >= 2 && a[0] == '-') {
            std::string key(1, a[1]);
            if (flags_no_val.find(key) != std::string::npos) { out.v[key].push_back("1"); continue; }
            if (flags_with_val.find(key) == std::string::npos) { err = "unknown option " + a; return false; }
            std::string val = a.substr(2);
            if (val.empty()) {
                if (i + 1 >= argc) { err = "option " + a + " needs a value"; return false; }
                val = argv[++i];
            }
            out.v[key].push_back(val);
        } else {
            err = "unexpected argument '" + a + "'";
            return false;
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// index

int cmd_index(int argc, char **argv, int first)
{
    Args a;
    std::string err;
    std::map<std::string, std::string> ln = {{"mode", "m"}, {"minseqlen", "l"}, {"descr", "d"}, {"title", "t"}, {"ref", "r"},
                                             {"threads", "T"}, {"log", "F"}, {"FileLogLevel", "f"}, {"device", "device"}};
    if (!parse_args(argc, argv, first, ln, "mlidtroTFf", "", a, err)) {
        fprintf(stderr, "%s index: %s\n", g_proc.c_str(), err.c_str());
        return 1;
    }
    if (!a.has("i") || !a.has("o") || !a.has("r")) {
        fprintf(stderr, "usage: %s index -i <fasta[.gz]> [-i <fasta>..] -o <out.sfx> -r <refspecies> [-l minseqlen] [-d descr] [-t title] [-T threads] [--device n]\n", g_proc.c_str());
        return 1;
    }
    if (a.has("F")) g_logfile = fopen(a.str("F").c_str(), "a");
    if (a.num("m", 0) != 0) { diag("Error: only standard indexing mode '-m0' is supported"); return 1; }
    int min_seq_len = a.has("l") ? a.num("l", 50) : 50;                  // kangax.cpp:275-280
    min_seq_len = std::max(1, std::min(1000000, min_seq_len));
    std::string ref = a.str("r").substr(0, 80);
    std::string title = a.has("t") ? a.str("t").substr(0, 63) : ref.substr(0, 63);
    std::string descr = a.has("d") ? a.str("d").substr(0, 1023) : ref;
    diag("Subprocess index Version %s starting", kProgVer);

    // CreateBioseqSuffixFile / ProcessFastaFile (kangax.cpp:545-690,774-926): genome_loader.cpp
    std::vector<std::string> files = a.v["i"];
    std::sort(files.begin(), files.end());                               // SG_GLOB_FULLSORT
    int nthreads = a.num("T", 0);
    if (nthreads <= 0) nthreads = effective_cpus();
    // (BK_TIMING=1: the stages' wall-clock on stderr)
    const bool timing = bk::env::timing();
    timespec ts0;
    clock_gettime(CLOCK_MONOTONIC, &ts0);
    auto lap = [&](const char *what) {
        if (!timing) return;
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        fprintf(stderr, "bk timing: index: %-44s %8.1f ms\n", what, 1e3 * (double)(ts.tv_sec - ts0.tv_sec) + 1e-6 * (double)(ts.tv_nsec - ts0.tv_nsec));
        ts0 = ts;
    };
    Genome G;
    if (load_genome(files, min_seq_len, std::max(1, std::min(nthreads, 128)), G)) return 1;
    lap("genome files taken in (parse, N runs)");
    bk::RawVec<uint8_t> &seq = G.seq;
    std::vector<bk::SfxEntry> &entries = G.entries;
    const uint32_t n_under = G.n_under;
    if (n_under) diag("ProcessFastaFile - %u sequences not accepted for indexing as length under %dbp ", n_under, min_seq_len);
    if (entries.empty()) { diag("Nothing to index"); return 1; }

    diag("CreateBioseqSuffixFile: sorting suffix array...");
    uint64_t n = seq.size();
    uint32_t el = n < bk::kThres5ByteEls ? 4 : 5;
    int dev = a.num("device", 0);
    if (bk_device_count() < 1) { diag("Fatal: no HIP device - the suffix sort runs on the GPU only"); return 1; }
    if (hipSetDevice(dev) != hipSuccess) { diag("Fatal: unable to select HIP device %d", dev); return 1; }
    uint8_t *d_seq = nullptr, *d_sa = nullptr;
    if (hipMalloc(&d_seq, n) != hipSuccess || hipMalloc(&d_sa, n * el) != hipSuccess) { diag("Fatal: unable to allocate device memory"); return 1; }
    if (hipMemcpy(d_seq, seq.data(), n, hipMemcpyHostToDevice) != hipSuccess) { diag("Fatal: upload failed"); return 1; }
    lap("HIP start-up, device buffers, bases uploaded");
    int rc = bk_build_sa_device(d_seq, n, d_sa, (int)el, dev);
    if (rc) { diag("Fatal: suffix sort failed: %s", bk_strerror(rc)); return 1; }
    lap("suffix array sorted on the device");
    bk::RawVec<uint8_t> sa;                                              // (12 GB for a human genome: sized, not zeroed first)
    sa.resize(n * el);
    if (hipMemcpy(sa.data(), d_sa, n * el, hipMemcpyDeviceToHost) != hipSuccess) { diag("Fatal: download failed"); return 1; }
    lap("suffix array downloaded (pageable)");
    (void)hipFree(d_seq);
    (void)hipFree(d_sa);
    lap("device buffers given back");
    rc = bk::sfx_write(a.str("o").c_str(), ref, descr, title, entries, seq.data(), n, sa.data(), el, &err, std::max(1, std::min(nthreads, 16)));
    if (rc) { diag("Fatal: %s", err.c_str()); return 1; }
    lap(".sfx written");
    diag("CreateBioseqSuffixFile: completed...");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// align

// BK_TIMING=1: wall-clock of the front end's own stages on stderr (the library prints its own)
struct HostClock {
    bool on = bk::env::timing();
    double t0 = now();
    static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
    static double wall() { timespec ts; clock_gettime(CLOCK_REALTIME, &ts); return (double)(ts.tv_sec % 60) + 1e-9 * (double)ts.tv_nsec; }      // (the log's seconds)
    void lap(const char *what) { if (!on) return; const double t = now(); fprintf(stderr, "bk timing: host: %-40s %7.1f ms   (done at :%06.3f)\n", what, 1e3 * (t - t0), wall()); t0 = t; }
};

// The loaders' contaminant matcher (read_loader.h) on a device: bk_contam_* of the library.  A file without a single sequence makes a matcher
// that cuts nothing (the reference then still prints its count lines).
struct DeviceContam : ContamMatcher {
    bk_contam *h = nullptr;
    ~DeviceContam() override { destroy(); }
    void destroy() { if (h) bk_contam_destroy(h); h = nullptr; }
    int create(int device, const std::vector<ContamEntry> &entries)
    {
        if (entries.empty()) return BK_OK;
        std::vector<bk_contam_entry> e(entries.size());
        for (size_t i = 0; i < entries.size(); i++) { e[i].bases = entries[i].bases.data(); e[i].len = (uint32_t)entries[i].bases.size(); e[i].use = (uint32_t)entries[i].use; }
        return bk_contam_create(&h, device, e.data(), (uint32_t)e.size());
    }
    int match(const uint8_t *bases, const uint32_t *lens, size_t n, bool pe2, int trim5, int trim3, uint16_t *out) override
    {
        if (!h) { memset(out, 0, 4 * n); return 0; }
        const int rc = bk_contam_match(h, bases, nullptr, lens, n, nullptr, pe2 ? 1 : 0, trim5, trim3, out);
        if (rc) diag("Load: the contaminant matcher failed: %s", bk_strerror(rc));
        return rc;
    }
};

// Everything `biokanga align` was asked for, validated the way kanga.cpp:298-1066 validates it
struct AlignOpts {
    int pe_mode = 0, ml_mode = 0, max_ml = 1, micro_indel = 0, splice_len = 0, min_chim = 0, pcr_win = -1, min_flank = 0, fmt = 5;
    int min_len = 50, max_len = 500, trim5 = 0, trim3 = 0, max_rpt_sam_seqs = 10000, nthreads = 1;
    bool clamp_ml = false, best_matches = false;
    bk_pe_params PE{};
    bk_align_params P{};
    SnpOpts snp;
    std::string site_prefs_path;           // -8: start-site octamer preferences into this file (empty: none)
    int site_prefs_ofs = -4;               // -9, cDfltRelSiteStartOfs
    std::string constraints_path;          // -5: loci base constraints from this CSV file (empty: none)
    int primer_subs = 0;                   // -6: align at min(-s + this, 15), then correct 5' primer artefacts back under -s (0: off)
    int user_subs = 10;                    // -s as given (m_MaxSubs); P.max_subs is the rate the reads are aligned at (m_InitalAlignSubs)
    std::vector<regex_t> re_excl, re_incl;
    int sam_tags = 0;                      // --sam-tags: mask of BK_SAMTAG_NM | BK_SAMTAG_MD written behind QUAL of accepted records (0: none, the reference's lines)
    uint64_t sam_tag_bytes() const { return ((sam_tags & BK_SAMTAG_NM) ? 8u : 0u) + ((sam_tags & BK_SAMTAG_MD) ? 16u : 0u); }      // .. about what they add to a line
    std::string coverage_path;             // --coverage: per-base depth of the accepted records into this bedGraph (empty: none; made on the first device)
    bool mark_dups = false;                // --mark-duplicates: FLAG 0x400 on the records of duplicate templates (grouped on the first device)
    std::string junctions_path;            // --junctions: the junction table of the spliced records into this file (empty: none; made on the first device)
    bool splice_strand = false;            // --splice-strand: XS:A:+ / XS:A:- on spliced records whose junction has a stranded motif
    std::vector<int> devices;              // --device n | --devices a,b,c | a-b: one context (+ upload / align / download pipeline) per entry
};

// 0, or 1 after the error message has been logged
int read_align_opts(Args &a, AlignOpts &o)
{
    o.pe_mode = a.num("U", 0);
    if (o.pe_mode < 0 || o.pe_mode > 4) { diag("Error: paired end processing mode '-U%d' must be in range 0..4", o.pe_mode); return 1; }
    if (o.pe_mode && (!a.has("u") || a.v["u"].size() != a.v["i"].size())) {
        diag("Error: paired end processing '-U%d' needs as many '-u' PE2 files as '-i' PE1 files", o.pe_mode);
        return 1;
    }
    o.PE = bk_pe_params{};
    o.PE.pe_mode = o.pe_mode;
    o.PE.pair_min_len = a.num("d", 100);            // cDfltPairMinLen
    o.PE.pair_max_len = a.num("D", 1000);           // cDfltPairMaxLen
    o.PE.pair_strand = a.has("E") ? 1 : 0;
    if (o.pe_mode && (o.PE.pair_min_len < 25 || o.PE.pair_max_len < o.PE.pair_min_len || o.PE.pair_max_len > 100000)) {
        diag("Error: paired end insert size range '-d%d -D%d' not accepted", o.PE.pair_min_len, o.PE.pair_max_len);
        return 1;
    }
    // -r multi-loci modes (kanga.cpp:482-486,535-539,666-694): 0 slough, 1 stats only, 2 random pick, 3 cluster with
    // uniques, 4 cluster with uniques + other multi-loci reads, 5 report all loci; -R loci limit, -X clamp
    o.ml_mode = a.num("r", 0);
    if (o.ml_mode < 0 || o.ml_mode > 5) { diag("Error: multiple aligned reads processing mode '-r%d' specified outside of range 0..5", o.ml_mode); return 1; }
    if (o.pe_mode && o.ml_mode) { diag("Error: Sorry, currently multiloci processing '-r%d' not supported in paired end '-U%d' processing", o.ml_mode, o.pe_mode); return 1; }
    o.max_ml = 1;

    if (o.ml_mode) {
        o.max_ml = a.num("R", 5);                                         // cDfltMaxMultiHits
        const int lim = o.ml_mode == 5 ? 100000 : 500;                    // cMaxAllHits / cMaxMultiHits
        if (o.max_ml < 2 || o.max_ml > lim) { diag("Error: multiple aligned reads '-R%d' specified outside of range 2..%d", o.max_ml, lim); return 1; }
        if (o.max_ml > BK_MAX_ML) { diag("Error: '-R%d' is above the %d loci per read this build keeps", o.max_ml, BK_MAX_ML); return 1; }
        o.best_matches = a.has("N");                                      // bLocateBestMatches (implies the clamp, kanga.cpp:686-694)
        o.clamp_ml = a.has("X") || o.best_matches;
    }
    // -g FASTQ quality scores: 0 Sanger / Illumina 1.8+, 1 Illumina 1.3+, 2 Solexa, 3 ignore (default; QUAL is then '*')
    g_sample_nth = a.num("#", 1);
    if (g_sample_nth < 1 || g_sample_nth > 10000) { diag("Error: sample every Nth raw read '-#%d' specified outside of range 1..10000", g_sample_nth); return 1; }
    g_qual_mode = a.num("g", 3);
    if (g_qual_mode < 0 || g_qual_mode > 3) { diag("Error: fastq quality '-g%d' specified outside of range 0..3", g_qual_mode); return 1; }
    // -a microInDels (kanga.cpp:696-710): looked for in reads the substitution-only phases leave unaligned
    o.micro_indel = a.num("a", 0);
    if (o.micro_indel < 0 || o.micro_indel > 20) { diag("Error: microInDel length maximum '-a%d' specified outside of range 0..20", o.micro_indel); return 1; }
    if (o.micro_indel && o.ml_mode == 5) { diag("Error: microInDels not supported when reporting multiloci alignments"); return 1; }
    if (o.micro_indel && o.pe_mode) { diag("Error: Sorry, currently microInDel processing '-a%d' not supported in paired end '-U%d' processing", o.micro_indel, o.pe_mode); return 1; }   // kanga.cpp:541-545
    // -x: trim aligned reads back from both ends until that many consecutive bases match (CAligner::AutoTrimFlanks)
    // -A RNA-seq splice junctions (kanga.cpp:726-742,810-811): looked for after the microInDel pass; switches flank trimming on
    o.splice_len = a.num("A", 0);
    if (o.splice_len != 0 && (o.splice_len < 25 || o.splice_len > 100000)) { diag("Error: RNAseq maximum splice junction separation '-A%d' must be either 0 or in the range 25..100000", o.splice_len); return 1; }
    if (o.splice_len && o.ml_mode == 5) { diag("Error: in report all multiloci mode '-r5', there is no splice junction processing.."); return 1; }
    if (o.splice_len && o.pe_mode) { diag("Error: Sorry, currently RNA-seq splice junction processing '-A%d' not supported in paired end '-U%d' processing", o.splice_len, o.pe_mode); return 1; }
    // -c chimeric trimming (kanga.cpp:648-664): reads nothing else aligned may be placed with their ends trimmed off
    o.min_chim = a.num("c", 0);
    if (o.min_chim != 0 && (o.min_chim < 50 || o.min_chim > 99)) { diag("Error: minimum chimeric length percentage '-c%d' specified outside of range 50..99", o.min_chim < 0 ? -o.min_chim : o.min_chim); return 1; }
    // (-c with -N: the reference refuses it itself, kanga.cpp:712-716)
    if (o.min_chim && o.ml_mode && a.has("N")) {
        diag("Error: Sorry, chimeric read processing not supported in this release if either SOLiD or locating multiple best matches also requested");
        return 1;
    }
    // (-c with -r1..4 and -a / -A: AlignReads runs the microInDel / splice junction searches between the substitution-only phases and the
    // chimeric call on one set of counts and hits, SfxArrayV2.cpp:7722-7757 - five reference runs byte-identical, tests/golden/chimmlindel)
    // -p / -P / -1 / -S SNP calling (kanga.cpp:866-925)

    o.snp.min_reads = a.num("p", 0);
    if (o.snp.min_reads != 0 && (o.snp.min_reads < 1 || o.snp.min_reads > 100)) { diag("Error: Minimum read coverage at any loci '-p%d' must be in range 1..100", o.snp.min_reads); return 1; }
    if (o.snp.min_reads > 0) {
        o.snp.qvalue = a.has("P") ? atof(a.str("P").c_str()) : 0.0;
        if (o.snp.qvalue < 0.0 || o.snp.qvalue > 0.40) { diag("Error: QValue '-P%1.5f' for controlling SNP FDR (Benjamini-Hochberg) must be in range 0.0 to 0.4", o.snp.qvalue); return 1; }
        if (o.snp.qvalue == 0.0) o.snp.qvalue = 0.05;
        const double pcnt = a.has("1") ? atof(a.str("1").c_str()) : 25.0;
        if (pcnt < 0.1 || pcnt > 35.0) { diag("Error: SNP minimum non-ref '-1%f' for controlling SNP FDR must be in range 0.1 to 35.0", pcnt); return 1; }
        o.snp.nonref_prop = pcnt / 100.0;
        if (o.ml_mode == 5) { diag("Error: SNP processing not currently supported if reporting multiloci alignments"); return 1; }
        o.snp.marker_len = a.num("K", 0);                    // kanga.cpp:928-952
        o.snp.centroid_path = a.str("7", "");                // kanga.cpp:954-960
        if (o.snp.marker_len != 0 && (o.snp.marker_len < 25 || o.snp.marker_len > 500)) { diag("Error: Marker length specified with '-K%d' must be in range 25 to 500", o.snp.marker_len); return 1; }
        if (o.snp.marker_len) {
            o.snp.marker_poly_thres = a.has("G") ? atof(a.str("G").c_str()) : (1.0 / 3.0);
            if (o.snp.marker_poly_thres < 0.0 || o.snp.marker_poly_thres > 0.50) { diag("Error: Max marker sequence base poymorphism specified with '-G%1.3f' must be in range 0.0 to 0.5", o.snp.marker_poly_thres); return 1; }
        }
    }
    // -k PCR differential amplification artefact reduction (kanga.cpp:718-724): window 0..250, off by default
    o.pcr_win = a.has("k") ? a.num("k", -1) : -1;
    if (a.has("k") && (o.pcr_win < 0 || o.pcr_win > 250)) { diag("Error: PCR differential amplification artefacts window length '-k%d' specified outside of range 0..250", o.pcr_win); return 1; }
    // -Z / -z chromosome exclude / include filters: POSIX extended regular expressions, case-insensitive (Aligner.cpp:4770-4795)

    for (const char *opt : {"Z", "z"})
        if (a.has(opt))
            for (const std::string &pat : a.v[opt]) {
                regex_t re;
                if (regcomp(&re, pat.c_str(), REG_EXTENDED | REG_ICASE)) { diag("Error: ProcessAlign: %s chrom RE '%s' error", opt[0] == 'Z' ? "exclude" : "include", pat.c_str()); return 1; }
                (opt[0] == 'Z' ? o.re_excl : o.re_incl).push_back(re);
            }
    // (with -U the reference consults the filters inside its pair rules, AcceptThisChromID at Aligner.cpp:2771-2786,3224,3323,3445: not built)
    o.min_flank = a.num("x", 0);
    if (o.min_flank < 0 || o.min_flank > 7) { diag("Error: Max flank trimming '-x%d' specified outside of range 0..7", o.min_flank); return 1; }      // cMaxAllowedSubs / 2
    o.P = bk_align_params{};
    // with -N the reads go through LocateBestMatches, which has no microInDel / splice junction branches (Aligner.cpp:9197-9218): the
    // options are accepted as the reference accepts them and only their host-side consequences remain (-A still switches flank trimming on)
    o.P.micro_indel_len = o.best_matches ? 0 : o.micro_indel;
    o.P.splice_junct_len = o.best_matches ? 0 : o.splice_len;
    o.P.pmode = a.num("m", 0);
    o.P.align_strand = a.num("Q", 0);
    o.P.min_edit_dist = a.num("e", 1);
    o.P.max_subs = o.user_subs = a.num("s", 10);    // cDfltAllowedSubs per 100bp
    if (o.splice_len > 0 && o.min_chim == 0 && o.min_flank == 0) o.min_flank = o.P.max_subs;      // MinFlankExacts = MaxSubs (kanga.cpp:810-811)
    // -6 5' primer artefact correction (kanga.cpp:784-795): the reads are aligned at the initial rate, the orphan recovery's cores and
    // the correction pass keep the user's (Aligner.cpp:208-213,3256,611)
    o.primer_subs = a.num("6", 0);
    if (o.primer_subs < 0 || o.primer_subs > bk::kMaxPrimerSubs) {
        diag("Error: PCR primer correction subs '-6%d' specified outside of range 0..%d\n", o.primer_subs, bk::kMaxPrimerSubs);
        return 1;
    }
    if (o.primer_subs != 0 && o.min_chim != 0) { diag("Error: PCR primer correction subs not allowed when also specifying chimeric trimming\n"); return 1; }
    if (o.primer_subs != 0 && o.ml_mode == 5) {
        // (every locus of a read is a record of its own there, each corrected against its own locus in a copy of the read the reference
        // makes for it: the records here share their read's bases)
        diag("Error: PCR primer correction subs '-6%d' is not available when reporting all multiloci alignments '-r5'", o.primer_subs);
        return 1;
    }
    if (o.primer_subs != 0) {
        if (o.user_subs < 0 || o.user_subs > bk::kMaxAllowedSubs) {
            diag("Error: Max allowed substitutions per 100bp read length '-s%d' specified outside of range %d..%d\n", o.user_subs, 0, bk::kMaxAllowedSubs);
            return 1;
        }
        o.P.max_subs = bk::primer_initial_subs(o.user_subs, o.primer_subs);
        o.P.orphan_core_subs1 = o.user_subs + 1;
    }
    o.P.min_chimeric_len = o.min_chim;
    o.P.max_ns = a.num("n", 1);
    o.P.max_ml = o.max_ml;
    o.P.clamp_ml = o.clamp_ml ? 1 : 0;
    o.P.best_matches = o.best_matches ? 1 : 0;
    o.fmt = a.num("M", 5);
    if (o.ml_mode == 5 && !(o.fmt == 0 || o.fmt == 4 || o.fmt == 5 || o.fmt == 6)) {      // kanga.cpp:830-834
        diag("Error: reporting all multiloci alignments '-r5' is only available with output formats '-M0', '-M4', '-M5' and '-M6'");
        return 1;
    }
    // --sam-tags NM | MD | NM,MD (ours: the reference writes no optional field on an accepted record)
    if (a.has("sam-tags")) {
        const std::string spec = a.str("sam-tags");
        for (size_t at = 0; at <= spec.size();) {
            size_t end = spec.find(',', at);
            if (end == std::string::npos) end = spec.size();
            const std::string name = spec.substr(at, end - at);
            if (name == "NM") o.sam_tags |= BK_SAMTAG_NM;
            else if (name == "MD") o.sam_tags |= BK_SAMTAG_MD;
            else {
                diag("Error: SAM tags '--sam-tags %s' must be a list of NM and MD ('%s' is neither)", spec.c_str(), name.c_str());
                return 1;
            }
            at = end + 1;
        }
        if (o.fmt >= 0 && o.fmt <= 4) {
            diag("Error: SAM tags '--sam-tags %s' are only available with SAM / BAM output formats '-M5' and '-M6'", spec.c_str());
            return 1;
        }
    }
    // --coverage <file> (ours: the depth of the final record set, whatever the output format)
    if (a.has("coverage")) {
        o.coverage_path = a.str("coverage");
        if (o.coverage_path.empty()) { diag("Error: coverage file '--coverage' needs a file name"); return 1; }
        if (o.coverage_path == a.str("o")) { diag("Error: coverage file '--coverage %s' is the output file '-o' itself", o.coverage_path.c_str()); return 1; }
    }
    // --mark-duplicates (ours: the reference's -k removes single-end reads by start, strand and length)
    if (a.has("mark-duplicates")) {
        o.mark_dups = true;
        if (o.fmt >= 0 && o.fmt <= 4) {
            diag("Error: duplicate marking '--mark-duplicates' is only available with SAM / BAM output formats '-M5' and '-M6'");
            return 1;
        }
        if (o.ml_mode == 5) {
            diag("Error: duplicate marking '--mark-duplicates' is not available when reporting all multiloci alignments '-r5'");
            return 1;
        }
    }
    // --junctions <file>, --splice-strand (ours: the reference writes a BED line per spliced read, with the read's strand)
    if (a.has("junctions")) {
        o.junctions_path = a.str("junctions");
        std::string jp = a.str("o");
        if (is_gz_name(jp)) jp.resize(jp.size() - 3);
        if (o.junctions_path.empty()) { diag("Error: junction table '--junctions' needs a file name"); return 1; }
        if (o.junctions_path == a.str("o")) { diag("Error: junction table '--junctions %s' is the output file '-o' itself", o.junctions_path.c_str()); return 1; }
        if (o.junctions_path == a.str("o") + ".jct" || o.junctions_path == jp + ".jct") {
            diag("Error: junction table '--junctions %s' is the junction BED file of '-o' itself", o.junctions_path.c_str());
            return 1;
        }
        if (!o.splice_len) { diag("Error: junction table '--junctions' needs RNAseq splice junction processing '-A<len>'"); return 1; }
    }
    if (a.has("splice-strand")) {
        o.splice_strand = true;
        if (o.fmt >= 0 && o.fmt <= 4) {
            diag("Error: transcript strand tags '--splice-strand' are only available with SAM / BAM output formats '-M5' and '-M6'");
            return 1;
        }
        if (!o.splice_len) { diag("Error: transcript strand tags '--splice-strand' need RNAseq splice junction processing '-A<len>'"); return 1; }
    }
    if (a.has("O") && o.fmt == 6) {                 // kanga.cpp:1015-1021
        diag("Error: Output induced substitution mode '-O<file>' not available in '-M6' output mode\n");
        return 1;
    }
    // -8 / -9 start-site octamer preferences (kanga.cpp:1029-1043)
    o.site_prefs_ofs = a.has("9") ? a.num("9", -4) : -4;
    if (abs(o.site_prefs_ofs) > BK_SITE_MAX_OFS) {
        diag("Error: offset read start sites '-9%d' when processing site octamer preferencing must be in range -100..100\n", o.site_prefs_ofs);
        return 1;
    }
    if (a.has("8")) {
        o.site_prefs_path = a.str("8");
        while (!o.site_prefs_path.empty() && (o.site_prefs_path.front() == '"' || o.site_prefs_path.front() == '\'')) o.site_prefs_path.erase(0, 1);      // CUtility::TrimQuotes
        while (!o.site_prefs_path.empty() && (o.site_prefs_path.back() == '"' || o.site_prefs_path.back() == '\'')) o.site_prefs_path.pop_back();
    }
    if (a.has("5")) o.constraints_path = a.str("5");        // (kanga.cpp:998-1004: the name as given)
    o.min_len = a.num("l", 50), o.max_len = a.num("L", 500);
    o.trim5 = a.num("y", 0), o.trim3 = a.num("Y", 0);
    o.max_rpt_sam_seqs = a.num("4", 10000);
    // -T: host threads for parsing, sorting and formatting (0 = all cores, capped like the reference's cMaxWorkerThreads)
    o.nthreads = a.num("T", 0);
    if (o.nthreads <= 0) o.nthreads = effective_cpus();                  // the cores the process may really use (cgroup quota included)
    if (o.nthreads < 1) o.nthreads = 1;
    if (o.nthreads > 128) o.nthreads = 128;
    if (o.P.pmode < 0 || o.P.pmode > 3 || o.P.align_strand < 0 || o.P.align_strand > 2 || o.P.min_edit_dist < 1 || o.P.min_edit_dist > 2 ||
        o.P.max_subs < 0 || o.P.max_subs > 25 || o.P.max_ns < 0 || o.P.max_ns > 5 || o.min_len < 15 || o.min_len > 2000 || o.max_len < o.min_len ||
        o.max_len > 2000 || o.fmt < 0 || o.fmt > 6) {
        diag("Error: an option value is outside its accepted range");
        return 1;
    }
    // --device n (one GPU) or --devices 0-7 / 0,1,2: the read batches are dealt round-robin over one context per entry
    if (a.has("devices")) {
        const std::string spec = a.str("devices");
        size_t at = 0;
        while (at < spec.size()) {
            size_t end = spec.find(',', at);
            if (end == std::string::npos) end = spec.size();
            const std::string part = spec.substr(at, end - at);
            const size_t dash = part.find('-');
            const int lo = atoi(part.c_str()), hi = dash == std::string::npos ? lo : atoi(part.c_str() + dash + 1);
            if (part.empty() || lo < 0 || hi < lo || hi > 1023) { diag("Error: '--devices %s' is not a list of device numbers / ranges", spec.c_str()); return 1; }
            for (int d = lo; d <= hi; d++) o.devices.push_back(d);
            at = end + 1;
        }
    } else
        o.devices.push_back(a.num("device", 0));
    if (o.devices.empty() || o.devices.size() > 64) { diag("Error: between 1 and 64 devices can be used"); return 1; }
    return 0;
}

// Long runs - from this many reads per device on - are cut into larger batches.
constexpr unsigned long long kLongRunMinReads = 600000000ULL;
// The index image a job gets - the suffix-ordered window array (a sixth of a 3.1 Gbp index, 25 GB), the k-mer table's second words, the
// third- and fourth-level search keys: all made behind the suffix array's upload, slice by slice while the next slice crosses PCIe -
// follows the library's one rule, bk_image_policy(reads per device): everything from BK_POLICY_MIN_READS reads on (0.1 - 0.2 s more load
// on a 3.1 Gbp index for 0.7 ns less per read of a hundred bases), the lean image that grows should the run turn out long below.
// bench.py measures its headline on the image this rule picks.

// what the alignment pass leaves for the policies above the boundary
struct AlignedSet {
    std::vector<bk_hit> hits;                      // one per read, load order
    std::vector<uint64_t> l_offs;                  // multi-loci modes: read i owns loci [l_offs[i], l_offs[i+1])
    std::vector<bk_loci> loci;
    std::vector<bk_loci_trims> loci_trims;         // -c with the multi-loci modes: end trims of every locus (else empty)
    std::vector<bk_seg2> seg2;                     // -a / -A / -c: second segment of each read (flags 0 = none)
    std::vector<uint64_t> seq_counts;              // per sequence: reads the SE pass accepted, summed over the devices (RCCL when > 1)
};


// The reads as they cross the boundary (the reference's loader hands its workers 1 byte/base, Aligner.cpp:9038-9055, of which three bits
// reach the hot path): 2 bit/base words + 16-bit lengths + the bases that are not a,c,g,t (bk_pack_reads), cut into the batches the
// pipelines will be fed, in page-locked memory - made by the host threads while the index image is still on its way to the device.
struct Submission {
    struct Batch { size_t lo, hi; uint64_t w0, w1, e0, e1, ticket; };
    std::vector<Batch> batches;
    uint32_t *words = nullptr;
    uint16_t *lens16 = nullptr;
    bk_nbase *exc = nullptr;
    uint64_t n_words = 0, cap_exc = 0, max_words = 1;
    uint64_t cap_words = 0, cap_lens = 0;          // what `early` made room for
    size_t max_reads = 1;
    uint32_t max_len = 0;
    void *registered = nullptr;                    // the result array, page-locked in place while results arrive in it
    // Page-locking memory is slow (0.2 s per GB with the parser's threads running): for plain-text inputs the buffers are made by a
    // thread of their own from the moment the input files' sizes are known - a read's words cannot outnumber its bytes in the file / 16
    std::thread early;
    void start_early(uint64_t input_bytes, uint32_t min_len)
    {
        early = std::thread([this, input_bytes, min_len]() {
            const uint64_t w = input_bytes / 16 + 4096, r = input_bytes / ((uint64_t)min_len + 3) + 4096, e = input_bytes / 448 + (1u << 20);
            words = (uint32_t *)bk_host_alloc((w + 64) * 4);
            lens16 = (uint16_t *)bk_host_alloc((r + 64) * 2);
            exc = (bk_nbase *)bk_host_alloc(e * sizeof(bk_nbase));
            if (words && lens16 && exc) { cap_words = w; cap_lens = r; cap_exc = e; }
            else { bk_host_free(words); bk_host_free(lens16); bk_host_free(exc); words = nullptr; lens16 = nullptr; exc = nullptr; }
        });
    }
    void release_results() { if (registered) { bk_host_unregister(registered); registered = nullptr; } }
    // the packed reads have served once the last batch is back: their page-locked memory is given back (0.18 s per GB) by a thread of its
    // own while the records are sorted, instead of at the end of the run
    std::thread releaser;
    std::vector<bk_nbase> exc_job;                 // the exceptions of all batches with `read` counting from the first read of the run
    // (with a SAM head start that reads the packed form: once that has taken it to the device; kept if the head start failed - the
    // formatter then uploads for itself)
    void release_packed_in_background(bk_sam_prep *after = nullptr, std::function<void()> then = nullptr)
    {
        if (early.joinable()) early.join();
        uint32_t *w = words; uint16_t *l = lens16; bk_nbase *e = exc;
        words = nullptr; lens16 = nullptr; exc = nullptr; cap_words = cap_lens = cap_exc = 0;
        looked = std::async(std::launch::deferred, []() {});       // (reset below when there is a head start to look at)
        if (after != nullptr) {
            auto seen = std::make_shared<std::promise<void>>();
            looked = seen->get_future();
            releaser = std::thread([w, l, e, after, seen, then]() {
                const int rc = bk_sam_prep_wait(after);
                seen->set_value();                      // (`after` may be consumed from here on)
                if (rc != BK_OK) return;
                if (then) then();
                bk_host_free(w); bk_host_free(l); bk_host_free(e);
            });
        } else
            releaser = std::thread([w, l, e]() { bk_host_free(w); bk_host_free(l); bk_host_free(e); });
    }
    std::future<void> looked;                      // ready once the releaser no longer needs the head start's handle
    void done_with_head_start() { if (looked.valid()) looked.wait(); }
    ~Submission()
    {
        if (early.joinable()) early.join();
        if (releaser.joinable()) releaser.join();
        release_results(); bk_host_free(words); bk_host_free(lens16); bk_host_free(exc);
    }
};

// Reads per batch.  A batch costs less per read the larger it is (every phase's wave-per-read launch lasts at least as long as its
// heaviest read: 3 M reads take 3.3 ns each, 12 M 2.2 ns, 50 M 2.0 ns) - but its scratch is allocated at 16 ms per GB (0.5 KB per
// read), and nothing overlaps the upload of a device's first batch.  Runs below the window array's threshold are over in a fraction
// of a second: 4 M reads first, then batches of 12 M; long runs grow to 32 M.  Small inputs: two batches per device.
int prepare_submission(const AlignOpts &o, const ReadStore &rs, size_t ndev, bool long_run, AlignedSet &A, Submission &S)
{
    const size_t nr = rs.size();
    HostClock clk;
    std::thread results([&]() {                    // (the record array is touched page by page: a thread of its own)
        HostClock c2;
        A.hits.reserve(nr);                        // (room first, marked for huge pages, then the records: 500 page faults per GB instead of 260 000)
        if (nr * sizeof(bk_hit) >= bk::kHugeFrom) {
            const uintptr_t lo = ((uintptr_t)A.hits.data() + bk::kHugePage - 1) & ~(uintptr_t)(bk::kHugePage - 1);
            const uintptr_t hi = ((uintptr_t)A.hits.data() + nr * sizeof(bk_hit)) & ~(uintptr_t)(bk::kHugePage - 1);
            if (hi > lo) (void)madvise((void *)lo, hi - lo, MADV_HUGEPAGE);
        }
        A.hits.resize(nr);
        c2.lap("result array sized");
        if (nr && bk_host_register(A.hits.data(), nr * sizeof(bk_hit)) == BK_OK) S.registered = A.hits.data();
        c2.lap("result array page-locked");
    });
    size_t per = long_run ? (32u << 20) : (12u << 20);
    const bool ramp = nr / ndev >= (12u << 20);
    if (!ramp) {
        per = 8u << 20;
        if (nr / ndev / 2 + 1 < per) per = std::max<size_t>(65536, nr / ndev / 2 + 1);
    }
    per += per & 1;
    for (size_t lo = 0, k = 0; lo < nr; k++) {
        size_t n = per;
        if (ramp) {
            const size_t round = k / ndev;                                           // this device's round-th batch
            n = round == 0 ? (4u << 20) : (round == 1 ? (12u << 20) : per);
        }
        if (nr - lo < n + n / 4) n = nr - lo;                                        // (no small last batch: it joins the one before)
        n += n & 1;
        Submission::Batch b{lo, std::min(nr, lo + n), 0, 0, 0, 0, 0};
        S.max_reads = std::max(S.max_reads, b.hi - b.lo);
        S.batches.push_back(b);
        lo = b.hi;
    }
    // words per batch (a read takes ceil(len / 16) of them), longest read
    {
        const int nt = std::max(1, std::min(o.nthreads, (int)S.batches.size()));
        std::vector<uint32_t> ml(S.batches.size(), 0);
        std::atomic<size_t> next{0};
        auto count = [&]() {
            for (size_t k; (k = next.fetch_add(1)) < S.batches.size();) {
                Submission::Batch &b = S.batches[k];
                uint64_t w = 0;
                uint32_t m = 0;
                for (size_t i = b.lo; i < b.hi; i++) { w += ((uint64_t)rs.lens[i] + 15) >> 4; m = std::max(m, rs.lens[i]); }
                b.w1 = w;
                ml[k] = m;
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < nt; t++) th.emplace_back(count);
        count();
        for (auto &t : th) t.join();
        uint64_t at = 0;
        for (size_t k = 0; k < S.batches.size(); k++) {
            Submission::Batch &b = S.batches[k];
            S.max_words = std::max(S.max_words, b.w1);
            b.w0 = at; at += b.w1; b.w1 = at;
            S.max_len = std::max(S.max_len, ml[k]);
        }
        S.n_words = at;
    }
    clk.lap("batches cut, words counted");
    if (S.early.joinable()) S.early.join();
    if (!(S.words && S.cap_words >= S.n_words && S.cap_lens >= nr)) {          // no head start, or one that guessed too low
        bk_host_free(S.words); bk_host_free(S.lens16); bk_host_free(S.exc);
        S.words = (uint32_t *)bk_host_alloc((S.n_words + 64) * 4);
        S.lens16 = (uint16_t *)bk_host_alloc((nr + 64) * 2);
        S.cap_exc = nr / 4 + (1u << 20);
        S.exc = (bk_nbase *)bk_host_alloc(S.cap_exc * sizeof(bk_nbase));
    }
    int rc = (S.words && S.lens16 && S.exc) ? BK_OK : BK_ERR_MEM;
    clk.lap("page-locked buffers for the packed reads");
    uint64_t e_at = 0;
    for (size_t k = 0; k < S.batches.size() && rc == BK_OK; k++) {
        Submission::Batch &b = S.batches[k];
        uint64_t n_exc = 0;
        rc = bk_pack_reads(rs.bases.data(), rs.offs.data() + b.lo, rs.lens.data() + b.lo, (uint32_t)(b.hi - b.lo), S.words + b.w0, S.lens16 + b.lo,
                           S.exc + e_at, S.cap_exc - e_at, &n_exc);
        if (rc == BK_ERR_MEM) {
            // more bases that are not a,c,g,t than room was made for: a larger list (what is packed so far is kept), this batch again
            const uint64_t cap2 = std::max<uint64_t>(2 * S.cap_exc, e_at + n_exc + (1u << 20));
            bk_nbase *e2 = (bk_nbase *)bk_host_alloc(cap2 * sizeof(bk_nbase));
            if (!e2) break;
            memcpy(e2, S.exc, e_at * sizeof(bk_nbase));
            bk_host_free(S.exc);
            S.exc = e2;
            S.cap_exc = cap2;
            rc = BK_OK;
            k--;
            continue;
        }
        b.e0 = e_at; e_at += n_exc; b.e1 = e_at;
    }
    if (rc == BK_OK) {
        S.exc_job.assign(S.exc, S.exc + e_at);
        for (const Submission::Batch &b : S.batches)
            for (uint64_t e = b.e0; e < b.e1; e++) S.exc_job[e].read += (uint32_t)b.lo;
    }
    clk.lap("reads packed to 2 bit/base");
    results.join();
    clk.lap("waited for the result array");
    if (rc) diag("Fatal: unable to pack the reads for the device: %s", bk_strerror(rc));
    return rc;
}

// CAligner::LocateCoredApprox over every loaded read: the packed batches go through one upload / align / download pipeline per device
// (bk_stream_*), batch b on device b mod N; with -U the paired-end association runs on the device-resident batch right after its SE
// pass (batches hold whole pairs).  Results land in load order whatever the number of devices, so everything downstream - the
// reference's sort order included - is the same as on one GPU.  The pipelines (their device buffers, the contexts' batch scratch)
// are set up by open_pipelines() BEFORE the clock of T_align starts: align_reads() only submits and collects.
int open_pipelines(const std::vector<bk_ctx *> &ctxs, const AlignOpts &o, const Submission &S, std::vector<bk_stream *> &st)
{
    st.assign(ctxs.size(), nullptr);
    std::vector<int> rcs(ctxs.size(), 0);
    std::vector<std::thread> th;
    for (size_t d = 0; d < ctxs.size(); d++)
        th.emplace_back([&, d]() {
            rcs[d] = bk_ctx_reserve(ctxs[d], (uint32_t)S.max_reads, std::max<uint32_t>(S.max_len, 16));
            if (!rcs[d]) rcs[d] = bk_stream_create_packed(&st[d], ctxs[d], (uint32_t)S.max_reads, S.max_words, 3, o.pe_mode ? &o.PE : nullptr);
        });
    for (auto &t : th) t.join();
    for (size_t d = 0; d < ctxs.size(); d++)
        if (rcs[d]) {
            diag("Fatal: unable to set up the device pipeline: %s", bk_strerror(rcs[d]));
            for (bk_stream *s : st) bk_stream_destroy(s);
            st.clear();
            return rcs[d];
        }
    return BK_OK;
}

int align_reads(const std::vector<bk_ctx *> &ctxs, std::vector<bk_stream *> &st, const AlignOpts &o, const ReadStore &rs, Submission &S, AlignedSet &A)
{
    const size_t ndev = ctxs.size();
    const bool lists = o.ml_mode != 0, segs = o.P.micro_indel_len || o.P.splice_junct_len || o.P.min_chimeric_len;
    if (lists) A.l_offs.assign(1, 0);
    std::vector<Submission::Batch> &batches = S.batches;
    auto close = [&]() { for (bk_stream *s : st) bk_stream_destroy(s); st.clear(); };
    auto collect = [&](size_t k) -> int {
        Submission::Batch &b = batches[k];
        bk_stream *s = st[k % ndev];
        int rc = bk_stream_wait(s, b.ticket);
        if (rc) { diag("Fatal: alignment failed: %s", bk_strerror(rc)); return rc; }
        const size_t n = b.hi - b.lo;
        if (segs) {
            const bk_seg2 *bs = nullptr;
            uint64_t ns = 0;
            rc = bk_stream_batch_seg2(s, b.ticket, &bs, &ns);
            if (rc || !bs || ns != n) { diag("Fatal: microInDel segments unavailable: %s", bk_strerror(rc)); return rc ? rc : BK_ERR_INTERNAL; }
            A.seg2.insert(A.seg2.end(), bs, bs + ns);
        }
        if (lists) {
            const uint64_t *bo = nullptr;
            const bk_loci *bl = nullptr;
            uint64_t nl = 0;
            rc = bk_stream_batch_loci(s, b.ticket, &bo, &bl, &nl);
            if (rc || !bo) { diag("Fatal: loci lists unavailable: %s", bk_strerror(rc)); return rc ? rc : BK_ERR_INTERNAL; }
            const uint64_t base = A.loci.size();
            for (size_t i = 1; i <= n; i++) A.l_offs.push_back(base + bo[i]);
            A.loci.insert(A.loci.end(), bl, bl + nl);
            if (o.P.min_chimeric_len) {
                const bk_loci_trims *bt = nullptr;
                uint64_t nt = 0;
                rc = bk_stream_batch_loci_trims(s, b.ticket, &bt, &nt);
                if (rc || (nl && (!bt || nt != nl))) { diag("Fatal: loci trims unavailable: %s", bk_strerror(rc)); return rc ? rc : BK_ERR_INTERNAL; }
                A.loci_trims.insert(A.loci_trims.end(), bt, bt + nt);
            }
        }
        if (segs || lists) bk_stream_release(s, b.ticket);
        return BK_OK;
    };
    // submit() blocks while a device's three buffer sets are busy, and a batch completes without being waited for, so the
    // loop below keeps every pipeline full; results are collected in load order, 3 * ndev batches behind the submissions
    size_t next_collect = 0;
    const size_t lag = 3 * ndev;
    for (size_t k = 0; k < batches.size(); k++) {
        Submission::Batch &b = batches[k];
        int rc = bk_stream_submit_packed(st[k % ndev], S.words + b.w0, b.w1 - b.w0, S.lens16 + b.lo, (uint32_t)(b.hi - b.lo), S.exc + b.e0, b.e1 - b.e0,
                                         A.hits.data() + b.lo, &b.ticket);
        if (rc) { diag("Fatal: alignment failed: %s", bk_strerror(rc)); close(); return rc; }
        while (next_collect + lag <= k) { rc = collect(next_collect++); if (rc) { close(); return rc; } }
    }
    while (next_collect < batches.size()) { int rc = collect(next_collect++); if (rc) { close(); return rc; } }
    // what crossed PCIe, and the pipelines' own clock (first batch submitted -> last result back, the slowest device)
    {
        bk_stream_stats tot{};
        for (bk_stream *s : st) {
            bk_stream_stats x{};
            if (bk_stream_get_stats(s, &x, 0) == BK_OK) {
                tot.batches += x.batches; tot.reads += x.reads; tot.bytes_h2d += x.bytes_h2d; tot.bytes_d2h += x.bytes_d2h;
                tot.seconds_first_submit_to_last_result = std::max(tot.seconds_first_submit_to_last_result, x.seconds_first_submit_to_last_result);
            }
        }
        if (tot.reads)
            diag("Device pipeline: %llu reads in %llu batches over %zu device(s), %.1f bytes per read host to device (2 bit/base), %.1f back, first submit to last result %.3f seconds",
                 (unsigned long long)tot.reads, (unsigned long long)tot.batches, ndev, (double)tot.bytes_h2d / (double)tot.reads, (double)tot.bytes_d2h / (double)tot.reads,
                 tot.seconds_first_submit_to_last_result);
    }
    close();
    // (the result array stays page-locked while nothing replaces it: the SAM formatter's upload of the records then is one DMA)
    if (o.ml_mode) S.release_results();
    // the path's one exchange step: per-sequence accepted-read counts summed over the devices
    A.seq_counts.assign(bk_num_entries(ctxs[0]), 0);
    int rc = bk_seq_counts_allreduce((bk_ctx *const *)ctxs.data(), (int)ndev, A.seq_counts.data(), (uint32_t)A.seq_counts.size(), 1);
    if (rc) { diag("Fatal: unable to reduce the per sequence hit counts over the devices: %s", bk_strerror(rc)); return rc; }
    return BK_OK;
}

// CAligner::ProcCoredApprox for MLMode != eMLdefault (Aligner.cpp:9241-9424): what becomes of the reads that aligned to more than one
// locus (-r1 statistics, -r2 random pick, -r3 / -r4 clustering, -r5 every locus its own record).  rec.src maps the records of -r5 back
// to their reads (the records then replace the reads in A.hits, which rec views).
// rec.rec_trims (with -c only): per record the end trims its placement carries - those of the locus chosen for it, or of the read's own
// unique chimeric placement.
void resolve_multi_loci(const AlignOpts &o, const ReadStore &rs, AlignedSet &A, bk::RecordSet &rec, std::vector<int> &multi_dist, const std::vector<uint8_t> *chrom_ok)
{
    std::vector<bk_hit> &hits = A.hits;
    std::vector<uint32_t> &src = rec.src;
    std::vector<bk_loci_trims> &rec_trims = rec.rec_trims;
    const size_t nr = hits.size();
    const std::vector<uint64_t> &l_offs = A.l_offs;
    const std::vector<bk_loci> &loci = A.loci;
    const bool with_trims = o.P.min_chimeric_len > 0;
    auto trims_of = [&](uint64_t locus) -> bk_loci_trims { return locus < A.loci_trims.size() ? A.loci_trims[locus] : bk_loci_trims{}; };
    if (with_trims) {
        rec_trims.assign(nr, bk_loci_trims{});
        for (size_t i = 0; i < nr && i < A.seg2.size(); i++)
            if (A.seg2[i].flags & 8) { rec_trims[i].left = A.seg2[i].match_len; rec_trims[i].right = A.seg2[i].read_ofs; rec_trims[i].chimeric = 1; }
    }
    // CAligner::ProcCoredApprox for MLMode != eMLdefault (Aligner.cpp:9241-9424); reads in load order, as -T1 runs them
    auto eff_count = [&](size_t i) -> uint32_t {            // LowHitInstances of a read that counts as eHRhits (after -X)
        const bk_hit &h = hits[i];
        if (h.rslt == BK_HR_HITS || (o.clamp_ml && h.rslt == BK_HR_HITINSTS)) return (uint32_t)(l_offs[i + 1] - l_offs[i]);
        return 0;
    };
    auto take = [&](bk_hit &h, const bk_loci &L) {
        h.chrom_id = L.chrom_id; h.match_loci = L.match_loci; h.match_len = L.match_len; h.strand = L.strand;
        h.mismatches = L.mismatches; h.nar = BK_NAR_ACCEPTED; h.num_hits = 1; h.low_hit_instances = 1;
    };
    uint64_t n_uniq = 0, n_multi = 0, n_loci = 0;
    for (size_t i = 0; i < nr; i++) {
        const uint32_t c = eff_count(i);
        if (!c) continue;
        n_loci += c;
        (c == 1 ? n_uniq : n_multi)++;
        if (o.ml_mode != 5) multi_dist[c - 1]++;
        if (o.clamp_ml && hits[i].rslt == BK_HR_HITINSTS) hits[i].low_hit_instances = (int16_t)c;
    }
    diag("Provisionally accepted %llu aligned reads (%llu uniquely, %llu aligning to multiloci) aligning to a total of %llu loci",
         (unsigned long long)(n_uniq + n_multi), (unsigned long long)n_uniq, (unsigned long long)n_multi, (unsigned long long)n_loci);
    if (o.ml_mode == 2) {
        // eMLrand: rand() % LowHitInstances for every eHRhits read, unique ones included (:9365-9366); the sequence is
        // glibc's unseeded one (glibc_rand.h), which is what a single-threaded reference run consumes in the same order
        bk::GlibcRand pick;
        for (size_t i = 0; i < nr; i++) {
            const uint32_t c = eff_count(i);
            if (!c) continue;
            const uint32_t k = (uint32_t)pick.next() % c;
            take(hits[i], loci[l_offs[i] + k]);
            if (with_trims) rec_trims[i] = trims_of(l_offs[i] + k);
        }
    } else if (o.ml_mode == 3 || o.ml_mode == 4) {
        uint32_t max_reads_len = 0;
        for (size_t i = 0; i < nr; i++) max_reads_len = std::max(max_reads_len, rs.lens[i]);
        bk::MultiAssign ma;
        for (size_t i = 0; i < nr; i++) {
            const uint32_t c = eff_count(i);
            for (uint32_t k = 0; k < c; k++) {
                const bk_loci_trims t = with_trims ? trims_of(l_offs[i] + k) : bk_loci_trims{};
                ma.add((uint32_t)i + 1, loci[l_offs[i] + k], c > 1, t.left, t.right, (uint32_t)(l_offs[i] + k));
            }
        }
        diag("Assigning %llu reads which aligned to multiple loci to a single loci", (unsigned long long)n_multi);
        bk::MultiAssignStats st = ma.assign(o.ml_mode == 3, o.nthreads, max_reads_len);
        for (const bk::MultiHitRec &m : ma.recs)
            if (m.multi && m.assigned) {
                take(hits[m.read_id - 1], m.loci);
                if (with_trims) rec_trims[m.read_id - 1] = trims_of(m.src);
            }
        diag("Clustering completed, removed %d unclustered orphans from %d putative resulting in %d (%d clustered near unique, %d clustered near other multiloci reads) multihit reads accepted as assigned",
             st.putative - st.assigned, st.putative, st.assigned, st.near_unique, st.near_multi);
    } else if (o.ml_mode == 5) {
        // eMLall: every locus becomes a record of its own, ReadID = order of creation (CAligner::WriteHitLoci / AddMultiHit,
        // Aligner.cpp:6666-6800); with -M6 reads without alignment (eHRnone, eHRHitInsts) are kept as one unaligned
        // record, everything else (EN, MMDelta) drops out (:9311-9352,9441-9449)
        std::vector<bk_hit> recs;
        std::vector<bk_loci_trims> rt;
        for (size_t i = 0; i < nr; i++) {
            const bk_hit &h = hits[i];
            const uint32_t c = eff_count(i);
            if (c) {
                // loci on sequences the -Z / -z filters reject never become records (CAligner::WriteHitLoci, Aligner.cpp:6739-6760); a read
                // that loses all of them is kept as one record without a hit in '-M6' only
                // The reference compacts the accepted loci in place with `if(pAcceptHit != pHit) *pAcceptHit++ = *pHit;` (:6748-6752): the
                // write position only moves when it differs from the read position, so an accepted locus at the front is overwritten by the
                // next accepted one and the LAST one kept comes out twice.  Reproduced as it stands.
                uint32_t kept = c;
                std::vector<uint32_t> pick(c);
                for (uint32_t k = 0; k < c; k++) pick[k] = k;
                if (chrom_ok) {
                    uint32_t acc = 0;
                    kept = 0;
                    for (uint32_t k = 0; k < c; k++) {
                        if (!(*chrom_ok)[loci[l_offs[i] + pick[k]].chrom_id]) continue;
                        kept++;
                        if (acc != k) pick[acc++] = pick[k];
                    }
                }
                for (uint32_t q = 0; q < kept; q++) {
                    const uint32_t k = pick[q];
                    bk_hit r = h;
                    take(r, loci[l_offs[i] + k]);
                    recs.push_back(r);
                    src.push_back((uint32_t)i);
                    if (with_trims) rt.push_back(trims_of(l_offs[i] + k));
                }
                if (!kept && o.fmt == 6) {
                    // (the record the reference keeps of such a read comes out of its FiltByChroms pass as "aligned to filtered target
                    // sequence": observed on the reference's own output, tests/golden/multi/r5R5ZmB.m6.sam.gz)
                    bk_hit r = h;
                    r.nar = 11;
                    r.num_hits = 0;
                    r.low_hit_instances = 0;
                    recs.push_back(r);
                    src.push_back((uint32_t)i);
                    if (with_trims) rt.push_back(bk_loci_trims{});
                }
            } else if (o.fmt == 6 && h.nar != BK_NAR_NS && (h.rslt == BK_HR_NONE || h.rslt == BK_HR_HITINSTS)) {
                bk_hit r = h;
                r.num_hits = 0;
                r.low_mm = 0;
                recs.push_back(r);
                src.push_back((uint32_t)i);
                if (with_trims) rt.push_back(bk_loci_trims{});
            }
        }
        if (with_trims) rec_trims.swap(rt);
        diag("Treating accepted %llu multialigned reads as uniquely aligned %llu source reads in subsequent processing",
             (unsigned long long)n_multi, (unsigned long long)(n_loci - n_uniq));
        hits.swap(recs);
    }
}

time_t g_t0 = 0;
// The last line of the log, then the process ends at once: every output file is closed and synced by now, and what the destructors of a
// large run would do - hand 20 GB of read store, records and page-locked buffers back page by page, take the HIP runtime down - the
// exit does wholesale (0.9 s of a 5.5 s run went there).
[[noreturn]] void end_process(int rc)
{
    diag("Exit code: %d Total processing time: %ld seconds", rc, (long)(time(nullptr) - g_t0));
    if (bk::env::timing()) {                     // what the exit has to give back
        if (FILE *f = fopen("/proc/self/smaps_rollup", "r")) {
            char line[256];
            while (fgets(line, sizeof line, f))
                if (!strncmp(line, "Rss:", 4) || !strncmp(line, "Anonymous:", 10) || !strncmp(line, "AnonHugePages:", 14) || !strncmp(line, "Shared_", 7) || !strncmp(line, "Private_", 8) || !strncmp(line, "ShmemPmdMapped:", 15))
                    fprintf(stderr, "bk timing: host: at exit %s", line);
            fclose(f);
        }
    }
    fflush(nullptr);
    _exit(rc);
}

// The contexts of a run, one per device: destroyed here and nowhere else (a large run ends in end_process() without coming by).
struct Contexts {
    std::vector<bk_ctx *> v;
    ~Contexts()
    {
        if (v.empty()) return;
        HostClock clk;
        for (bk_ctx *c : v) bk_ctx_destroy(c);
        clk.lap("contexts destroyed");
    }
};

// One `align` run, from its options to its files.  The members stand in the order the run makes them and go in the reverse one:
//  - the contexts outlive everything that works on a device: the head start's worker thread (joined by PrepGuard, or by the releaser
//    thread that Submission and Unlock join) reads its context until it ends
//  - Unlock is declared after the read store and A: runs before either goes - the releaser thread may still be giving the read store's
//    bases back
//  - PrepGuard goes before Unlock and Submission: it waits until the releaser has looked at the head start, then gives it back
struct AlignRun {
    // the options, and what follows from them and the input files' sizes before anything is loaded
    Args a;
    AlignOpts o;
    DeviceContam contam;                           // -H: the loaders' matcher, on the first device
    ContamTrimming contam_trims;
    ContamTrimming *ct = nullptr;                  // (null without -H)
    uint64_t est_reads = 0, plain_bytes = 0;
    bool all_plain = true, long_run = false;
    std::string opath;                             // -o
    bool sam_plain = false, pre_early = false;     // SAM text into a regular file / whose pages are made from the start of the run on
    uint32_t ctx_flags = 0;                        // bk_image_policy and its overrides
    std::string wa;                                // --window-array as given
    bool wa_off = false, want_array = false;
    // the contexts, one per device, and the threads that load their index images
    size_t ndev = 1;
    Contexts ctxs;
    bk_ctx *ctx = nullptr;                         // the first device's
    std::vector<int> ctx_rc;
    std::vector<std::thread> loaders;
    int load_rc = 0;                               // what the read loader returned while they ran
    // -5: the constraints on the first device (declared behind the contexts: goes before them)
    struct ConstraintSet { bk_constraints *p = nullptr; ~ConstraintSet() { bk_constraints_destroy(p); } } constraints;
    std::vector<uint8_t> constrained;              // by chrom_id: the sequence carries a constraint
    // the index's entries
    std::string species;
    uint32_t n_ent = 0;
    std::vector<bk_entry_info> ents;
    Submission S;
    SamPrealloc pre;
    ReadStore rs;
    AlignedSet A;
    struct Unlock { Submission &S; ~Unlock() { if (S.releaser.joinable()) S.releaser.join(); S.release_results(); } } unlock_results{S};
    // the SAM formatter's head start on the device
    bk_sam_prep *sam_prep = nullptr;
    bk_sam_job pk_job{};
    struct PrepGuard { bk_sam_prep *&p; Submission &S; ~PrepGuard() { if (p) { S.done_with_head_start(); bk_sam_prep_free(p); p = nullptr; } } } prep_guard{sam_prep, S};      // (not consumed: given back)
    bool bases_dropped = false;
    // the records, and what the steps behind the alignment make of them
    bk::RecordSet rec{A.hits, A.seg2, {}, {}, {}};
    std::vector<int> multi_dist;
    std::vector<uint8_t> chrom_ok;                 // -Z / -z: AcceptThisChromID by chrom_id (empty: no expressions)
    uint64_t nar[20] = {0};                        // ReportAlignStats: records per NAR
    std::vector<uint32_t> order;                   // SortReadHits(eRSMHitMatch): index in load (ReadID) order -> reference order
    bk::SitePrefs site_prefs;                      // -8
    bool with_site_prefs = false;

    std::vector<const char *> entry_names() const { std::vector<const char *> n; for (const bk_entry_info &e : ents) n.push_back(e.name); return n; }
};

// Every stage below: 0, or 1 after its error message has been logged.

int parse_align_args(int argc, char **argv, int first, Args &a)
{
    std::string err;
    std::map<std::string, std::string> ln = {
        {"mode", "m"}, {"alignstrand", "Q"}, {"editdelta", "e"}, {"substitutions", "s"}, {"maxns", "n"}, {"trim5", "y"},
        {"trim3", "Y"}, {"minacceptreadlen", "l"}, {"maxacceptreadlen", "L"}, {"format", "M"}, {"in", "i"}, {"sfx", "I"},
        {"out", "o"}, {"stats", "O"}, {"threads", "T"}, {"log", "F"}, {"FileLogLevel", "f"}, {"pemode", "U"}, {"mlmode", "r"},
        {"quality", "g"}, {"device", "device"}, {"devices", "devices"}, {"window-array", "window-array"}, {"index-image", "index-image"}, {"rptsamseqsthres", "4"}, {"pair", "u"}, {"pairminlen", "d"}, {"pairmaxlen", "D"},
        {"pairstrand", "E"}, {"nonealign", "j"}, {"multialign", "J"}, {"title", "t"}, {"maxmulti", "R"}, {"clampmaxmulti", "X"},
        {"bestmatches", "N"}, {"microindellen", "a"}, {"minflankexacts", "x"}, {"splicejunctlen", "A"}, {"minchimeric", "c"}, {"pcrwin", "k"}, {"samplenthrawread", "#"}, {"chromexclude", "Z"}, {"chromeinclude", "z"},
        {"contaminants", "H"}, {"minsnpreads", "p"}, {"qvalue", "P"}, {"snpnonrefpcnt", "1"}, {"snpfile", "S"}, {"markerlen", "K"}, {"markerpolythres", "G"}, {"snpcentroid", "7"},
        {"siteprefs", "8"}, {"siteprefsofs", "9"}, {"pcrprimersubs", "6"}, {"lociconstraints", "5"}, {"sam-tags", "sam-tags"}, {"coverage", "coverage"}, {"mark-duplicates", "mark-duplicates"},
        {"junctions", "junctions"}, {"splice-strand", "splice-strand"}};
    if (!parse_args(argc, argv, first, ln, "mQesnyYlLMiIoOTFfUrg4udDjJtRaxAck#ZzpP1SKG7H8965", "EXN", a, err, {"mark-duplicates", "splice-strand"})) {
        fprintf(stderr, "%s align: %s\n", g_proc.c_str(), err.c_str());
        return 1;
    }
    if (!a.has("i") || !a.has("I") || !a.has("o")) {
        fprintf(stderr, "usage: %s align -i <reads> -I <genome.sfx> -o <out.sam> [-s subs] [-e delta] [-Q strand] [-m mode] [-n maxNs] "
                        "[-l minlen] [-L maxlen] [-M 0|5|6] [-O stats] [--device n | --devices a-b] [--window-array on|off] [--index-image lean|full] [--sam-tags NM,MD] [--coverage depth.bedgraph] [--mark-duplicates] [--junctions sj.tab] [--splice-strand]\n", g_proc.c_str());
        return 1;
    }
    return 0;
}

// -H: the contaminants file is read and its matcher made on the first device before anything else (CAligner::Align loads it in front of
// the index, Aligner.cpp:253-270); the matcher needs no index, so it trims the reads while the index image is still travelling
int make_contam_matcher(AlignRun &r)
{
    if (!r.a.has("H") || r.a.str("H").empty()) return 0;
    const std::string cf = r.a.str("H");
    param_line("Contaminant sequences file: '%s'\n", cf.c_str());
    std::vector<ContamEntry> entries;
    if (load_contaminants(cf, entries)) { diag("Unable to load contaminate sequences file '%s'", cf.c_str()); return 1; }
    if (const int crc = r.contam.create(r.o.devices[0], entries)) { diag("Fatal: unable to set up the contaminant matcher on device %d: %s", r.o.devices[0], bk_strerror(crc)); return 1; }
    r.contam_trims.matcher = &r.contam;
    r.contam_trims.keep = true;
    r.ct = &r.contam_trims;
    return 0;
}

int print_param_lines(const AlignOpts &o)
{
    if (!o.site_prefs_path.empty()) {               // (parameter lines, kanga.cpp:1290-1293)
        param_line("Offset read start sites when processing site octamer preferencing: %d\nAligned read octamer site preferencing into this file: '%s'\n",
                   o.site_prefs_ofs, o.site_prefs_path.c_str());
        OutBuf sp_file;                             // the reference creates the file before it loads anything (an empty one stays when no read is accepted)
        sp_file.open(o.site_prefs_path.c_str());
        if (sp_file.fd < 0) { diag("Fatal: unable to create '%s'", o.site_prefs_path.c_str()); return 1; }
        sp_file.close();
    }
    if (o.primer_subs > 0) param_line("correcting PCR 5' artefacts : %d\n", o.primer_subs);      // (kanga.cpp:1146-1147)
    if (!o.constraints_path.empty()) param_line("Loci base constraints file: '%s'\n", o.constraints_path.c_str());      // (kanga.cpp:1264)
    return 0;
}

// The image pays from BK_POLICY_MIN_READS reads per device on (bk_image_policy).  The decision is made HERE, from the size of
// the input files, before a single read is parsed: the array then comes with the index image (made behind the slices of the suffix
// array's upload) instead of in front of the first batch.  A FASTA record of a 100-base read is about 120 bytes, a FASTQ one about
// 250; gzip'd files hold about four times their size.
void estimate_input(AlignRun &r)
{
    for (const char *opt : {"i", "u"})
        if (r.a.has(opt))
            for (const std::string &fn : r.a.v[opt]) {
                // (gzip'd files too: they are inflated whole like plain ones are mapped, and say - bgzip'd ones exactly - how much text they hold)
                const uint64_t text = bk::text_bytes_estimate(fn);
                if (!text) continue;
                const bool fq = fn.find(".fq") != std::string::npos || fn.find(".fastq") != std::string::npos;
                r.est_reads += text / (fq ? 250 : 120);
                r.plain_bytes += text;
                r.all_plain = r.all_plain && r.o.nthreads > 1;
            }
    r.long_run = r.est_reads / r.ndev >= kLongRunMinReads;
}

void start_early_buffers(AlignRun &r)
{
    const AlignOpts &o = r.o;
    if (r.all_plain && r.plain_bytes >= (256u << 20)) r.S.start_early(r.plain_bytes, (uint32_t)std::max(15, o.min_len));
    // SAM text goes into a file of known approximate size.  A large plain-text input tells that size now (a record is the read's name and
    // bases - and qualities - as the input holds them plus about 31 bytes, 55 for a paired end; a FASTA record of 100 bases is 117 bytes):
    // the file's pages are allocated, zeroed and mapped by background threads from here on - 7 GB for 50 M reads of 100 bases, which the
    // writers would otherwise wait for.  Other inputs: once the reads are loaded (start_sam_file_late).
    r.opath = r.a.str("o");
    struct stat ost;
    const bool out_special = stat(r.opath.c_str(), &ost) == 0 && !S_ISREG(ost.st_mode);      // a FIFO, /dev/fd/N of a process substitution, /dev/null
    r.sam_plain = o.fmt >= 5 && !out_special && !is_bam_name(r.opath) && !is_gz_name(r.opath);
    r.pre_early = r.sam_plain && r.all_plain && r.plain_bytes >= bk::env::sam_early_min(256ULL << 20);      // (tests lower the input size from which the file is started early)
    const uint64_t pre_early_est = (1u << 20) + r.plain_bytes + r.plain_bytes / (o.pe_mode ? 2 : 3) + o.sam_tag_bytes() * r.est_reads;
    if (r.pre_early) r.pre.start(r.opath.c_str(), pre_early_est, 2);
}

// bk_image_policy, from the reads a device is going to align; --window-array on | off and --index-image lean | full override its two halves
void choose_index_image(AlignRun &r)
{
    r.ctx_flags = bk_image_policy(r.est_reads / r.ndev);
    r.wa = r.a.has("window-array") ? r.a.str("window-array") : std::string();
    r.wa_off = r.wa == "off" || r.wa == "0" || r.wa == "no";
    if (r.wa_off) r.ctx_flags &= ~BK_CTX_WINDOW_ARRAY_EAGER;
    else if (!r.wa.empty()) r.ctx_flags |= BK_CTX_WINDOW_ARRAY_EAGER;
    r.want_array = (r.ctx_flags & BK_CTX_WINDOW_ARRAY_EAGER) != 0;
    const std::string img = r.a.has("index-image") ? r.a.str("index-image") : std::string();
    if (img == "full") r.ctx_flags &= ~(BK_CTX_GROW_IMAGE | BK_CTX_LEAN_IMAGE);
    else if (img == "lean") r.ctx_flags = (r.ctx_flags & ~BK_CTX_GROW_IMAGE) | BK_CTX_LEAN_IMAGE;
}

int load_all_reads(AlignRun &r, int nthreads, ReadStore &into)
{
    const AlignOpts &o = r.o;
    return o.pe_mode ? load_reads_pe(r.a.v["i"], r.a.v["u"], o.trim5, o.trim3, o.min_len, o.max_len, nthreads, into, r.ct)
                     : load_reads(r.a.v["i"], o.trim5, o.trim3, o.min_len, o.max_len, nthreads, into, r.ct);
}

// index images travel to the devices (one loader thread each) while this thread parses the reads: the two longest serial steps
// of a run overlap (the reference loads its reads in the background of the alignment instead, Aligner.cpp:4820-4860).
// The loader threads run from here until pack_reads_and_join_index() has joined them: nothing returns early in between, which is
// why this stage keeps its result in load_rc.
void load_reads_behind_index(AlignRun &r)
{
    // the first device reads the .sfx and builds the tables; the others receive the finished image device to device (xGMI)
    r.ctxs.v.assign(r.ndev, nullptr);
    r.ctx_rc.assign(r.ndev, 0);
    r.loaders.emplace_back([&r]() {
        r.ctx_rc[0] = bk_ctx_create_ex(&r.ctxs.v[0], r.a.str("I").c_str(), r.o.devices[0], &r.o.P, r.ctx_flags);
        if (r.ctx_rc[0] || r.ndev == 1) return;
        std::vector<std::thread> cloners;
        for (size_t d = 1; d < r.ndev; d++) cloners.emplace_back([&r, d]() { r.ctx_rc[d] = bk_ctx_clone(&r.ctxs.v[d], r.ctxs.v[0], r.o.devices[d]); });
        for (auto &t : cloners) t.join();
    });
    // (the index loader's threads - the HIP runtime coming up, four feeding the upload - the page-locking of the packed reads' buffers and
    // the output file's pages run meanwhile: the parser leaves them their share of the cores, or a CPU quota stalls all of them in turn)
    const int parse_threads = std::max(std::min(r.o.nthreads, 4), r.o.nthreads - 6);
    r.load_rc = load_all_reads(r, parse_threads, r.rs);
    r.contam.destroy();                             // (its staging and device buffers have served)
}

// .. and, still behind the index load: the reads packed for the boundary, the result array page-locked
int pack_reads_and_join_index(AlignRun &r)
{
    int rc = r.load_rc;
    if (!rc && r.rs.size()) rc = prepare_submission(r.o, r.rs, r.ndev, r.long_run, r.A, r.S);
    if (!rc && r.pre_early) r.pre.add_threads(2);   // (two while the parser's threads allocate their own memory, four from here on)
    { HostClock jc; for (auto &t : r.loaders) t.join(); jc.lap("waited for the index image"); }
    for (size_t d = 0; d < r.ndev; d++)
        if (r.ctx_rc[d]) { diag("Fatal: unable to load genome assembly suffix array: %s", bk_strerror(r.ctx_rc[d])); return 1; }
    if (rc) return 1;
    r.ctx = r.ctxs.v[0];
    r.species = bk_dataset_name(r.ctx);
    r.n_ent = bk_num_entries(r.ctx);
    r.ents.resize(r.n_ent);
    for (uint32_t i = 0; i < r.n_ent; i++) bk_get_entry(r.ctx, i, &r.ents[i]);
    diag("Genome Assembly Name: '%s'", r.species.c_str());
    diag("Genome assembly suffix array loaded");
    return 0;
}

// -5: the constraints are read as soon as the index's sequences are known (CAligner::Align, Aligner.cpp:328-337) and travel to the
// first device, which checks the records against them behind the alignment (apply_loci_constraints)
int load_constraints(AlignRun &r)
{
    const std::string &path = r.o.constraints_path;
    diag("Loading loci base constraints from CSV file '%s' ...", path.c_str());
    std::vector<bk_constraint> cons;
    size_t n_chroms = 0;
    std::string err;
    if (bk::load_loci_constraints(path, r.ents, cons, n_chroms, err)) {
        diag("%s", err.c_str());
        diag("Unable to load loci constraints");
        return 1;
    }
    const int rc = bk_constraints_create(r.ctx, cons.data(), (uint32_t)cons.size(), &r.constraints.p);
    if (rc) { diag("Fatal: unable to set up the loci base constraints on device %d: %s", r.o.devices[0], bk_strerror(rc)); return 1; }
    r.constrained = bk::constrained_chroms(cons);
    diag("Completed loading %d loci base constraints for %d target sequences from CSV file '%s'", (int)cons.size(), (int)n_chroms, path.c_str());
    return 0;
}

void tune_and_describe_image(AlignRun &r)
{
    // (the other devices' contexts, copies of the first's image, make their window arrays when their first batch arrives)
    // (--window-array on asks for it whatever the index: one of 5-byte elements gets it only so - "use_swin" 2 -, the policy's own
    // choice leaves it without: making it goes over a 17 Gbp index twice)
    for (bk_ctx *c : r.ctxs.v) (void)bk_ctx_tune(c, "use_swin", r.want_array ? ((!r.wa.empty() && !r.wa_off) ? 2 : 1) : 0);
    diag("Index image: %s, suffix-ordered window array %s (%zu reads per device, %llu estimated from the input files' sizes; every table comes with the index from %llu reads per device on; --index-image lean | full and --window-array on | off override)",
         (r.ctx_flags & BK_CTX_LEAN_IMAGE) ? "lean" : ((r.ctx_flags & BK_CTX_GROW_IMAGE) ? "lean, grows on a long run" : "every table"),
         !r.want_array ? "off" : ((bk_sfx_el_size(r.ctx) == 5 && (r.wa.empty() || r.wa_off)) ? "off (an index of 5-byte elements gets it with --window-array on only)" : "on"), r.rs.size() / r.ctxs.v.size(),
         (unsigned long long)(r.est_reads / r.ndev), (unsigned long long)BK_POLICY_MIN_READS);
}

// (the SAM file of any other large run is started now: name + bases (+ qualities) + about 31 bytes per record, 55 for a paired end)
void start_sam_file_late(AlignRun &r)
{
    const size_t nr = r.rs.size();
    if (!r.sam_plain || r.pre.fd >= 0) return;
    if (nr < (size_t)bk::env::sam_device_min(200000ULL)) return;                // (tests lower the size from which the large-run machinery is used)
    uint64_t est = (1u << 20) + r.rs.name_bytes() + 40ULL * nr + (r.o.pe_mode ? 24ULL * nr : 0) + (uint64_t)r.n_ent * 128;
    est += (uint64_t)(g_qual_mode != 3 ? 2 : 1) * r.rs.base_bytes() + r.o.sam_tag_bytes() * nr;
    r.pre.start(r.opath.c_str(), est);
}

// -Z / -z by CAligner::AcceptThisChromID (chrom_accept_table: exclusion first, not the rule of FiltByChroms further down)
int make_accept_table(AlignRun &r)
{
    if (r.o.re_excl.empty() && r.o.re_incl.empty()) return 0;
    const std::vector<uint8_t> ok = bk::chrom_accept_table(r.entry_names(), r.o.re_excl, r.o.re_incl);
    r.chrom_ok.assign(1, 1);                        // (indexed by chrom_id, which counts from 1)
    r.chrom_ok.insert(r.chrom_ok.end(), ok.begin(), ok.end());
    // the paired-end rules consult the filters while they pair (AcceptProvPE, the orphan recovery's anchors, the single-end acceptance)
    if (r.o.pe_mode)
        for (bk_ctx *c : r.ctxs.v)
            if (const int rc = bk_ctx_set_chrom_filter(c, r.chrom_ok.data(), (uint32_t)r.chrom_ok.size())) { diag("Error: chromosome filter table: %s", bk_strerror(rc)); return 1; }
    return 0;
}

int run_alignment(AlignRun &r)
{
    const size_t nr = r.rs.size();
    // the pipelines' device buffers and the contexts' batch scratch are in place before the clock of T_align starts (the reference sizes its
    // per-thread scratch before its workers start, Aligner.cpp:8771-8790)
    std::vector<bk_stream *> streams;
    if (nr && open_pipelines(r.ctxs.v, r.o, r.S, streams)) return 1;
    diag("Now aligning with minimum core size of %dbp...\n", bk_min_core_len(r.ctx));
    if (r.o.pe_mode) diag("Paired end association and partner alignment processing runs with the alignment of each batch");
    if (nr && align_reads(r.ctxs.v, streams, r.o, r.rs, r.S, r.A)) return 1;
    if (!nr) r.A.seq_counts.assign(r.n_ent, 0);
    diag("Alignment of %zu from %zu loaded completed", nr, nr);
    return 0;
}

// the SAM records of a large run are formatted by the device (report.cpp): what it needs of the reads travels there while the
// host resolves, filters and sorts.  The head start is given the READS, in every mode: -r5's records are made later and come with
// the job of bk_sam_format, which names the read of each (bk_sam_job.src, n_src_reads = the reads handed over here)
void start_sam_head(AlignRun &r)
{
    const AlignOpts &o = r.o;
    const Args &a = r.a;
    ReadStore &rs = r.rs;
    Submission &S = r.S;
    const size_t nr = rs.size();
    // (-6 overwrites bases of the read store further down: no head start then - the formatter uploads the byte form, corrected, when
    // the records are written, and the bases are never dropped: may_drop_bases needs the head start)
    // (-5 changes NARs, not bases: the head start goes ahead, as it does with -k)
    if (r.pre.fd >= 0 && r.rec.size() == rs.lens.size() && o.primer_subs == 0) {
        bk_sam_job hj{};
        hj.bases = rs.bases.data(); hj.n_bases = rs.bases.size(); hj.offs = rs.offs.data(); hj.lens = rs.lens.data();
        hj.names = rs.names.data(); hj.n_name_bytes = rs.names.size(); hj.name_ofs = rs.name_ofs.data(); hj.n_reads = nr;
        // without scores in the read store (FASTA, or -g3) the formatter reads the packed form the alignment was fed from: page-locked,
        // a quarter of the bytes, no host thread copies anything
        if (g_qual_mode == 3 && S.words != nullptr && S.lens16 != nullptr) {
            hj.pk_words = S.words; hj.n_pk_words = S.n_words; hj.pk_lens16 = S.lens16; hj.pk_exc = S.exc_job.data(); hj.n_pk_exc = S.exc_job.size();
            hj.bases = nullptr; hj.n_bases = 0; hj.offs = nullptr; hj.lens = nullptr;
        }
        r.pk_job = hj;
        const uint64_t per_rec = (rs.name_bytes() + (uint64_t)(g_qual_mode != 3 ? 2 : 1) * rs.base_bytes()) / std::max<size_t>(nr, 1) + 64 + (o.pe_mode ? 24 : 0) + o.sam_tag_bytes();
        if (bk_sam_prepare(r.ctx, &hj, (uint32_t)std::min<uint64_t>(per_rec + per_rec / 8, 1u << 20), &r.sam_prep) != BK_OK) { r.sam_prep = nullptr; r.pk_job = bk_sam_job{}; }
    }
    // The read store's bases - 5 GB of a 50 M-read run, a third of a second to hand back at the exit - have served too once the device
    // holds the packed reads, unless an output of this run still reads them (-j / -J, -O, SNP calling); should the device decline
    // after all, the host formatter loads them again (restore_reads)
    // (.. and only when every read file can be read a second time - a FIFO or a process substitution cannot: should the device decline
    // the SAM records, the host formatter reloads the reads)
    bool inputs_regular = true;
    for (const char *opt : {"i", "u"})
        if (a.has(opt))
            for (const std::string &fn : a.v.at(opt)) { struct stat ist; inputs_regular = inputs_regular && stat(fn.c_str(), &ist) == 0 && S_ISREG(ist.st_mode); }
    // (.. and not in the modes whose later steps read the bases on the host: the flank trimmer of -x / -A, the .jct / .ind files of -A / -a,
    // -c's and -r5's records, the constraint pass of -5, which gathers the bases of the reads over a constraint - there the read store stays whole)
    const bool host_reads_bases = o.ml_mode == 5 || o.micro_indel || o.splice_len || o.min_chim || o.min_flank || !o.constraints_path.empty();
    const bool may_drop_bases = inputs_regular && !host_reads_bases && r.pk_job.pk_words != nullptr && r.sam_prep != nullptr && !a.has("j") && !a.has("J") && !a.has("O") && o.snp.min_reads <= 0;
    if (nr)
        S.release_packed_in_background(r.pk_job.pk_words != nullptr ? r.sam_prep : nullptr,
                                       may_drop_bases ? std::function<void()>([&r]() { bk::RawVec<uint8_t> none; r.rs.bases.swap(none); r.bases_dropped = true; })
                                                      : std::function<void()>());
}

// the read store's bases back, should start_sam_head() have dropped them and the device decline the SAM records after all
int restore_reads(AlignRun &r)
{
    ReadStore &rs = r.rs;
    if (r.S.releaser.joinable()) r.S.releaser.join();
    if (!r.bases_dropped) return 0;
    diag("The device declined the SAM records: loading the reads again for the host's formatter");
    ReadStore again;
    // (-H: the cuts the first load found are used again, nothing is matched a second time)
    r.contam_trims.matcher = nullptr;
    r.contam_trims.replay_at = 0;
    const int rl = load_all_reads(r, r.o.nthreads, again);
    if (rl || again.size() != rs.size()) return 1;
    rs.bases.swap(again.bases); rs.offs.swap(again.offs); rs.used_bases = again.used_bases;
    r.bases_dropped = false;
    return 0;
}

void resolve_multi_and_count_pairs(AlignRun &r)
{
    const AlignOpts &o = r.o;
    r.multi_dist.assign((size_t)o.max_ml, 0);
    if (o.ml_mode) resolve_multi_loci(o, r.rs, r.A, r.rec, r.multi_dist, r.chrom_ok.empty() ? nullptr : &r.chrom_ok);
    if (o.pe_mode) {
        // CAligner::ProcessPairedEnds ran on the device with each batch (reads are held interleaved PE1,PE2, Aligner.cpp:11349-11355)
        const std::vector<bk_hit> &hits = r.rec.hits;
        const size_t nr = r.rec.size();
        size_t n_pe = 0;
        for (size_t i = 0; i < nr; i += 2) n_pe += (hits[i].flags & 0x80) && (hits[i + 1].flags & 0x80);
        diag("From %zu paired reads there were %zu accepted as paired", nr / 2, n_pe);
    }
}

// -c: chimeric placements keep the trims AdaptiveTrim found (ProcCoredApprox :9292-9299); the flank trimmer leaves them alone (:1641)
void keep_chimeric_trims(bk::RecordSet &rec)
{
    rec.ensure_trims();
    size_t n_ch = 0;
    for (size_t i = 0; i < rec.size(); i++)
        if (rec.hits[i].nar == BK_NAR_ACCEPTED && rec.is_chimeric(i)) {
            rec.trims.left[i] = rec.rec_trims.empty() ? rec.seg2[rec.RD(i)].match_len : rec.rec_trims[i].left;
            rec.trims.right[i] = rec.rec_trims.empty() ? rec.seg2[rec.RD(i)].read_ofs : rec.rec_trims[i].right;
            n_ch++;
        }
    diag("Of the accepted aligned reads, %zu were chimeric", n_ch);
}

// -5: CAligner::IdentifyConstraintViolations, behind the paired-end association and the multi-loci assignment, before -k, -6 and -x
// (Aligner.cpp:594).  Every accepted record on a constrained sequence goes to the first device with its adjusted loci (both segments
// of a two-segment read; -c's trims are in place by now, as they are in the reference's records from the alignment on); the device
// looks at the bases of those that lie over a constraint.  A violated record becomes eNARLociConstrained, with -U its mate too
int apply_loci_constraints(AlignRun &r)
{
    const AlignOpts &o = r.o;
    const ReadStore &rs = r.rs;
    bk::RecordSet &rec = r.rec;
    std::vector<bk_hit> &hits = rec.hits;
    const char *kind = o.pe_mode ? "PE" : "SE";
    diag("Identifying %s loci base constraint violations ...", kind);
    HostClock clk;
    bk::RawVec<bk_constraint_req> reqs;
    bk::RawVec<uint32_t> rec_of;
    par_select(rec.size(), o.nthreads, [&](size_t i) { return bk::constraint_selects(hits[i], r.constrained); },
               [&](size_t at, size_t i) {
                   const size_t rd = rec.RD(i);
                   reqs[at] = bk::constraint_request(hits[i], rec.a_start(hits[i], i), rec.a_len(hits[i], i), rec.TL(i), rec.has_seg2(i) ? &rec.seg2[rd] : nullptr, rs.offs[rd], rs.lens[rd]);
                   rec_of[at] = (uint32_t)i;
               },
               [&](size_t n) { reqs.resize(n); rec_of.resize(n); });
    bk::RawVec<uint8_t> status(reqs.size());
    clk.lap("constraint requests made");
    uint64_t counts[4];
    const int rc = bk_constraints_check(r.constraints.p, reqs.data(), reqs.size(), rs.bases.data(), rs.bases.size(), status.data(), counts);
    if (rc) { diag("Fatal: the loci base constraint check failed: %s", bk_strerror(rc)); return 1; }
    clk.lap("constraints checked (device)");
    size_t n_marked = 0;
    for (size_t k = 0; k < reqs.size(); k++) {
        const int m = bk::constraint_apply(status[k], hits[rec_of[k]]);
        if (m < 0) { diag("Fatal: the loci base constraint check turned a request down"); return 1; }
        n_marked += (size_t)m;
    }
    if (o.pe_mode) n_marked += bk::constraint_mark_mates(hits);
    clk.lap("constraint violations marked");
    diag("Identified %d %s loci base constraint violations", (int)n_marked, kind);
    return 0;
}

// CAligner::SortHitMatch (Aligner.cpp:10069-10114), ties left to the replica of the reference's sort.  The comparator's fields are
// packed into three words per record first (NAR | NumHits class: 1 before the others | NumHits | ChromID, then AdjStartLoci |
// AdjHitLen, then Strand | LowMMCnt; records whose NumHits is not 1 compare equal beyond NumHits, so their other fields stay 0): the
// quicksort then walks keys lying next to each other instead of chasing record indexes through the result array - same
// comparisons, same outcome, same order
struct SortRec { uint64_t hi, lo; uint32_t tail, idx; };
void sorted_order(const bk::RecordSet &rec, int nthreads, std::vector<uint32_t> &ord)
{
    const size_t nr = rec.size();
    auto sort_cmp = [](const SortRec &x, const SortRec &y) -> int {
        if (x.hi != y.hi) return x.hi < y.hi ? -1 : 1;
        if (x.lo != y.lo) return x.lo < y.lo ? -1 : 1;
        if (x.tail != y.tail) return x.tail < y.tail ? -1 : 1;
        return 0;
    };
    bk::RawVec<SortRec> recs(nr);
    auto fill = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            const bk_hit &p = rec.hits[i];
            SortRec &r = recs[i];
            r.idx = (uint32_t)i;
            if (p.num_hits == 1) {
                r.hi = ((uint64_t)p.nar << 41) | (uint64_t)p.chrom_id;
                r.lo = ((uint64_t)rec.a_start(p, i) << 32) | (uint64_t)rec.a_len(p, i);
                r.tail = ((uint32_t)p.strand << 8) | (uint32_t)(uint8_t)(p.low_mm + 128);
            } else {
                r.hi = ((uint64_t)p.nar << 41) | (1ULL << 40) | ((uint64_t)p.num_hits << 32);
                r.lo = 0;
                r.tail = 0;
            }
        }
    };
    HostClock clk;
    par_ranges(nr, nthreads, [&](size_t lo, size_t hi, int) { fill(lo, hi); });
    clk.lap("sort records filled");
    bk::ref_order_sort(recs.data(), (int64_t)nr, sort_cmp, nthreads);
    clk.lap("sorted (the reference's order of equal records)");
    ord.resize(nr);
    par_ranges(nr, nthreads, [&](size_t lo, size_t hi, int) { for (size_t i = lo; i < hi; i++) ord[i] = recs[i].idx; });
    clk.lap("order taken");
}

// -k: CAligner::ReducePCRduplicates runs on the sorted set, before the flank trimmer (Aligner.cpp:598-610)
void reduce_pcr_artefacts(AlignRun &r)
{
    bk::RecordSet &rec = r.rec;
    diag("Processing to reduce PCR differential amplification artefacts processing started..");
    std::vector<uint32_t> ord;
    sorted_order(rec, r.o.nthreads, ord);
    const size_t n_dup = bk::reduce_pcr_duplicates(rec.hits, ord, [&](size_t i) { return rec.a_start(rec.hits[i], i); }, [&](size_t i) { return rec.a_len(rec.hits[i], i); }, r.o.pcr_win);
    diag("Removed %zu potential PCR artefact reads", n_dup);
}

// -6: CAligner::PCR5PrimerCorrect(m_MaxSubs), between -k and the flank trimmer (Aligner.cpp:608-617): the reads still above the user's
// rate go to the first device with their first twelve bases; its answers patch the read store and the records (primer_correct.h).
// The reference sorts behind the pass since LowMMCnt is a sort key: every sorted_order() after it is made from the records as they stand
int correct_primer_artefacts(AlignRun &r)
{
    const AlignOpts &o = r.o;
    ReadStore &rs = r.rs;
    bk::RecordSet &rec = r.rec;
    std::vector<bk_hit> &hits = rec.hits;
    diag("PCR 5' Primer correction processing started..");
    diag("Starting PCR 5' %dbp primer correction processing targeting substitution rate of %d ...", BK_PRIMER_KLEN, o.user_subs);
    HostClock clk;
    bk::RawVec<bk_primer_req> reqs;
    bk::RawVec<uint32_t> rec_of;
    par_select(rec.size(), o.nthreads, [&](size_t i) { return bk::primer_selects(hits[i], rec.has_seg2(i), rs.lens[rec.RD(i)], o.user_subs); },
               [&](size_t at, size_t i) {
                   reqs[at] = bk::primer_request(hits[i], rs.bases.data() + rs.offs[rec.RD(i)], rs.lens[rec.RD(i)], o.user_subs);
                   rec_of[at] = (uint32_t)i;
               },
               [&](size_t n) { reqs.resize(n); rec_of.resize(n); });
    bk::RawVec<bk_primer_res> res(reqs.size());
    clk.lap("primer correction requests made");
    const int prc = bk_primer_correct(r.ctx, reqs.data(), reqs.size(), res.data());
    if (prc) { diag("Fatal: the 5' primer correction failed: %s", bk_strerror(prc)); return 1; }
    clk.lap("primer windows compared (device)");
    // (the pass writes Seg[0].Mismatches, not TrimMismatches - which the CSV writers and the -O statistics print, and which only the
    // flank trimmer computes again, for the reads it trims, :1788: the counts as they stood before the pass are kept as the trims')
    rec.ensure_trims();
    bk::PrimerStats pst;
    for (size_t k = 0; k < reqs.size(); k++) {
        const size_t i = rec_of[k];
        if (bk::primer_apply(res[k], hits[i], rs.bases.data() + rs.offs[rec.RD(i)], pst)) { diag("Fatal: the 5' primer correction turned a request down"); return 1; }
    }
    clk.lap("primer corrections applied");
    diag("Completed PCR 5' primer correction, %llu reads with %llu bases corrected, %llu reads with excessive substitutions rejected",
         (unsigned long long)pst.reads, (unsigned long long)pst.bases, (unsigned long long)pst.rejected);
    diag("PCR 5' Primer correction processing completed");
    return 0;
}

// -x (and forced by -A): CAligner::AutoTrimFlanks
int trim_flanks(AlignRun &r)
{
    const ReadStore &rs = r.rs;
    bk::RecordSet &rec = r.rec;
    diag("Starting 5' and 3' flank sequence autotrim processing...");
    bk::SfxFile sft;
    std::string serr;
    if (bk::sfx_open(r.a.str("I").c_str(), sft, &serr) != 0) { diag("Fatal: %s", serr.c_str()); return 1; }
    bk::auto_trim_flanks(rec.hits, [&](size_t i) { return rec.has_seg2(i) || rec.is_chimeric(i); }, [&](size_t i) { return rs.bases.data() + rs.offs[rec.RD(i)]; },
                         [&](size_t i) -> const uint8_t * {
                             const bk_hit &h = rec.hits[i];
                             return (h.chrom_id >= 1 && h.chrom_id <= r.n_ent) ? sft.seq + r.ents[h.chrom_id - 1].start_ofs + h.match_loci : nullptr;
                         },
                         r.o.min_flank, r.o.pe_mode != 0, r.o.nthreads, rec.trims);
    diag("Finished 5' and 3' flank sequence autotriming, %zu plus strand and %zu minus strand aligned reads removed", rec.trims.removed_plus,
         rec.trims.removed_minus);
    return 0;
}

// orphan junction filters, splice junctions first (Aligner.cpp:630-650)
void remove_orphan_junctions(AlignRun &r)
{
    if (r.o.splice_len) {
        diag("Removal of orphan splice junction processing started..");
        auto n = bk::remove_orphan_segs(r.rec.hits, r.rec.seg2, 4, 7);
        diag("From %zu reads with putative splice junctions %zu orphans were removed", n.first, n.second);
    }
    if (r.o.micro_indel) {
        diag("Removal of orphan microInDels processing started..");
        auto n = bk::remove_orphan_segs(r.rec.hits, r.rec.seg2, 1, 8);
        diag("From %zu reads with putative microIndels %zu orphans were removed", n.first, n.second);
    }
}

// -Z / -z by CAligner::FiltByChroms (chrom_keep_table: inclusion first); accepted reads on the other sequences become eNARChromFilt
void filter_by_chroms(AlignRun &r)
{
    diag("Now filtering matches by chromosome");
    const std::vector<uint8_t> keep = bk::chrom_keep_table(r.entry_names(), r.o.re_excl, r.o.re_incl);
    size_t n_filt = 0;
    for (bk_hit &h : r.rec.hits)
        if (h.nar == BK_NAR_ACCEPTED && h.chrom_id >= 1 && h.chrom_id <= r.n_ent && !keep[h.chrom_id - 1]) { h.nar = 11; h.num_hits = 0; h.low_hit_instances = 0; n_filt++; }
    diag("Filtering by chromosome completed - removed %zu  matches", n_filt);
}

// CAligner::ReportAlignStats (Aligner.cpp:3493-3822): strand counts, the simulated-reads truth check, NAR histogram
struct AcceptedCounts { uint64_t acc = 0, plus = 0; size_t first = 0; };      // accepted records, those on '+', the first one in load order

AcceptedCounts count_nars(AlignRun &r)
{
    const std::vector<bk_hit> &hits = r.rec.hits;
    const size_t nr = hits.size();
    const int nt = std::max(1, r.o.nthreads);
    std::vector<std::array<uint64_t, 24>> part((size_t)nt);
    std::vector<size_t> first((size_t)nt, nr);
    for (auto &pt : part) pt.fill(0);
    par_ranges(nr, nt, [&](size_t lo, size_t hi, int t) {
        std::array<uint64_t, 24> c{};
        size_t f = nr;
        for (size_t i = lo; i < hi; i++) {
            const bk_hit &h = hits[i];
            c[h.nar < 20 ? h.nar : 0]++;
            if (h.nar == BK_NAR_ACCEPTED) { c[20]++; c[21] += h.strand == '+'; if (f == nr) f = i; }
        }
        part[(size_t)t] = c; first[(size_t)t] = f;
    });
    AcceptedCounts tot;
    tot.first = nr;
    for (int t = 0; t < nt; t++) {
        for (int k = 0; k < 20; k++) r.nar[k] += part[(size_t)t][(size_t)k];
        tot.acc += part[(size_t)t][20]; tot.plus += part[(size_t)t][21];
        tot.first = std::min(tot.first, first[(size_t)t]);
    }
    return tot;
}

// Reads named by `biokanga simreads` carry where they came from (lcl|usimreads|id|chrom|start|end|len|strand|..): an accepted
// alignment on the named sequence counts as high confidence when one or both of its ends are the named ones, anything
// else as misaligned.  Reads are visited in load order; the first accepted read decides whether the set is simulated, and
// a later accepted read that does not parse ends the check - and drops the line - exactly as the reference's loop does
// (:3560-3650).  The descriptors are parsed with the reference's own sscanf formats.
void check_simulated_reads(AlignRun &r, const AcceptedCounts &tot)
{
    const bk::RecordSet &rec = r.rec;
    uint64_t n2 = 0, n1 = 0, n_mis = 0;
    bool sim = false;
    // (the accepted reads were counted by all threads; the truth check below visits reads only while the set looks simulated)
    for (size_t i = tot.first; i < rec.size(); i++) {
        const bk_hit &h = rec.hits[i];
        if (h.nar != BK_NAR_ACCEPTED) continue;
        if (!(sim || i == tot.first)) break;
        char typ[100], xchrom[300], x1c[100], x2c[100], xstrand;
        int id, xs, xe, xl, xerrs;
        const char *nm = r.rs.name(rec.RD(i));
        if (strlen(nm) > 127) continue;
        int its = sscanf(nm, "%99[^|]|usimreads|%d|%99[^|]|%d|%d|%d|%c|%d", typ, &id, xchrom, &xs, &xe, &xl, &xstrand, &xerrs);
        if (its >= 6) sim = true;
        else {
            its = sscanf(nm, "%99[^|]|usimreads|%d|%99[^|]|%99[^|]|%99[^|]|%d|%d|%d|%c|%d", typ, &id, xchrom, x1c, x2c, &xs, &xe, &xl, &xstrand, &xerrs);
            if (its < 8) sim = false;
            else { strcat(xchrom, "|"); strcat(xchrom, x1c); strcat(xchrom, "|"); strcat(xchrom, x2c); sim = true; }
        }
        if (!sim) continue;
        if (h.chrom_id < 1 || h.chrom_id > r.n_ent || strcasecmp(r.ents[h.chrom_id - 1].name, xchrom)) { n_mis++; continue; }
        const long left = (long)h.match_loci;
        const long right = rec.has_seg2(i) ? (long)rec.seg2[rec.RD(i)].match_loci + rec.seg2[rec.RD(i)].match_len - 1 : left + h.match_len - 1;
        if (left == xs || right == xe) (left != xs || right != xe ? n1 : n2)++;
        else n_mis++;
    }
    diag("From %zu source reads there are %llu accepted alignments, %llu on '+' strand, %llu on '-' strand", r.rs.size(), (unsigned long long)tot.acc,
         (unsigned long long)tot.plus, (unsigned long long)(tot.acc - tot.plus));
    if (sim)
        diag("There are %llu (%llu 2 edge, %llu 1 edge) high confidence aligned simulated reads with %llu misaligned", (unsigned long long)(n2 + n1),
             (unsigned long long)n2, (unsigned long long)n1, (unsigned long long)n_mis);
}

// nothing behind the alignment changed an acceptance: the per-sequence counts the devices kept (summed over them by the exchange
// step) must add up to the accepted reads counted here
int check_seq_counts(AlignRun &r)
{
    const AlignOpts &o = r.o;
    if (o.pe_mode || o.ml_mode || o.micro_indel || o.splice_len || o.min_chim || o.pcr_win >= 0 || o.min_flank || o.primer_subs || !o.constraints_path.empty() || !o.re_excl.empty() || !o.re_incl.empty()) return 0;
    uint64_t tot = 0;
    for (uint64_t c : r.A.seq_counts) tot += c;
    if (tot != r.nar[1]) { diag("Fatal: the devices counted %llu accepted reads, the result records hold %llu", (unsigned long long)tot, (unsigned long long)r.nar[1]); return 1; }
    if (r.ndev > 1) diag("Accepted read counts per sequence reduced over %zu devices: %llu reads", r.ndev, (unsigned long long)tot);
    return 0;
}

int report_align_stats(AlignRun &r)
{
    check_simulated_reads(r, count_nars(r));
    diag("Unable to align %llu source reads of which %llu were not aligned as they contained excessive number of indeterminate 'N' bases",
         (unsigned long long)(r.rec.size() - r.nar[1]), (unsigned long long)r.nar[2]);
    diag("Read nonalignment reason summary:");
    for (int k = 0; k < 20; k++) diag("   %llu (%s) %s", (unsigned long long)r.nar[k], kNarTag[k], kNarDescr[k]);
    return check_seq_counts(r);
}

// -8: CAligner::ProcessSiteProbabilites, called between ReportAlignStats - which leaves the reads sorted - and the writers
// (Aligner.cpp:706), when reads were accepted.  The visited reads' Seg[0] as it stands (MatchLoci / MatchLen, not the flank-trimmed
// start) goes to the first device, which gathers the eight target bases of every start site; the sequential rest is site_prefs.h.
int gather_site_prefs(AlignRun &r)
{
    const bk::RecordSet &rec = r.rec;
    const std::vector<uint32_t> &order = r.order;
    sorted_order(rec, r.o.nthreads, r.order);
    diag("Processing for alignment site probabilities...");
    HostClock clk;
    // (by all threads: a stretch of the sorted order each)
    bk::RawVec<bk_site_req> reqs;
    bk::RawVec<uint32_t> rec_of;
    par_select(order.size(), r.o.nthreads, [&](size_t k) { return rec.hits[order[k]].nar == BK_NAR_ACCEPTED && !rec.has_seg2(order[k]); },
               [&](size_t at, size_t k) {
                   const bk_hit &h = rec.hits[order[k]];
                   reqs[at] = bk_site_req{h.chrom_id, h.match_loci, h.match_len, h.strand, 0};
                   rec_of[at] = order[k];
               },
               [&](size_t n) { reqs.resize(n); rec_of.resize(n); });
    bk::RawVec<bk_site_res> res(reqs.size());
    clk.lap("site requests made");
    const int sprc = bk_site_octamers(r.ctx, reqs.data(), reqs.size(), r.o.site_prefs_ofs, res.data());
    if (sprc) { diag("Fatal: the start-site octamer gather failed: %s", bk_strerror(sprc)); return 1; }
    clk.lap("site octamers gathered (device)");
    bk::site_prefs_pass(reqs.data(), res.data(), rec_of.data(), reqs.size(), rec.size(), r.site_prefs);
    bk::site_prefs_scale(r.site_prefs);
    clk.lap("site preferences counted and scaled");
    diag("Completed alignment site probabilities");
    return 0;
}

// --mark-duplicates: the templates of the final record set in load order go to the first device (bk_mark_duplicates), the records of
// the duplicates among them get their byte in rec.dup, which every writer turns into FLAG 0x400; nothing else of a record changes
int mark_duplicates(AlignRun &r)
{
    bk::RecordSet &rec = r.rec;
    if (r.ctx == nullptr) { diag("Fatal: '--mark-duplicates' needs a device context"); return 1; }
    diag("Processing to mark duplicate templates...");
    HostClock clk;
    std::vector<bk_dup_req> reqs;
    std::vector<uint32_t> first;
    duplicate_templates(rec, r.o.pe_mode != 0, reqs, first);
    size_t n_pairs = 0;
    for (const bk_dup_req &q : reqs) n_pairs += q.strand_mate != 0;
    clk.lap("duplicate requests made");
    std::vector<uint8_t> answers(reqs.size());
    bk_dup_totals tot{};
    const int rc = bk_mark_duplicates(r.ctx, reqs.data(), reqs.size(), answers.data(), &tot);
    if (rc != BK_OK) { diag("Fatal: the duplicates could not be marked on the device: %s", bk_strerror(rc)); return 1; }
    clk.lap("duplicates grouped (device)");
    if (tot.flagged) { diag("Fatal: the duplicate marking pass turned %llu of %zu requests down", (unsigned long long)tot.flagged, reqs.size()); return 1; }
    const long n_marked = duplicate_apply(rec, reqs, first, answers);
    if (n_marked < 0) { diag("Fatal: the duplicate marking pass left a request unanswered"); return 1; }
    clk.lap("duplicate records marked");
    diag("Duplicates: %zu templates (%zu fragments, %zu pairs) in %llu groups, %llu templates (%ld records) marked as duplicates, largest group %llu", reqs.size(),
         reqs.size() - n_pairs, n_pairs, (unsigned long long)tot.groups, (unsigned long long)tot.duplicates, n_marked, (unsigned long long)tot.max_group);
    return 0;
}

// --junctions / --splice-strand: one request per accepted record of the final record set whose line has an N goes to the first device
// (bk_junctions); the table is written here, the strands go into rec.xs, which every SAM / BAM writer turns into XS:A:<c>; nothing else of a
// record changes
int splice_junctions(AlignRun &r)
{
    bk::RecordSet &rec = r.rec;
    const AlignOpts &o = r.o;
    if (r.ctx == nullptr) { diag("Fatal: '--junctions' / '--splice-strand' need a device context"); return 1; }
    diag("Processing splice junctions of the accepted alignments...");
    HostClock clk;
    std::vector<bk_junction_req> reqs;
    std::vector<uint32_t> rec_of;
    junction_requests(rec, reqs, rec_of);
    clk.lap("junction requests made");
    const bool table = !o.junctions_path.empty();
    std::vector<uint8_t> strands(reqs.size());
    std::vector<bk_junction> jcts(table ? reqs.size() : 0);
    uint64_t nj = 0;
    bk_junction_totals tot{};
    const int rc = bk_junctions(r.ctx, reqs.data(), reqs.size(), o.splice_strand ? strands.data() : nullptr, table ? jcts.data() : nullptr, jcts.size(), &nj, &tot);
    if (rc != BK_OK) { diag("Fatal: the splice junctions could not be made on the device: %s", bk_strerror(rc)); return 1; }
    clk.lap("junctions grouped (device)");
    if (tot.flagged) diag("Warning: the junction pass turned %llu of %zu requests down", (unsigned long long)tot.flagged, reqs.size());
    if (o.splice_strand) junction_apply_strands(rec, rec_of, strands);
    if (table) {
        std::string text;
        for (uint64_t k = 0; k < nj; k++) {
            const bk_junction &j = jcts[k];
            if (j.chrom_id < 1 || j.chrom_id > r.n_ent) { diag("Fatal: the junction pass returned a sequence that is none of the index"); return 1; }
            junction_line(j, r.ents[j.chrom_id - 1].name, text);
        }
        OutBuf out;
        out.open(o.junctions_path.c_str());
        if (out.fd < 0) { diag("Fatal: unable to create '%s'", o.junctions_path.c_str()); return 1; }
        out.put(text);
        out.close();
        if (out.failed) { diag("Fatal error: unable to write the junction table to '%s'", o.junctions_path.c_str()); return 1; }
        clk.lap("junction table written");
    }
    diag("Junctions: %zu spliced records, %llu junctions (%llu GT/AG, %llu other canonical, %llu non-canonical), most reads at one junction %llu", reqs.size(),
         (unsigned long long)tot.junctions, (unsigned long long)(tot.by_motif[1] + tot.by_motif[2]),
         (unsigned long long)(tot.by_motif[3] + tot.by_motif[4] + tot.by_motif[5] + tot.by_motif[6]), (unsigned long long)tot.by_motif[0], (unsigned long long)tot.max_reads);
    return 0;
}

// the writers, then the files that come behind them: the site preferences of -8, the SNPs of -p.  0, or the failed writer's code.
int write_reports(AlignRun &r)
{
    AlignOpts &o = r.o;
    const Args &a = r.a;
    diag("Reporting of aligned result set started...");
    diag("Sorting alignments by ascending chrom.loci");
    if (!r.with_site_prefs) sorted_order(r.rec, o.nthreads, r.order);

    Report R{a, r.rs, r.rec, r.ents, r.species, r.n_ent, r.multi_dist, r.order, o.pe_mode, o.ml_mode, o.max_ml, o.fmt, o.nthreads, o.micro_indel, o.splice_len, o.max_rpt_sam_seqs};
    R.ctx = r.ctx;
    R.sam_tags = (uint32_t)o.sam_tags;
    R.site_prefs = r.with_site_prefs ? &r.site_prefs : nullptr;
    R.pre = r.pre.fd >= 0 ? &r.pre : nullptr;
    r.S.done_with_head_start();
    R.restore_reads = [&r]() { return restore_reads(r); };
    R.sam_prep = r.sam_prep;
    R.pk_words = r.pk_job.pk_words; R.n_pk_words = r.pk_job.n_pk_words; R.pk_lens16 = r.pk_job.pk_lens16; R.pk_exc = r.pk_job.pk_exc; R.n_pk_exc = r.pk_job.n_pk_exc;
    r.sam_prep = nullptr;                          // (the report owns it from here)
    // ".bam": BGZF-compressed BAM with its BAI index; else SAM / CSV / BED text
    const std::string opath = a.str("o");
    int rr = (o.fmt >= 5 && is_bam_name(opath)) ? report_bam(R, opath) : report_text(R);
    if (R.sam_prep) { bk_sam_prep_free(R.sam_prep); R.sam_prep = nullptr; }        // (the report took another path)
    if (rr == 0 && !o.coverage_path.empty()) rr = write_coverage(R, o.coverage_path);      // --coverage: behind the writer, on the first device
    if (rr == 0 && r.with_site_prefs) {             // WriteSitePrefs, behind the writers and the -O statistics (Aligner.cpp:743)
        std::string csv;
        bk::site_prefs_csv(r.site_prefs, csv);
        OutBuf sp_file;
        sp_file.open(o.site_prefs_path.c_str());
        const bool opened = sp_file.fd >= 0;
        if (opened) { sp_file.put(csv); sp_file.close(); }
        if (!opened || sp_file.failed) { diag("Fatal error: unable to write the site preferences to '%s'", o.site_prefs_path.c_str()); rr = -85; }
    }
    // SNPs: the file is only opened for '-M0' .. '-M5' (Aligner.cpp:4488), and only processed when reads were accepted (:746)
    if (rr == 0 && o.snp.min_reads > 0 && o.fmt <= 5) {
        o.snp.path = a.has("S") ? a.str("S") : opath + ".snp";
        o.snp.bed = o.fmt == 4;
        o.snp.vcf = !o.snp.bed && o.snp.path.size() >= 4 && !strcasecmp(o.snp.path.c_str() + o.snp.path.size() - 4, ".vcf");     // Aligner.cpp:157-165
        o.snp.title = a.str("t", "kanga");
        o.snp.sfx_path = a.str("I");
        bool any = false;
        for (const bk_hit &h : r.rec.hits) if (h.nar == BK_NAR_ACCEPTED) { any = true; break; }
        if (any) rr = process_snps(r.ctx, R, o.snp);
        else for (const char *ext : {"", ".disnp.csv", ".trisnp.csv", ".markers"}) { if (ext[1] == 'm' && !o.snp.marker_len) continue; OutBuf e; e.open((o.snp.path + ext).c_str()); e.close(); }
    }
    return rr;
}

// The run, top to bottom, in the reference's order (CAligner::Align, Aligner.cpp:195-760)
int cmd_align(int argc, char **argv, int first)
{
    AlignRun r;
    const AlignOpts &o = r.o;
    if (parse_align_args(argc, argv, first, r.a)) return 1;
    if (r.a.has("F")) g_logfile = fopen(r.a.str("F").c_str(), "a");
    diag("Subprocess align Version %s starting", kProgVer);
    if (read_align_opts(r.a, r.o)) return 1;
    r.ndev = o.devices.size();
    if (make_contam_matcher(r)) return 1;
    if (print_param_lines(o)) return 1;

    diag("Loading suffix array file '%s'", r.a.str("I").c_str());
    estimate_input(r);
    start_early_buffers(r);
    choose_index_image(r);
    load_reads_behind_index(r);                     // (the loader threads run ..
    if (pack_reads_and_join_index(r)) return 1;     //  .. until here: no return in between)
    if (!o.constraints_path.empty() && load_constraints(r)) return 1;
    tune_and_describe_image(r);
    start_sam_file_late(r);
    if (make_accept_table(r)) return 1;
    if (run_alignment(r)) return 1;
    start_sam_head(r);

    resolve_multi_and_count_pairs(r);
    if (o.min_chim) keep_chimeric_trims(r.rec);
    if (!o.constraints_path.empty() && apply_loci_constraints(r)) return 1;
    if (o.pcr_win >= 0 && !o.pe_mode) reduce_pcr_artefacts(r);
    if (o.primer_subs > 0 && correct_primer_artefacts(r)) return 1;
    if (o.min_flank > 0 && trim_flanks(r)) return 1;
    remove_orphan_junctions(r);
    if (!o.re_excl.empty() || !o.re_incl.empty()) filter_by_chroms(r);
    if (report_align_stats(r)) return 1;
    if (o.mark_dups && mark_duplicates(r)) return 1;
    if ((!o.junctions_path.empty() || o.splice_strand) && splice_junctions(r)) return 1;

    r.with_site_prefs = !o.site_prefs_path.empty() && r.nar[1] > 0;
    if (r.with_site_prefs && gather_site_prefs(r)) return 1;
    const int rr = write_reports(r);
    if (rr == 0 && r.rec.size() >= 1000000) {       // (small runs unwind normally: leak checkers and tests see every destructor)
        r.pre.finish();
        end_process(rr);                            // (contexts, page-locked buffers and the address space go with the process)
    }
    return rr;
}

// CUtility::arg_parsefromfile (libbiokanga/Utility.cpp:793-910; called first thing by every sub-process, kanga.cpp:298): an argument
// "@file" is replaced by the options found in that file - one or more per line, separated by blanks or tabs except inside quotes
// (the quote characters stay part of the option, as they do there); empty lines and lines starting with '#', ';' or "//" are skipped
bool expand_param_files(int argc, char **argv, std::vector<std::string> &out)
{
    for (int i = 0; i < argc; i++) {
        if (argv[i][0] != '@') { out.push_back(argv[i]); continue; }
        std::string fn = argv[i] + 1;
        while (!fn.empty() && isspace((unsigned char)fn.back())) fn.pop_back();
        size_t b0 = 0;
        while (b0 < fn.size() && isspace((unsigned char)fn[b0])) b0++;
        fn = fn.substr(b0);
        FILE *f = fn.empty() ? nullptr : fopen(fn.c_str(), "r");
        if (!f) { printf("Unable to open options file '%s'\nError: %s", fn.c_str(), strerror(errno)); return false; }
        char line[8192];
        while (fgets(line, sizeof(line), f)) {
            std::string l = line;
            while (!l.empty() && isspace((unsigned char)l.back())) l.pop_back();
            size_t a = 0;
            while (a < l.size() && isspace((unsigned char)l[a])) a++;
            l = l.substr(a);
            if (l.empty() || l[0] == '#' || l[0] == ';' || (l[0] == '/' && l.size() > 1 && l[1] == '/')) continue;
            std::string opt;
            bool in_quotes = false, in_param = false;
            for (size_t k = 0; k <= l.size(); k++) {
                char ch = k < l.size() ? l[k] : '\0';
                if (ch == 0x16) ch = '-';
                if (ch == '"' || ch == '\'') { in_quotes = !in_quotes; in_param = true; opt.push_back(ch); continue; }
                if ((ch == ' ' || ch == '\t') && in_quotes) { opt.push_back(ch); continue; }
                if (ch == ' ' || ch == '\t' || ch == '\0') {
                    if (!in_param && ch != '\0') continue;
                    out.push_back(opt);
                    opt.clear();
                    in_quotes = in_param = false;
                    continue;
                }
                in_param = true;
                opt.push_back(ch);
            }
        }
        fclose(f);
    }
    return true;
}

}  // namespace

int main(int argc_in, char **argv_in)
{
    std::vector<std::string> expanded;
    if (!expand_param_files(argc_in, argv_in, expanded)) return 1;
    std::vector<char *> argv_vec;
    for (std::string &a : expanded) argv_vec.push_back(&a[0]);
    argv_vec.push_back(nullptr);
    const int argc = (int)expanded.size();
    char **argv = argv_vec.data();
    // gszProcName: basename of argv[0] without extension (biokanga.cpp:236-246)
    std::string p = argv[0];
    size_t sl = p.find_last_of('/');
    if (sl != std::string::npos) p = p.substr(sl + 1);
    size_t dot = p.find_last_of('.');
    if (dot != std::string::npos && dot > 0) p = p.substr(0, dot);
    if (!p.empty()) g_proc = p;
    if (argc < 2) {
        fprintf(stderr, "%s: MI355X build of the BioKanga `index` and `align` sub-processes (%s)\nusage: %s index|align <options>\n",
                g_proc.c_str(), bk_version(), g_proc.c_str());
        return 1;
    }
    g_t0 = time(nullptr);
    int rc;
    std::string sub = argv[1];
    if (sub == "index" || sub == "kangax") rc = cmd_index(argc, argv, 2);
    else if (sub == "align" || sub == "kanga") rc = cmd_align(argc, argv, 2);
    else {
        fprintf(stderr, "%s: sub-process '%s' is outside the supported hot path (index, align)\n", g_proc.c_str(), sub.c_str());
        return 1;
    }
    diag("Exit code: %d Total processing time: %ld seconds", rc, (long)(time(nullptr) - g_t0));
    return rc;
}
