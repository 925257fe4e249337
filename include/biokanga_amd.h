/*
 * biokanga_amd.h - C ABI of the MI355X-native `biokanga align` hot path (libbiokanga_amd.so).
 *
 * Drop-in boundary.  The reference (csiro-crop-informatics/biokanga v4.4.2) has no FFI of its own;
 * the seam is the pair of call sites SURVEY.md §8(b) names:
 *   - per read : CSfxArrayV3::AlignReads            libbiokanga/SfxArrayV2.h:585-606, called from
 *                CAligner::ProcCoredApprox          biokanga/Aligner.cpp:9220-9237
 *   - per batch: CAligner::LocateCoredApprox        biokanga/Aligner.h:930-931 (Aligner.cpp:8651)
 * bk_align_batch() is the batch form of the first placed where the second is: it consumes the
 * reads exactly as CAligner holds them (1 byte/base: bits 0-2 base, bit 3 soft-mask, bits 4-7
 * quality, biokanga/Aligner.cpp:9038-9055) and fills, per read, the fields ProcCoredApprox writes
 * into tsReadHit (NAR, NumHits, LowHitInstances, LowMMCnt, NxtLowMMCnt, HitLoci.Hit.Seg[0]).
 *
 * Plain pointers and sizes only; no C++/torch types.  Every function returns 0 (eBSFSuccess) or a
 * negative teBSFrsltCodes value (libbiokanga/ErrorCodes.h:15-95); HIP/RCCL failures map to
 * BK_ERR_INTERNAL.  The library never calls exit().  There is NO CPU fallback: without a usable
 * HIP device every compute entry point fails with BK_ERR_NODEVICE.
 */
#ifndef BIOKANGA_AMD_H
#define BIOKANGA_AMD_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* teBSFrsltCodes subset (libbiokanga/ErrorCodes.h) */
#define BK_OK               0
#define BK_ERR_INTERNAL    (-1)    /* eBSFerrInternal  */
#define BK_ERR_PARAMS      (-100)  /* eBSFerrParams    */
#define BK_ERR_MEM         (-95)   /* eBSFerrMem       */
#define BK_ERR_NOTBIOSEQ   (-94)   /* eBSFerrNotBioseq */
#define BK_ERR_OPNFILE     (-90)   /* eBSFerrOpnFile   */
#define BK_ERR_CREATEFILE  (-89)   /* eBSFerrCreateFile*/
#define BK_ERR_FILEVER     (-86)   /* eBSFerrFileVer   */
#define BK_ERR_FILEACCESS  (-85)   /* eBSFerrFileAccess*/
#define BK_ERR_NODEVICE    (-2)    /* ours: no HIP device / kernels unavailable */

/* tHRslt, libbiokanga/SfxArrayV2.h:68-74 */
enum { BK_HR_NONE = 0, BK_HR_HITS = 1, BK_HR_MMDELTA = 2, BK_HR_HITINSTS = 3, BK_HR_RMMDELTA = 4 };
/* teNAR, biokanga/Aligner.h:106-128 (values produced by the hot path) */
enum { BK_NAR_UNALIGNED = 0, BK_NAR_ACCEPTED = 1, BK_NAR_NS = 2, BK_NAR_NOHIT = 3, BK_NAR_MMDELTA = 4,
       BK_NAR_MULTIALIGN = 5 };

/* alignment parameters = the `biokanga align` options that reach the hot path
 * (biokanga/kanga.cpp:194-294) */
typedef struct bk_align_params {
    int32_t max_subs;       /* -s  max substitutions per 100 bp (reference default 10)         */
    int32_t min_edit_dist;  /* -e  minimum Hamming delta to the next best hit, 1 or 2           */
    int32_t align_strand;   /* -Q  0 both strands, 1 sense only, 2 antisense only               */
    int32_t pmode;          /* -m  0 default, 1 more sensitive, 2 ultra sensitive, 3 less sens. */
    int32_t max_ns;         /* -n  max indeterminate bases per 100 bp (default 1)               */
    int32_t max_ml;         /* -R  MaxMLmatches (MaxHits of AlignReads): 1 in the default -r0 mode, 2..BK_MAX_ML in the
                             *     multi-loci modes -r1..-r5, whose loci lists bk_batch_loci() then returns         */
    int32_t clamp_ml;       /* -X  with max_ml > 1: reads with more than max_ml loci (rslt eHRHitInsts) also get a loci
                             *     list, of their first max_ml loci (bClampMaxMLmatches, Aligner.cpp:9243-9248)        */
    int32_t best_matches;   /* -N  with max_ml > 1: CSfxArrayV3::LocateBestMatches instead of AlignReads - per read the (up to)
                             *     max_ml loci with the fewest mismatches, none above the -s limit, ordered by mismatches
                             *     then discovery; bk_hit.rslt is eHRhits / eHRnone, LowMMCnt and NxtLowMMCnt stay 0          */
    int32_t micro_indel_len;/* -a  0, or the longest microInDel (1..20) looked for in reads the AlignReads phases leave unaligned
                             *     (CSfxArrayV3::LocateInDels); second segments come back through bk_batch_seg2()             */
    int32_t splice_junct_len;/* -A  0, or the longest splice junction (25..100000) looked for in reads still unaligned after that
                             *     (CSfxArrayV3::LocateSpliceJuncts); second segments through bk_batch_seg2(), flags bit 2      */
    int32_t min_chimeric_len;/* -c  0, or 50..99: reads nothing else aligned may be placed end-trimmed, keeping at least this percentage of
                             *     their length (chimeric form of LocateCoreMultiples); trims through bk_batch_seg2(), flags bit 3 */
    int32_t orphan_core_subs1;/* -6  0: nothing; r + 1: the paired-end orphan recovery derives its core length from rate r per 100 bp (the user's -s,
                             *     m_MaxSubs at Aligner.cpp:3256,3354) while max_subs - then the initial rate min(s + n, 15) - stays what
                             *     its alignments may carry (pPars->MaxSubs, :3275,3373).  One more than the rate: -s0 -6 n is legal     */
} bk_align_params;

/* per-read result: the tsReadHit fields written by ProcCoredApprox (Aligner.cpp:9311-9479) and
 * tsHitLoci.Seg[0] (SfxArrayV2.h:219-240).  20 bytes, little endian. */
typedef struct bk_hit {
    uint32_t chrom_id;           /* Seg[0].ChromID = tsSfxEntry.EntryID (1..n), 0 if none        */
    uint32_t match_loci;         /* Seg[0].MatchLoci, 0-based within the entry                   */
    uint16_t match_len;          /* Seg[0].MatchLen                                              */
    int16_t  low_hit_instances;  /* tsReadHit.LowHitInstances                                    */
    uint8_t  rslt;               /* tHRslt returned by AlignReads                                */
    uint8_t  nar;                /* teNAR                                                        */
    uint8_t  strand;             /* '+', '-' or '?'                                              */
    int8_t   low_mm;             /* tsReadHit.LowMMCnt                                           */
    int8_t   nxt_low_mm;         /* tsReadHit.NxtLowMMCnt                                        */
    uint8_t  num_hits;           /* tsReadHit.NumHits                                            */
    uint8_t  mismatches;         /* Seg[0].Mismatches (Hamming score of the accepted hit)        */
    uint8_t  flags;              /* bit 7: FlgPEAligned (bk_pair_batch); bits 0-6: the engine's, no meaning outside it */
} bk_hit;

/* counters behind the "algorithmic bytes" figure of SURVEY.md §8(d); all are counts of what the
 * REFERENCE algorithm does for the same reads (independent of our data layout) */
typedef struct bk_counters {
    uint64_t n_reads;
    uint64_t n_search;      /* LocateFirstExact calls                                  */
    uint64_t n_cand;        /* candidates Hamming-extended (new, in-bounds targets)    */
    uint64_t n_lcm_calls;   /* LocateCoreMultiples invocations                         */
    uint64_t n_heavy;       /* (ours) LocateCoreMultiples calls routed to the wave-per-read kernels */
    uint64_t n_cand_heavy;  /* (ours) the part of n_cand processed by the wave-per-read kernels    */
    uint64_t reserved[2];
} bk_counters;

/* timing of the device work of the last bk_align_batch*() call, measured with HIP events on the
 * stream the kernels were launched on */
typedef struct bk_timing {
    float    ms_total;          /* first kernel start -> last kernel end                       */
    float    ms_search;         /* sum over launches of the SA-interval search kernel          */
    float    ms_extend;         /* sum over launches of the candidate walk / Hamming kernel    */
    float    ms_heavy;          /* sum over launches of the wave-per-read kernel               */
    float    ms_other;          /* pack / finalize                                             */
    uint32_t n_search_launches;
    uint32_t n_extend_launches;
    uint32_t n_heavy_launches;
    uint32_t n_search_b_launches;
    /* the search stage by kernel (ms_search = their sum + the clears of the interval records): pass A (k-mer table + small buckets),
     * the grouping of pass B's work list (keys + radix sort), pass B (bisection of the big buckets) */
    float    ms_search_a;
    float    ms_search_sort;
    float    ms_search_b;
    float    ms_prep;           /* read preparation (2-bit rows of both strands, N policy, first active list); part of ms_other */
} bk_timing;

typedef struct bk_entry_info {
    uint32_t entry_id;
    uint32_t seq_len;
    uint64_t start_ofs;
    uint64_t end_ofs;
    char     name[81];
} bk_entry_info;

typedef struct bk_ctx bk_ctx;

const char *bk_version(void);
const char *bk_strerror(int rc);
/* number of usable HIP devices (0 if none); never fails */
int  bk_device_count(void);

/* Replaces CSfxArrayV3::Open + SetTargBlock (libbiokanga/SfxArrayV2.cpp:891-1103,1836-1890) and the
 * MinCoreLen/MaxIter set-up of CAligner::Align / LocateCoredApprox (Aligner.cpp:341-356,8725-8761):
 * reads the .sfx file, uploads target + suffix array to HBM, builds the k-mer interval table. */
int  bk_ctx_create(bk_ctx **out, const char *sfx_path, int device_id, const bk_align_params *p);
/* The same with flags.  BK_CTX_WINDOW_ARRAY_EAGER: the suffix-ordered window array - 48 bytes for every suffix of the part of the suffix
 * array the wave kernel's long walks visit, a sixth of a 3.1 Gbp index (25 GB) - is part of the image from the start: made slice by
 * slice behind the suffix array's upload, as the other tables are, for reads of a hundred bases (a first batch that is searched with
 * other core lengths makes it again: 0.1 s); without the flag the array is made when the first batch it can serve arrives (tuning knob
 * "use_swin").  Replaces the candidates' random target reads of LocateCoreMultiples' walk (libbiokanga/SfxArrayV2.cpp:5862-5915) by a
 * streaming read; results never depend on it. */
#define BK_CTX_WINDOW_ARRAY_EAGER 1u
/* BK_CTX_LEAN_IMAGE: the tables that only pay from tens of millions of reads on are left out - the k-mer table's second words (a
 * bucket's only key, or the map of its keys' first five bits; "use_ktab2": 17 GB more at 3.1 Gbp, 0.18 ns per read of a hundred bases
 * together with the next) and the third- and fourth-level search keys ("use_k3": 4 bytes per suffix each).  Without the flag they are
 * part of the image wherever a fifth of the HBM stays free behind them, made behind the suffix array's upload like the other tables
 * (0.05 - 0.2 s of a 3.1 Gbp index's load on an idle device: profiles/r06_*_e2e_image*.txt).  Results never depend on it. */
#define BK_CTX_LEAN_IMAGE 2u
/* BK_CTX_NO_DEEP_KEYS: the third- and fourth-level search keys alone are left out (8 bytes per suffix: 26 GB at 3.1 Gbp).  Results
 * never depend on it. */
#define BK_CTX_NO_DEEP_KEYS 4u
/* BK_CTX_GROW_IMAGE: the context starts with the lean image - what a job of a few million reads wants - and, should it turn out to
 * align 5 x BK_POLICY_MIN_READS reads after all (tuning knob "grow_after_reads"), makes the tables BK_CTX_LEAN_IMAGE leaves out in the
 * background: a thread of its own allocates and fills them on a stream of its own and the next batch after they are complete takes
 * them in.  "image_wait" makes them at once and waits; the environment's BK_GROW_AFTER_READS=<n> sets the threshold of every context
 * created with the flag and makes the batch after the one that started the worker wait for it (tests: a small run that grows).
 * Results never depend on it. */
#define BK_CTX_GROW_IMAGE 8u
/* The image a job gets, by ONE rule for the command line (`biokanga align`, which knows its read count from the input files' sizes),
 * the benchmark and any other caller: the flags for bk_ctx_create_ex from the reads one device is going to align.  From
 * BK_POLICY_MIN_READS on: every table and the window array from the start (BK_CTX_WINDOW_ARRAY_EAGER - 0.1 - 0.2 s more load for 0.7 ns
 * less per read of a hundred bases at 3.1 Gbp); below, or when the count is not known (0): BK_CTX_GROW_IMAGE. */
#define BK_POLICY_MIN_READS 20000000ULL
uint32_t bk_image_policy(uint64_t reads_per_device);
int  bk_ctx_create_ex(bk_ctx **out, const char *sfx_path, int device_id, const bk_align_params *p, uint32_t flags);

/* Same, from an index image already resident in HBM (synthetic benchmarks, GPU-built indexes):
 * d_seq  = concat_len bytes, 1 byte/base, eBaseEOS(7) after every entry (tsSfxBlock.SeqSuffix)
 * d_sa   = concat_len suffix array elements of sfx_el_size (4 or 5) bytes, little endian
 * entries (host) describe the sequences as tsSfxEntry does.  The buffers are copied/re-packed;
 * the caller keeps ownership and may free them after the call returns. */
int  bk_ctx_create_from_device(bk_ctx **out, const void *d_seq, uint64_t concat_len, const void *d_sa,
                               int sfx_el_size, const bk_entry_info *entries, uint32_t n_entries,
                               int device_id, const bk_align_params *p);

/* A second context on another (or the same) device from the finished index image of `src`: every table is copied device to device
 * (hipMemcpyPeer: over xGMI between two GPUs) instead of reading the .sfx again and rebuilding the tables there - how one process
 * replicates the index over the GPUs of a node.  Parameters are those of `src`; tuning knobs set on `src` after its
 * creation that change the image (kmer_bits, use_k2, use_isa, use_tgt2) are inherited with it. */
int  bk_ctx_clone(bk_ctx **out, const bk_ctx *src, int device_id);

void bk_ctx_destroy(bk_ctx *ctx);

/* Sizes the context's batch scratch (read rows, interval records, work lists, sort buffers) for batches of up to max_batch_reads reads
 * of up to max_read_len bases NOW, and makes the table of the reads' core geometry per length under the parameters as they stand, so that
 * no allocation is left for the first batch to pay inside T_align - the reference sizes its
 * per-thread scratch before its workers start, too (CAligner::LocateCoredApprox, Aligner.cpp:8771-8790).  Optional for the blocking
 * calls and the pipeline (batches grow the scratch on demand), required by bk_align_batch_device_async. */
int  bk_ctx_reserve(bk_ctx *ctx, uint32_t max_batch_reads, uint32_t max_read_len);

/* The chromosome filters (-Z / -z) as the paired-end rules see them: accept[id] != 0 <=> CAligner::AcceptThisChromID(id) (Aligner.cpp:2651-2715),
 * consulted by AcceptProvPE (:2771-2786), by the anchors of the orphan recovery (:3224,3323) and by the single-end acceptance at the end of
 * ProcessPairedEnds (:3445-3473).  ids >= n pass; n == 0 removes the table.  Only bk_pair_batch* (and pipelines created with `pe`) look at it:
 * the filters never change a single read's alignment. */
int  bk_ctx_set_chrom_filter(bk_ctx *ctx, const uint8_t *accept, uint32_t n);

/* change alignment parameters (re-derives MinCoreLen, MaxIter, slides) */
int  bk_ctx_set_params(bk_ctx *ctx, const bk_align_params *p);
/* cross-check knobs: results never depend on them; the test-suite runs independent implementations of the same step against
 * each other through these.  name =
 *   "kmer_bits" (k of the k-mer table, 2..16)   "use_ktab" (0: plain bisection)   "use_k2" (second-level key array)
 *   "use_iv32" (phase 0 hands the interval of a read's first k + 16 bases to the later phases)   "lazy_search" (small buckets handed on unverified)
 *   "iv_poison" (test hook, 0: the interval records a phase can use are filled with ones in front of its search - nothing clears them
 *   otherwise, the search stores the slot of every core a read has -, so that a slot read without having been written in that phase shows)
 *   "wave_len_spec" (1, the default: a batch whose reads all have the same number of 16-base dwords gets the wave kernel's form compiled
 *   for that count; 0: the generic form always.  Host only: which kernel is launched, no kernel argument)
 *   "use_ktab2" (k-mer table entries of two words, 17 GB more at k = 16: 1, the default - a bucket of one suffix carries its second-level key and is
 *   settled by the line that names it; 2 - it carries the suffix array element and the search hands the suffix on for the extension to check:
 *   no trip to the suffix array for it, but every bucket whose key the search would have turned down is a candidate - slower, round 6)
 *   "grow_after_reads" / "grow_state" / "image_wait" (BK_CTX_GROW_IMAGE: the reads after which the long-run tables are made; 0 not started, 1 being
 *   made, 2 made, 3 nothing made, 4 taken in, 5 not a growing context; make them now and wait: returns key arrays + 4 if the k-mer table carries keys)
 *   "use_k3" (0..2: key arrays of the 15 bases behind the second-level keys' and of the 15 behind those - 4 bytes per suffix each, where the
 *   HBM has the room; how many there are: "k3_resident")
 *   "sort_lists" (bit 0: search work list grouped by bucket - by default only where the index has no third-level keys -, bit 1: wave list
 *   sorted, bit 2: .. longest read first)
 *   "search_split" (pass B of the search in two launches: the key levels, then - a lane per item again, all of one kind - the bisections
 *   over suffix array and target that they leave and the full searches; 1 by default where the work list is not grouped, 0 where it is.
 *   Host only: which kernels are launched; the same records either way)
 *   "prep_search0" (phase 0's first search pass inside the read preparation instead of a launch of its own; 1 by default, in effect on
 *   the register-window path with the two-word k-mer table and 4-byte elements.  Host only; the same records either way)
 *   "use_wave" (wave kernel, 0: general hash-set kernel)   "use_isa" (inverse suffix
 *   array dedupe, 0: hash set)   "use_tgt2" (2 bit/base window compare)   "heavy_thresh" (longest interval the lane/flat kernels take, 0..100)
 *   "use_swin" (suffix-ordered window array: 0 none - every window from the 2-bit target; 1 for the part of the suffix array the wave kernel's long
 *   walks visit, reads of <= 100 bases and the middle cores of reads of <= 160; 2 the same whatever the batch's longest read; 3 for every suffix.
 *   An index of 5-byte elements gets the partial array only at 2: making it goes over such an index twice - once to find the shortest run
 *   length whose coverage fits the memory that is free -, 2 s at 17 Gbp for a seventh of its wave kernel's time)
 *   "swin_budget_kb" (most the partial array may take; 0: a third of what every suffix would, within half of the free HBM - nearly all of it for an
 *   index beyond 2^32 suffixes)   "swin_skip_short" (the coverage rule without the reads' this many shortest core lengths; 0)
 *   "ktab_wide" (tests: 1 = the k-mer table with 64-bit bucket starts whatever the index's size, packed as an index beyond 2^32 suffixes has
 *   it - a 64-bit start per 2^16 codes + 32-bit offsets, half the bytes -, 2 = unpacked; rebuilt)   "ktab_packed" (read only)
 *   "swin_resident", "swin_mbytes", "swin_setup_us", "swin_covered_ppm", "swin_core_lens" (read only, value ignored: whether the window array
 *   is in HBM right now, what it occupies, what making it took, the share of the suffix array it holds, the core lengths its coverage is for)
 *   "async_phases" (1: the main path's phase loop never reads a count back - launches sized by bounds, sorts by the previous chunk's
 *   needs; 0: counts read back between launches, as every other configuration does)
 *   "force_rccl" (bk_seq_counts_allreduce goes through RCCL - a communicator of one rank - even when every context sits on one device; how many
 *   of a context's reductions did, and the ranks of the last one's communicator: "rccl_allreduces", "rccl_ranks", read only)
 *   "debug_stop_phase" (test hook, see bk_debug_intervals)
 *   "chunk_reads" (reads per pass over the phases)   "max_read_len"   "site_chunk" (requests bk_site_octamers stages at a time)
 *   "primer_chunk" (requests bk_primer_correct stages at a time; "primer_buf_bytes": what its staging holds now, read only)
 *   "constraint_chunk" (requests bk_constraints_check stages at a time)
 *   "samtag_chunk" (requests bk_samtags stages at a time; "samtag_buf_bytes": what its staging holds now, read only)
 *   "coverage_slice_bases" (target bases bk_coverage_* takes per slice, one int32 each; 0 - the default - until the first call
 *   derives it from the free memory), "coverage_run_chunk" (runs per sink call), "coverage_req_chunk" (requests staged at a time),
 *   "coverage_buf_bytes" (what its staging holds now, device and page-locked; read only)
 *   "dup_table_slots" (slots of bk_mark_duplicates' table; 0 - the default - derives them per call: the smallest power of two
 *   >= 2 n, at least 1024; any other value is checked by the call), "dup_buf_bytes" (what its staging and table hold now; read only)
 *   "junction_table_slots", "junction_buf_bytes" (the same two for bk_junctions)
 * returns the old value or <0 */
int64_t bk_ctx_tune(bk_ctx *ctx, const char *name, int64_t value);

uint32_t bk_num_entries(const bk_ctx *ctx);
int  bk_get_entry(const bk_ctx *ctx, uint32_t idx, bk_entry_info *out);
const char *bk_dataset_name(const bk_ctx *ctx);
uint64_t bk_concat_len(const bk_ctx *ctx);
int  bk_sfx_el_size(const bk_ctx *ctx);
int  bk_min_core_len(const bk_ctx *ctx);

/* Batch form of CSfxArrayV3::AlignReads over host buffers (blocking).
 * bases: all reads concatenated, 1 byte/base as CAligner holds them; offs[i] = start of read i in
 * bases; lens[i] = read length (<= 2000); out[nreads]. */
int  bk_align_batch(bk_ctx *ctx, const uint8_t *bases, const uint64_t *offs, const uint32_t *lens,
                    uint32_t nreads, bk_hit *out);

/* Same over buffers already resident in HBM on the context's device.  The kernels are launched on `stream` (a
 * hipStream_t, NULL = the context's own stream), after whatever that stream already holds.  The call is
 * HOST-SYNCHRONOUS: it measures the batch's longest read, sizes (and may allocate) the batch scratch, and returns when the
 * results are in d_out; `sync` is accepted and has no effect.  The overlapped form (uploads, kernels and downloads of
 * consecutive batches running concurrently) is bk_stream_*; the form that only enqueues is below. */
int  bk_align_batch_device(bk_ctx *ctx, const void *d_bases, const void *d_offs, const void *d_lens,
                           uint32_t nreads, void *d_out, void *stream, int sync);

/* The same batch ENQUEUED on `stream` - every phase of AlignReads, none of it waited for: the call returns as soon as the launches
 * are made, d_out is complete when `stream` reaches that point.  A consumer kernel enqueued on the same stream (or on another
 * one behind an event recorded there) sees the results without the host ever waiting: the counts the phases produce - reads still
 * unaligned, work items, reads for the wave kernel - stay in device memory and the kernels size themselves by them
 * (the reference's workers never leave their loop either, Aligner.cpp:8943-9527).
 * Needs: the scratch in place for batches of this size and read length (bk_ctx_reserve - called again after bk_ctx_set_params has changed
 * -s / -e / -M: the geometry table it makes goes by them), max_read_len >= the longest read of the
 * batch (the kernel family is picked by it; a longer read is reported by the NEXT call as BK_ERR_PARAMS - its records are not to be
 * used: the search gave it the core geometry of a read of max_read_len bases), reads of at most 512
 * bases, the default result form (no multi-loci lists, -a / -A / -c, -N), one batch of a context in flight per stream - the
 * scratch belongs to the context.  Otherwise BK_ERR_PARAMS before anything is launched: use the blocking call. */
int  bk_align_batch_device_async(bk_ctx *ctx, const void *d_bases, const void *d_offs, const void *d_lens,
                                 uint32_t nreads, uint32_t max_read_len, void *d_out, void *stream);

/* ---- packed reads: 2 bit/base across PCIe ------------------------------------------------------------------------
 * The 1 byte/base form above is how CAligner holds reads; of its 8 bits the hot path uses 3 (Aligner.cpp:9038-9055) and almost
 * always only 2.  Packed form of a batch:
 *   words  read i owns ceil(lens[i] / 16) consecutive 32-bit words, reads back to back in order; base j of a read sits in bits
 *          31-2(j%16) .. 30-2(j%16) of its word j/16 (first base in the top bits): 0 a, 1 c, 2 g, 3 t.  Bits past a read's end are ignored.
 *   lens   16 bits per read (reads are <= 2000 bases)
 *   exc    every base whose code (bits 0-2 of its byte in the 1 byte/base form) is not 0..3 - the indeterminate base N (4), or anything
 *          else (5..7, which make the reference refuse the read) - as runs: `run` + 1 consecutive bases of a read from `pos` on
 *          carry `code`; strictly ascending by (read, pos), runs do not overlap; the 2-bit fields of such bases are ignored.  Empty
 *          for most batches; a read of nothing but N is one entry.
 * 100-base reads cross PCIe as 30 bytes instead of 104.  Results are those of the 1 byte/base calls, bit for bit. */
typedef struct bk_nbase {
    uint32_t read;               /* index of the read within the batch */
    uint16_t pos;                /* first base of the run              */
    uint8_t  code;               /* 4 (N) .. 7                         */
    uint8_t  run;                /* further bases with the same code (0..255) */
} bk_nbase;                      /* 8 bytes */
/* number of words the packed form of these reads takes */
uint64_t bk_packed_words(const uint32_t *lens, uint32_t nreads);
/* host-side packer (the loader thread's job; uses a few threads): 1 byte/base reads -> the packed form.  offs == NULL: reads lie back
 * to back.  words must hold bk_packed_words(lens, nreads) entries, lens16 nreads, exc exc_cap entries; *n_exc receives the number of exceptions FOUND - when it exceeds exc_cap only the first exc_cap were stored and the call fails
 * with BK_ERR_MEM, to be repeated with a larger array.  Reads longer than 2000 bases: BK_ERR_PARAMS. */
int  bk_pack_reads(const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint32_t nreads, uint32_t *words, uint16_t *lens16,
                   bk_nbase *exc, uint64_t exc_cap, uint64_t *n_exc);
/* bk_align_batch over the packed form (host buffers, blocking); n_words = bk_packed_words() of the batch */
int  bk_align_batch_packed(bk_ctx *ctx, const uint32_t *words, uint64_t n_words, const uint16_t *lens, uint32_t nreads,
                           const bk_nbase *exc, uint64_t n_exc, bk_hit *out);

/* Paired-end association after the SE pass = CAligner::ProcessPairedEnds (biokanga/Aligner.cpp:
 * 2876-3489) incl. orphan recovery by CSfxArrayV3::AlignPairedRead (libbiokanga/SfxArrayV2.cpp:8247).
 * Reads and hits are interleaved PE1, PE2, PE1, PE2 ... (2 * n_pairs of each); hits must be the
 * results bk_align_batch() returned for exactly these reads and are updated in place
 * (NAR, NumHits, LowHitInstances, LowMMCnt, Seg[0]); bk_hit.flags bit 7 = FlgPEAligned. */
typedef struct bk_pe_params {
    int32_t pe_mode;        /* -U  1 orphan recovery, 2 unique only, 3 = 1 + leftover ends as SE, 4 = 2 + SE */
    int32_t pair_min_len;   /* -d  minimum insert (default 100)  */
    int32_t pair_max_len;   /* -D  maximum insert (default 1000) */
    int32_t pair_strand;    /* -E  both ends on the same strand  */
} bk_pe_params;
int  bk_pair_batch(bk_ctx *ctx, const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint32_t n_pairs,
                   bk_hit *hits, const bk_pe_params *pe);
/* the same on buffers already resident in HBM on the context's GPU (d_hits = what bk_align_batch_device wrote
 * for exactly these reads); nothing crosses PCIe */
int  bk_pair_batch_device(bk_ctx *ctx, const void *d_bases, const void *d_offs, const void *d_lens, uint32_t n_pairs,
                          void *d_hits, const bk_pe_params *pe);
/* The same with the reads' bk_seg2 records (2 * n_pairs, what bk_batch_seg2() returned for exactly these reads; see below), updated in
 * place.  Required on a context with min_chimeric_len > 0 (`-c` together with `-U`; BK_ERR_PARAMS without them): ProcessPairedEnds then
 * measures inserts between the trimmed ends (AdjStartLoci / AdjEndLoci, Aligner.cpp:1528-1544) and AlignPairedRead may place the orphan's
 * partner end-trimmed down to min_chimeric_len percent of its length (MinPutLen, SfxArrayV2.cpp:8327-8330), taking the longest trimmed
 * stretch, then the fewest mismatches, first in scan order; a recovered partner's record is replaced as a whole - flags = FlgChimeric
 * with its trims, or 0 (whatever second segment it had is gone).  A pipeline created with pe != NULL does this by itself. */
struct bk_seg2;
int  bk_pair_batch_seg2(bk_ctx *ctx, const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint32_t n_pairs,
                        bk_hit *hits, struct bk_seg2 *seg2, const bk_pe_params *pe);
int  bk_pair_batch_seg2_device(bk_ctx *ctx, const void *d_bases, const void *d_offs, const void *d_lens, uint32_t n_pairs,
                               void *d_hits, void *d_seg2, const bk_pe_params *pe);

/* ---- multi-loci modes (-r1..-r5: AlignReads called with MaxHits = -R > 1) ---------------------- */
/* One locus of a read that aligned to 1..MaxHits places with the same, lowest, number of mismatches: the
 * Seg[0] fields of the tsHitLoci entries LocateCoreMultiples leaves in pHits[] (SfxArrayV2.cpp:6157-6205),
 * in the reference's discovery order ('+' strand first, cores in order, suffix-array order within a core) -
 * the order `-r5` reports them in and `-r2` indexes with rand() (Aligner.cpp:9337-9366).  12 bytes. */
#define BK_MAX_ML 32766
typedef struct bk_loci {
    uint32_t chrom_id;           /* Seg[0].ChromID                  */
    uint32_t match_loci;         /* Seg[0].MatchLoci                */
    uint16_t match_len;          /* Seg[0].MatchLen                 */
    uint8_t  strand;             /* '+' or '-'                      */
    uint8_t  mismatches;         /* Seg[0].Mismatches               */
} bk_loci;
/* Loci lists of the reads of the LAST bk_align_batch()/bk_align_batch_device() call on a context created
 * with max_ml > 1: read r owns loci[offs[r] .. offs[r+1]), that is LowHitInstances entries when its
 * bk_hit.rslt is eHRhits (1 for a unique read, whose record it repeats), max_ml entries when it is eHRHitInsts
 * and clamp_ml is set, and none otherwise.  The pointers
 * are host memory owned by the context, valid until its next align call.  With max_ml == 1 there are no
 * lists (*n_loci = 0, NULL pointers).  What to do with them (-r1 statistics, -r2 random pick, -r3/-r4
 * clustering, -r5 report all; Aligner.cpp:9328-9424,5105-5272) is host policy above this boundary. */
int  bk_batch_loci(bk_ctx *ctx, const uint64_t **offs, const bk_loci **loci, uint64_t *n_loci);
/* With min_chimeric_len > 0 as well (`-c` together with `-r1..5`): the chimeric LocateCoreMultiples call is made with MaxHits = max_ml
 * too and every locus it returns keeps its own end trims (tsSegLoci.TrimLeft / TrimRight of a FlgChimeric hit, read orientation,
 * SfxArrayV2.cpp:6027-6070).  One entry per locus of bk_batch_loci(), in the same order; all zero for loci of the ordinary calls.
 * NULL / 0 on other contexts.  6 bytes. */
typedef struct bk_loci_trims {
    uint16_t left, right;        /* Seg[0].TrimLeft / TrimRight                                  */
    uint8_t  chimeric;           /* FlgChimeric                                                  */
    uint8_t  reserved;
} bk_loci_trims;
int  bk_batch_loci_trims(bk_ctx *ctx, const bk_loci_trims **trims, uint64_t *n_loci);

/* ---- microInDels (-a) ---------------------------------------------------------------------- */
/* Second segment of a read aligned with a microInDel (tsHitLoci.Seg[1] and flags, SfxArrayV2.h:219-240): the read's bk_hit holds
 * the first segment (match_loci / match_len / mismatches of Seg[0]; low_mm = mismatches of both, nxt_low_mm = low_mm + 2 as
 * LocateInDels returns them, SfxArrayV2.cpp:7655-7657).  12 bytes. */
typedef struct bk_seg2 {
    uint32_t match_loci;         /* Seg[1].MatchLoci, 0-based within the entry of Seg[0]          */
    uint16_t match_len;          /* Seg[1].MatchLen                                               */
    uint16_t read_ofs;           /* Seg[1].ReadOfs: first read base of the second segment        */
    uint8_t  mismatches;         /* Seg[1].Mismatches                                             */
    uint8_t  flags;              /* bit 0 FlgInDel, bit 1 FlgInsert (gap is in the read), bit 2 FlgSplice; bit 3 FlgChimeric: no second segment,
                                  * match_len = Seg[0].TrimLeft, read_ofs = Seg[0].TrimRight (read orientation); 0 = plain hit */
    uint16_t score;              /* tsHitLoci.Score                                               */
} bk_seg2;
/* One entry per read of the LAST align call on a context created with micro_indel_len > 0 (host memory owned by the context,
 * valid until its next align call; NULL / 0 otherwise).  Orphan removal (CAligner::RemoveOrphanMicroInDels, Aligner.cpp:2382-2470)
 * is host policy above this boundary. */
int  bk_batch_seg2(bk_ctx *ctx, const bk_seg2 **seg2, uint64_t *n);

/* ---- overlapped pipeline: host buffers in -> host results out ---------------------------------------------------
 * Batch form of the reference's loader-thread / aligner-threads overlap (CAligner::LoadReads + ThreadedIterReads,
 * biokanga/Aligner.cpp:4820-4860,9636-9704): batch k+1 crosses PCIe while batch k runs through the AlignReads phases
 * and the results of batch k-1 travel back, on three HIP streams driven by three host threads owned by the stream
 * object.  T_align of the metric (first batch submitted -> last result back) is what bk_stream_get_stats() reports.
 * While a stream exists the context's own align / pair / loci / seg2 calls must not be used from other threads. */
typedef struct bk_stream bk_stream;
typedef struct bk_stream_stats {
    uint64_t batches, reads;
    uint64_t bytes_h2d, bytes_d2h;                      /* what crossed PCIe */
    double   seconds_first_submit_to_last_result;       /* T_align of the batches since the last reset */
} bk_stream_stats;
/* page-locked host memory (hipHostMalloc): buffers the stream DMAs from / to directly.  Pageable buffers are accepted
 * too and are staged by the HIP runtime (slower). */
void *bk_host_alloc(size_t bytes);
void  bk_host_free(void *p);
/* .. or memory the caller already owns, page-locked in place (hipHostRegister) for as long as results or reads travel through it:
 * what the command line does with its result array.  0 or a negative code; unregister before the memory is freed. */
int   bk_host_register(void *p, size_t bytes);
void  bk_host_unregister(void *p);
/* depth = sets of device buffers (2..4 is useful: one uploading, one aligning, one downloading); every batch may hold up to
 * max_batch_reads reads in max_batch_bases bytes.  pe != NULL: batches hold whole pairs interleaved PE1, PE2 and the
 * paired-end association (bk_pair_batch_device) runs on the resident buffers right after the SE pass. */
int  bk_stream_create(bk_stream **out, bk_ctx *ctx, uint32_t max_batch_reads, uint64_t max_batch_bases, int depth, const bk_pe_params *pe);
/* The same for a caller that only submits packed batches (bk_stream_submit_packed) of at most max_batch_words 32-bit words: the device
 * buffers hold 4 bytes per 16 bases instead of 16, a quarter of the memory (and of the allocation time) of the general form.
 * bk_stream_submit() on such a pipeline is refused. */
int  bk_stream_create_packed(bk_stream **out, bk_ctx *ctx, uint32_t max_batch_reads, uint64_t max_batch_words, int depth, const bk_pe_params *pe);
/* bases[0 .. nbases) holds the reads of this batch, 1 byte/base as CAligner holds them; offs[i] = start of read i within
 * bases, or offs == NULL when the reads lie back to back in lens order (the offsets are then computed on the device and
 * 8 bytes per read stay off PCIe); out[nreads].  Returns once the batch is queued (it blocks only while all `depth`
 * buffer sets are busy); every buffer must stay valid and untouched until bk_stream_wait(ticket) has returned. */
int  bk_stream_submit(bk_stream *s, const uint8_t *bases, uint64_t nbases, const uint64_t *offs, const uint32_t *lens, uint32_t nreads,
                      bk_hit *out, uint64_t *ticket);
/* the same with the batch in the packed form (see bk_align_batch_packed) */
int  bk_stream_submit_packed(bk_stream *s, const uint32_t *words, uint64_t n_words, const uint16_t *lens, uint32_t nreads,
                             const bk_nbase *exc, uint64_t n_exc, bk_hit *out, uint64_t *ticket);
/* blocks until the results of that batch are in its `out`; returns the batch's result code (each ticket once, unless the
 * context runs a list mode - then bk_stream_batch_loci / _seg2 stay available until bk_stream_release) */
/* Device-resident, asynchronous form of bk_align_batch_device (+ bk_pair_batch_device on a pipeline with pe): reads and result
 * buffer already in HBM on the context's GPU.  The call records a point on `producer_stream` (a hipStream_t, NULL = the default stream)
 * and returns; the batch is aligned, in submission order with the pipeline's other batches, once everything enqueued on that stream
 * before the call has run - the caller's thread never waits for the phase loop (CAligner's loader || workers overlap, Aligner.cpp:4820-4860,
 * for a producer that is itself device code).  d_hits is complete, visible to every stream, when bk_stream_wait(ticket) has returned; the
 * buffers must stay untouched until then.  No size limit other than the context's own. */
int  bk_stream_submit_device(bk_stream *s, const void *d_bases, const void *d_offs, const void *d_lens, uint32_t nreads, void *d_hits,
                             void *producer_stream, uint64_t *ticket);
int  bk_stream_wait(bk_stream *s, uint64_t ticket);
int  bk_stream_batch_loci(bk_stream *s, uint64_t ticket, const uint64_t **offs, const bk_loci **loci, uint64_t *n_loci);
int  bk_stream_batch_seg2(bk_stream *s, uint64_t ticket, const bk_seg2 **seg2, uint64_t *n);
int  bk_stream_batch_loci_trims(bk_stream *s, uint64_t ticket, const bk_loci_trims **trims, uint64_t *n_loci);
int  bk_stream_release(bk_stream *s, uint64_t ticket);
/* waits for everything submitted; first failing batch's code or BK_OK */
int  bk_stream_drain(bk_stream *s);
int  bk_stream_get_stats(bk_stream *s, bk_stream_stats *out, int reset);
void bk_stream_destroy(bk_stream *s);

/* counters/timing accumulated since the last reset */
int  bk_get_counters(bk_ctx *ctx, bk_counters *out, int reset);
int  bk_get_timing(bk_ctx *ctx, bk_timing *out, int reset);

/* per-sequence count of accepted reads since the last reset (CAligner::ReportTargHitCnts,
 * Aligner.cpp:5475-5537) - the vector the multi-GPU run sum-reduces over RCCL.  n = bk_num_entries */
int  bk_seq_counts(bk_ctx *ctx, uint64_t *per_entry_hits, uint32_t n, int reset);
/* The path's one exchange step (what CAligner::ReportTargHitCnts and the "@SQ has hits" decision of
 * Aligner.cpp:5475-5537,5606-5637 see on a single host): the count vectors of the `n` contexts of one process - one context per
 * GPU, each fed its own shard of the reads - are sum-reduced where they lie in HBM, with RCCL (ncclAllReduce over xGMI) between
 * distinct devices; contexts sharing a device are added up there first.  `out` (n_entries values, may be NULL) receives the
 * total; reset != 0 then clears the per-context counts.  Multi-process runs reduce bk_seq_counts() through their own
 * communicator instead (bench.py: torch.distributed / RCCL). */
int  bk_seq_counts_allreduce(bk_ctx *const *ctxs, int n, uint64_t *out, uint32_t n_entries, int reset);

/* ---- SNP calling (-p / -P / -1 / -S) --------------------------------------------------------- */
/* The pile-up and the per-locus screening of CAligner::ProcessSNPs (biokanga/Aligner.cpp:7737-7960) and of the first
 * loop of CAligner::OutputSNPs (:6880-7110) on the GPU: per-locus counts of reference / non-reference read bases live
 * in HBM (6 x uint32 per target base), reads are piled up with atomic adds, and only the loci that qualify as putative
 * SNPs travel back.  P-values (CStats::Binomial), the Benjamini-Hochberg cut and the CSV/BED/VCF writers are host
 * policy above this boundary (biokanga_amd/csrc/host/snp.cpp). */
typedef struct bk_snp_aln {      /* one accepted alignment without InDel/splice, after every host filter */
    uint32_t read_idx;           /* read of this call the alignment belongs to                              */
    uint32_t chrom_id;           /* Seg[0].ChromID                                                          */
    uint32_t loci;               /* AdjStartLoci(Seg[0])  (Aligner.cpp:1528)                                */
    uint16_t len;                /* AdjHitLen(Seg[0])     (Aligner.cpp:1546)                                */
    uint16_t read_ofs;           /* Seg[0].ReadOfs + TrimLeft: first read base of the aligned part          */
    uint8_t  strand;             /* '+' | '-' : '-' piles up the reverse complement of those read bases     */
    uint8_t  reserved[3];
} bk_snp_aln;                    /* 20 bytes */
typedef struct bk_snp_site {     /* a locus passing the coverage / non-reference proportion screen (:6932-6960) */
    uint32_t loci;
    uint32_t num_ref;            /* tsSNPcnts.NumRefBases                                                   */
    uint32_t non_ref[5];         /* tsSNPcnts.NonRefBaseCnts a,c,g,t,n (their sum = NumNonRefBases)         */
    uint32_t win_mismatches;     /* LocalTotMismatches of the 51 base background window at this locus       */
    uint32_t win_matches;        /* LocalTotMatches                                                         */
    uint32_t ref_base;           /* tsSNPcnts.RefBase 0..3                                                  */
} bk_snp_site;                   /* 40 bytes */
typedef struct bk_snp_chrom {    /* whole-sequence totals OutputSNPs needs (:6881, :6927-6931) */
    uint64_t tot_match, tot_mismatch;        /* tsChromSNPs.TotMatch / TotMismatch                          */
    uint64_t loci_covered, bases_coverage;   /* contribution to m_LociBasesCovered / m_LociBasesCoverage    */
} bk_snp_chrom;
/* allocate (first call) and zero the per-locus counts */
int  bk_snp_reset(bk_ctx *ctx);
/* pile up `n_alns` alignments of the `nreads` host-resident reads; may be called any number of times */
int  bk_snp_pileup(bk_ctx *ctx, const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint32_t nreads,
                   const bk_snp_aln *alns, uint64_t n_alns);
/* the same on reads already resident in HBM on the context's GPU (e.g. the buffers bk_align_batch_device was given) and a device
 * array of alignments; asynchronous on the context's stream unless `sync`.  The caller guarantees what bk_snp_pileup checks:
 * read_idx < nreads, read_ofs + len within the read, chrom_id a sequence of the index */
int  bk_snp_pileup_device(bk_ctx *ctx, const void *d_bases, const void *d_offs, uint32_t nreads, const void *d_alns, uint64_t n_alns, int sync);
/* screen sequence `chrom_id`: loci covered by >= min_reads bases of which >= 1 and a proportion >= min_nonref_prop differ
 * from the target, in ascending loci order (host memory owned by the context, valid until its next call) */
int  bk_snp_sites(bk_ctx *ctx, uint32_t chrom_id, int32_t min_reads, double min_nonref_prop,
                  const bk_snp_site **sites, uint64_t *n_sites, bk_snp_chrom *totals);
/* the counts of `n` consecutive loci of sequence `chrom_id` from `loci` on, 7 uint32 per locus: NumRefBases, NonRefBaseCnts a,c,g,t,n and
 * the target base - what the marker sequences of `-K` are assembled from (OutputSNPs, Aligner.cpp:7006-7086) */
int  bk_snp_counts(bk_ctx *ctx, uint32_t chrom_id, uint32_t loci, uint32_t n, uint32_t *out);
/* SNP centroids (`-7 <file>`): adds, for every locus of sequence `chrom_id` covered by >= min_reads bases and at least 3 bases away from
 * both ends, one to num_insts[k], k = the 7 target bases centred on the locus as a base-4 number (first base most significant; loci with a
 * non-ACGT base in the window are skipped) - tsSNPCentroid.NumInsts of OutputSNPs (Aligner.cpp:6934-6953).  num_insts: 16384 uint32. */
#define BK_SNP_CENTROIDS 16384
int  bk_snp_centroid_insts(bk_ctx *ctx, uint32_t chrom_id, int32_t min_reads, uint32_t *num_insts);

/* ---- start-site octamer preferences (-8 / -9) --------------------------------------------------- */
/* The gather of CAligner::ProcessSiteProbabilites (biokanga/Aligner.cpp:8121-8172) on the GPU: for every alignment the eight target
 * bases at its start site - MatchLoci + rel_ofs for '+', MatchLoci + MatchLen - 1 - rel_ofs - 7 for '-', in the reference's 32-bit
 * unsigned arithmetic, then its end clamp (site + 8 >= sequence length: site = length - 9) - from the 4-bit target resident in HBM.
 * For '-' the eight bases are reverse-complemented.  The sequential rest of that routine (PrevLoci, the counts, the scaling, the
 * writer) is host policy above this boundary (biokanga_amd/csrc/host/site_prefs.h). */
typedef struct bk_site_req {     /* one alignment: Seg[0] as it stands */
    uint32_t chrom_id;           /* Seg[0].ChromID                                                          */
    uint32_t match_loci;         /* Seg[0].MatchLoci                                                        */
    uint16_t match_len;          /* Seg[0].MatchLen                                                         */
    uint8_t  strand;             /* '+' | '-'                                                               */
    uint8_t  reserved;
} bk_site_req;                   /* 12 bytes */
typedef struct bk_site_res {
    uint32_t codes;              /* eight 3-bit base codes in buffer order, the first in bits 23..21, the last in bits 2..0 (all of
                                  * them < 4: codes is the octamer's index); bit 31: the site lies outside the sequence, nothing fetched */
    uint32_t site;               /* the site (HitLoci) after the clamp                                      */
} bk_site_res;                   /* 8 bytes */
#define BK_SITE_MAX_OFS 100      /* cMaxSitePrefOfs */
/* host arrays, blocking; staged through buffers of the context in chunks.  BK_ERR_PARAMS before anything is launched: |rel_ofs| >
 * BK_SITE_MAX_OFS, a chrom_id that is no sequence of the index, a strand other than '+' / '-' */
int  bk_site_octamers(bk_ctx *ctx, const bk_site_req *reqs, uint64_t n, int32_t rel_ofs, bk_site_res *out);
/* the same HBM to HBM on the context's GPU (d_out 8-byte aligned); asynchronous on the context's stream unless `sync`.  The caller
 * guarantees the requests (one whose chrom_id is no sequence of the index comes back as "nothing fetched") */
int  bk_site_octamers_device(bk_ctx *ctx, const void *d_reqs, uint64_t n, int32_t rel_ofs, void *d_out, int sync);

/* ---- 5' primer artefact correction (-6) ----------------------------------------------------------- */
/* The per-read half of CAligner::PCR5PrimerCorrect (biokanga/Aligner.cpp:2052-2088) on the GPU: the first BK_PRIMER_KLEN bases of a
 * read as loaded against the target it aligned to - the target's bases from MatchLoci for '+'; for '-' the last BK_PRIMER_KLEN bases
 * of the match, reversed, codes 0..3 complemented - from the 4-bit target resident in HBM.  Mismatches (read code & 7 against what
 * GetSeq answers; the indexer cleared the FASTA's lower-case flag, so that is 0..4) are corrected left to right until the count is
 * down to max_mms; a read that cannot get there is rejected.  Which records are asked about, and what becomes of the answers, is host
 * policy above this boundary (biokanga_amd/csrc/host/primer_correct.h). */
#define BK_PRIMER_KLEN 12        /* KLen of PCR5PrimerCorrect (Aligner.h:782) */
typedef struct bk_primer_req {
    uint64_t codes;              /* the read's first 12 base codes (& 7), 3 bits each, the first in bits 35..33, the last in bits 2..0 */
    uint32_t chrom_id;           /* Seg[0].ChromID                                                          */
    uint32_t match_loci;         /* Seg[0].MatchLoci                                                        */
    uint16_t match_len;          /* Seg[0].MatchLen (= the read's length), >= BK_PRIMER_KLEN                 */
    uint8_t  strand;             /* '+' | '-'                                                               */
    uint8_t  low_mm;             /* LowMMCnt                                                                */
    uint8_t  max_mms;            /* (rate * ReadLen + 50) / 100                                             */
    uint8_t  reserved[3];
} bk_primer_req;                 /* 24 bytes */
enum { BK_PRIMER_UNTOUCHED = 0, BK_PRIMER_CORRECTED = 1, BK_PRIMER_REJECTED = 2, BK_PRIMER_BAD = 0x80 };
typedef struct bk_primer_res {
    uint64_t codes;              /* the 12 codes afterwards, laid out as in the request (corrected ones hold the target's code) */
    uint16_t mask;               /* corrected positions: bit k = base k of the read                         */
    uint8_t  status;             /* BK_PRIMER_*; BK_PRIMER_BAD: no such sequence or a window outside it, nothing fetched */
    uint8_t  mismatches;         /* the new LowMMCnt (the request's where nothing was corrected)            */
    uint8_t  n_corrected;        /* bases corrected                                                         */
    uint8_t  reserved[3];
} bk_primer_res;                 /* 16 bytes */
/* host arrays, blocking; staged through buffers of the context in chunks (made by the first call: a run without -6 allocates nothing).
 * BK_ERR_PARAMS before anything is launched: a chrom_id that is no sequence of the index, a strand other than '+' / '-',
 * match_len < BK_PRIMER_KLEN, a match that leaves its sequence.  n == 0 launches nothing */
int  bk_primer_correct(bk_ctx *ctx, const bk_primer_req *reqs, uint64_t n, bk_primer_res *out);
/* the same HBM to HBM on the context's GPU (d_reqs 8-byte, d_out 16-byte aligned); asynchronous on the context's stream unless `sync`.
 * The caller guarantees the requests (a bad one comes back BK_PRIMER_BAD, nothing fetched) */
int  bk_primer_correct_device(bk_ctx *ctx, const void *d_reqs, uint64_t n, void *d_out, int sync);

/* ---- loci base constraints (-5) -------------------------------------------------------------------- */
/* CAligner::IdentifyConstraintViolations' per-record half (AcceptLociConstraints / AcceptBaseConstraint, biokanga/Aligner.cpp:2480-2595)
 * on the GPU: "reads aligned over lcA:100 are only accepted if they carry C or T there".  A constraint names a sequence, an inclusive
 * range of loci and the bases allowed there: bits 0..3 = A C G T, bit 4 = R, "the read's base equals the target's".  A record is
 * walked base by base over its one or two aligned segments, the read `& 7` and reverse-complemented as a whole for '-'; it violates
 * when ANY constraint that covers a walked locus allows neither the base's bit nor (with R) equality with the target's base.  A read N
 * has no bit; it equals a target N under R.  The limits are the reference's (Aligner.h:74-75).  Which records are asked about and what
 * becomes of the answers is host policy above this boundary (biokanga_amd/csrc/host/loci_constraints.h). */
#define BK_MAX_CONSTRAINED_SEQS 64
#define BK_MAX_CONSTRAINTS      6400
#define BK_CONSTRAINT_R         0x10
typedef struct bk_constraint {
    uint32_t chrom_id;           /* EntryID of the constrained sequence                                     */
    uint32_t start, end;         /* first and last constrained locus, 0-based, start <= end < the sequence's length */
    uint8_t  mask;               /* 1 A | 2 C | 4 G | 8 T | BK_CONSTRAINT_R; not 0                           */
    uint8_t  reserved[3];
} bk_constraint;                 /* 16 bytes */
typedef struct bk_constraint_seg {
    uint32_t start;              /* AdjStartLoci of the segment                                             */
    uint16_t len;                /* its loci (AdjEndLoci - AdjStartLoci + 1); 0: nothing walked             */
    uint16_t read_idx;           /* ReadOfs + TrimLeft: index of the first locus' base in the read as aligned */
} bk_constraint_seg;             /* 8 bytes */
typedef struct bk_constraint_req {
    uint64_t read_ofs;           /* the read's first base in `bases` (a byte per base, code in the low three bits) */
    uint32_t chrom_id;           /* Seg[0].ChromID - both segments are walked on it                         */
    uint16_t read_len;           /* ReadLen                                                                 */
    uint8_t  strand;             /* '+' | '-'                                                               */
    uint8_t  n_segs;             /* 1, or 2 with FlagSegs                                                   */
    bk_constraint_seg seg[2];
} bk_constraint_req;             /* 32 bytes */
/* one status byte per request; BAD: nothing was read for it - no such sequence, a strand other than '+' / '-', n_segs not 1 | 2, a
 * segment that leaves its sequence or its read, a read outside `bases` */
enum { BK_CONSTRAINT_UNTOUCHED = 0, BK_CONSTRAINT_TOUCHED = 1, BK_CONSTRAINT_VIOLATED = 2, BK_CONSTRAINT_BAD = 0x80 };
typedef struct bk_constraints bk_constraints;
/* The constraints of a run on the context's GPU: sorted by (sequence, start, end) with a slice per sequence and the running maximum of
 * `end` inside each, about 100 KB at most.  BK_ERR_PARAMS: n > BK_MAX_CONSTRAINTS, more than BK_MAX_CONSTRAINED_SEQS sequences, a
 * chrom_id that is no sequence of the index, start > end, end outside the sequence, a mask of 0 or with bits above BK_CONSTRAINT_R.
 * n == 0 is a set that touches nothing.  The set must be destroyed before its context. */
int  bk_constraints_create(bk_ctx *ctx, const bk_constraint *constraints, uint32_t n, bk_constraints **out);
void bk_constraints_destroy(bk_constraints *set);
/* host arrays, blocking, in chunks of "constraint_chunk" requests: the requests travel to the device, k_constraint_touch (one lane
 * per request, geometry only) answers UNTOUCHED / BAD and lists the requests whose segments overlap a constraint, the host gathers the
 * bases of those reads alone into page-locked staging, k_constraint_check (one wave per listed request) walks them.  The staging is
 * made by the first call that has requests.  counts[4]: requests UNTOUCHED, TOUCHED (and accepted), VIOLATED, BAD - may be NULL.
 * n_bases: the bytes of `bases`. */
int  bk_constraints_check(bk_constraints *set, const bk_constraint_req *reqs, uint64_t n, const uint8_t *bases, uint64_t n_bases,
                          uint8_t *status_out, uint64_t counts[4]);

/* ---- SAM records formatted on the device -------------------------------------------------------------------------
 * CAligner::ReportBAMread (biokanga/Aligner.cpp:5768-6126; CSAMfile::AddAlignment, SAMfile.cpp:2100-2283) prints one text line per
 * read; for tens of millions of reads that is byte-parallel work.  bk_sam_format() takes the reads, their names, their records and
 * the order the lines are wanted in (the reference's sort order is the host's business) and hands the lines back as text, in
 * slices: a lane per record measures its line, a prefix sum places it, the lane writes it.  With pe_mode the reads are interleaved
 * PE1, PE2 and carry the flags bk_pair_batch left.
 * The sink is called once per slice with the slice's text and its offset within the whole text; up to two calls may run at the
 * same time (on threads of the library), each must return 0.  Lines are those of the reference's SAM body, byte for byte.
 *
 * Two index spaces.  A READ is an entry of the read store; a RECORD is one line to write.  Without `src` they are the same thing:
 * record i is read i, and n_reads counts both.  With `src` (-r5: a read owns a record per reported locus) n_reads counts the
 * RECORDS and n_src_reads the reads; record i belongs to read src[i].
 *   by read:   bases / offs / lens, names / name_ofs, pk_*, seg2 and the head start (`prep`, given the reads alone)
 *   by record: hits, the entries of order, trim_left / trim_right, src, dup, xs
 * What a record may carry besides its bk_hit:
 *   dup                    - the verdict of bk_mark_duplicates (below): FLAG |= 0x400 on an accepted record, nothing else moves;
 *   xs                     - the strand answer of bk_junctions (below): '+' or '-' appends XS:A:<c> to an accepted record's line, behind
 *                            NM / MD where bk_sam_format_tags writes those; any other byte, and every unaccepted line: nothing;
 *   trim_left / trim_right - end trims in read orientation (-x, -A, -c: tsSegLoci.TrimLeft / TrimRight): POS moves to AdjStartLoci,
 *                            the M run shrinks to AdjHitLen and the trimmed ends are written as soft clips, swapped on the '-' strand;
 *   seg2 of its read       - a second segment (flags & 5: microInDel or splice junction) adds <gap>N, <n>I or <gap>D and <len2>M
 *                            to the CIGAR, as CAligner::ReportBAMread does (Aligner.cpp:5986-6033).  Flag bit 3 (chimeric trims
 *                            travelling in match_len / read_ofs) is NOT read here: hand those over in trim_left / trim_right.
 * In a paired record PNEXT and TLEN come from the mate's trimmed start and length.  `src` together with pe_mode is BK_ERR_PARAMS
 * (the reference refuses -r with -U). */
struct bk_sam_prep;
typedef struct bk_sam_job {
    const uint8_t  *bases;        /* all reads, 1 byte/base as CAligner holds them (quality in bits 4-7 when loaded)      */
    uint64_t        n_bases;
    const uint64_t *offs;         /* n_reads: start of read i in bases                                                     */
    const uint32_t *lens;         /* n_reads                                                                               */
    const char     *names;        /* the reads' names, NUL-terminated, back to back in read order                          */
    uint64_t        n_name_bytes;
    const uint64_t *name_ofs;     /* n_reads: start of name i in names                                                     */
    const bk_hit   *hits;         /* n_reads records                                                                       */
    uint64_t        n_reads;      /* reads = records; with `src`: records (the reads are n_src_reads)                      */
    const uint32_t *order;        /* n_order record numbers: the lines in output order                                     */
    uint64_t        n_order;
    int32_t         report_unaligned;   /* -M6: reads without an accepted alignment get a line too (FLAG 4, YU:Z:<reason>) */
    int32_t         pe_mode;            /* 0, or the -U mode the records were paired under                                 */
    struct bk_sam_prep *prep;           /* NULL, or what bk_sam_prepare() started for exactly these reads (consumed by the call)   */
    /* The reads in the packed form of bk_pack_reads instead of bases / offs / lens (those may then be NULL; QUAL is '*'): all reads'
     * words back to back in read order, their 16-bit lengths, and the exceptions with `read` counting from the job's first read.
     * A 100-base read then travels as 30 bytes instead of 112 - from the buffers the alignment was fed from, when those are still there. */
    const uint32_t *pk_words;
    uint64_t        n_pk_words;
    const uint16_t *pk_lens16;
    const bk_nbase *pk_exc;
    uint64_t        n_pk_exc;
    /* (all NULL / 0 in a job of plain records: one segment, no end trims, a record per read) */
    const uint32_t *src;          /* NULL, or n_reads entries: record -> read                                              */
    uint64_t        n_src_reads;  /* with `src`: reads in the read store (ignored without)                                 */
    const bk_seg2  *seg2;         /* NULL, or one per READ, as bk_batch_seg2() returns them                                */
    const uint16_t *trim_left;    /* NULL (both), or one per RECORD, read orientation                                      */
    const uint16_t *trim_right;
    const uint8_t  *dup;          /* NULL, or one per RECORD (--mark-duplicates): non-zero adds 0x400 to the FLAG of an accepted record */
    const uint8_t  *xs;           /* NULL, or one per RECORD (--splice-strand): '+' or '-' adds \tXS:A:<c> at the end of an accepted record's line */
} bk_sam_job;
/* Optional head start: everything of a job that is known once the reads are aligned - the read store, the names, the buffers the
 * text leaves the device through - can travel while the host still sorts.  bk_sam_prepare() returns at once (a thread of the library
 * does the work; `job`'s bases / offs / lens / names / name_ofs must stay valid until bk_sam_format() or bk_sam_prep_free()), hits and
 * order are not looked at.  text_bytes_per_record: expected length of a line (sizes the pinned text buffers; 0 = let the first slice
 * size them).  Pass the handle in bk_sam_job.prep; a handle that is not used is given back with bk_sam_prep_free(). */
typedef struct bk_sam_prep bk_sam_prep;
int  bk_sam_prepare(bk_ctx *ctx, const bk_sam_job *job, uint32_t text_bytes_per_record, bk_sam_prep **out);
void bk_sam_prep_free(bk_sam_prep *prep);
/* blocks until the head start's transfers are over (the job's read-side arrays may be released then); returns their result code */
int  bk_sam_prep_wait(bk_sam_prep *prep);
typedef int (*bk_sam_sink)(void *user, const char *text, uint64_t n_bytes, uint64_t text_offset);
int  bk_sam_format(bk_ctx *ctx, const bk_sam_job *job, bk_sam_sink sink, void *user, uint64_t *n_reported, uint64_t *n_bytes);

/* ---- NM:i and MD:Z of SAM records (--sam-tags) ----------------------------------------------------------------------
 * The reference writes neither; consumers want both.  The tags are a literal walk of the line as written - what any SAM consumer would
 * compute from it - against the sequence AS INDEXED (codes a c g t n of the .sfx, the lower-case flag gone; the indexer turns every 13th
 * N of a long N run into a random base, so the FASTA may differ):
 *   the record's POS, CIGAR and SEQ (SEQ already reverse complemented for '-'); S and I consume SEQ only, N and D the target only, M
 *   both, base by base.  An M base matches when SEQ's letter equals the target's and is one of ACGT; an N on either side mismatches.
 *   NM:i = mismatching M bases + all I bases + all D bases.
 *   MD:Z = [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*: run lengths always written (0 at either end and between adjacent mismatches), a mismatch
 *   writes the target's letter, D writes ^ and the deleted target letters; N, I and S write nothing and a match run continues across them.
 * A record whose CIGAR is not a well-formed walk - a number <= 0, a walk that does not consume exactly SEQ, or one that leaves its
 * sequence - gets no tags (nor does one whose NM would not fit 16 bits).  The CIGAR is [c5 S] m M [c3 S] [gap N|I|D m2 M], the only
 * shape the writers make. */
#define BK_SAMTAG_NM 1
#define BK_SAMTAG_MD 2
#define BK_SAMTAG_NONE 0xFFFFu     /* the NM answer of a request without tags */
typedef struct bk_samtag_req {
    uint64_t read_ofs;           /* the read's first base in `bases` (a byte per base as loaded, code in the low three bits) */
    uint32_t chrom_id;           /* RNAME's EntryID                                                          */
    uint32_t pos;                /* 0-based position of the first M base in that sequence (POS - 1)         */
    uint16_t read_len;           /* bases of the read = letters of SEQ                                       */
    uint8_t  strand;             /* '+' | '-': for '-' SEQ is the read reverse complemented                  */
    uint8_t  gop;                /* 0: one M run; 'N' | 'I' | 'D': the operation in front of the second       */
    uint16_t c5, m, c3, m2;      /* [c5 S] m M [c3 S] [gap gop m2 M]; m2 is ignored without gop              */
    int32_t  gap;
} bk_samtag_req;                 /* 32 bytes */
/* host arrays, blocking; in chunks of "samtag_chunk" requests through staging the context owns (made by the first call: a run without
 * the option allocates nothing; "samtag_buf_bytes", read only, says what it holds).  nm_out[i] = NM of request i or BK_SAMTAG_NONE;
 * md_ofs[0..n] = where request i's MD text starts in md_text (md_ofs[n] = all of it; a request without tags has none), no terminators.
 * md_ofs == NULL and md_text == NULL: NM alone.  *md_needed (may be NULL) = the bytes of all MD text; when md_cap is smaller the call
 * returns BK_ERR_MEM and has written nothing but *md_needed.  A request whose sequence does not exist, whose read leaves `bases`
 * (n_bases bytes) or whose walk is malformed answers "no tags" for itself only.  BK_ERR_PARAMS, before anything is launched: a NULL
 * array, one of md_ofs / md_text without the other, a strand other than '+' / '-'. */
int  bk_samtags(bk_ctx *ctx, const bk_samtag_req *reqs, uint64_t n, const uint8_t *bases, uint64_t n_bases, uint16_t *nm_out,
                uint64_t *md_ofs, char *md_text, uint64_t md_cap, uint64_t *md_needed);
/* bk_sam_format with the tags of the mask `tags` (BK_SAMTAG_NM | BK_SAMTAG_MD) inside the lines of accepted records:
 * ...QUAL\tNM:i:<n>\tMD:Z:<s>\n, only the tags asked for, NM first; measured in the measuring pass and written in the writing pass of
 * the formatter.  A record without tags (see above) and the lines of unaccepted reads are as bk_sam_format writes them; tags == 0 IS
 * bk_sam_format.  BK_ERR_PARAMS: bits beyond the two. */
int  bk_sam_format_tags(bk_ctx *ctx, const bk_sam_job *job, uint32_t tags, bk_sam_sink sink, void *user, uint64_t *n_reported, uint64_t *n_bytes);

/* ---- per-base depth of the accepted records as a bedGraph (--coverage) ------------------------------------------------
 * Ours, as --sam-tags is: the reference has no such output.  THE RULE: the depth at a target position is the number of accepted
 * records whose line as written has an M base there.  The walk is the one --sam-tags uses, the numbers put_cigar prints -
 * [c5 S] m M [c3 S] [gap N|I|D m2 M] from POS: M counts; S and I touch no target base; N and D skip `gap` target bases without
 * counting them; behind an I the second M run starts where the first ended.  Every record counts on its own - both mates of a
 * pair even where they overlap, every locus of a read under -r5.
 * The output is a bedGraph: one line name<TAB>start<TAB>end<TAB>depth<LF> per maximal run of equal non-zero depth, 0-based,
 * half-open, decimal numbers without padding, sequences in index order, runs by start; no track line, no zero-depth runs (what
 * `bedtools genomecov -bg -split` prints); a run never spans two sequences.
 * On the device: the target is taken in slices of whole sequences (as many as fit "coverage_slice_bases"; a longer sequence
 * gets a slice of its own), one int32 per base; a lane per request adds +1 / -1 at the ends of its M runs, an inclusive sum turns
 * the deltas into depth, the run starts and run ends are counted per tile, placed by a prefix sum and written out
 * "coverage_run_chunk" runs at a time.  bk_coverage_text formats every chunk of runs on the device (a lane per line: measure,
 * prefix sum, write) and hands the text on in pieces of 16 * "coverage_run_chunk" bytes: lines may straddle two sink calls.
 * Requests may come in any order (the answer does not depend on it); in output order neighbouring lanes hit neighbouring words. */
typedef struct bk_cov_req {
    uint32_t chrom_id;           /* the sequence's EntryID                                                    */
    uint32_t pos;                /* 0-based position of the first M base in that sequence                    */
    uint16_t m;                  /* the first M run                                                           */
    uint16_t m2;                 /* the second M run; 0: none                                                 */
    int32_t  gap;                /* target bases between the runs (N, D); 0 behind an I                       */
} bk_cov_req;                    /* 16 bytes */
typedef struct bk_cov_run {
    uint32_t chrom_id;
    uint32_t start, end;         /* 0-based, half-open                                                        */
    uint32_t depth;
} bk_cov_run;                    /* 16 bytes */
typedef struct bk_cov_totals {
    uint64_t runs;               /* runs delivered = lines of the bedGraph                                    */
    uint64_t covered;            /* positions with depth > 0                                                  */
    uint64_t depth_sum;          /* sum of depth over all positions = M bases of the requests that counted   */
    uint64_t max_depth;
    uint64_t flagged;            /* requests flagged (below)                                                  */
} bk_cov_totals;
/* runs[0 .. n_runs) in output order; run_offset = how many were delivered before; must return 0 */
typedef int (*bk_cov_run_sink)(void *user, const bk_cov_run *runs, uint64_t n_runs, uint64_t run_offset);
/* Host requests, blocking, everything on the context's stream; the sinks are called on the caller's thread, one call at a time,
 * with increasing offsets.  Staging belongs to the context and is made by the first call (a run without the option allocates
 * nothing; "coverage_buf_bytes", read only, says what is held).
 * A request is FLAGGED when its sequence does not exist, m is 0, gap is negative or either M run leaves its sequence: it
 * contributes nothing from either run, is counted in totals->flagged and harms no other request.
 * BK_ERR_PARAMS, before anything is launched: reqs == NULL with n > 0, a NULL sink, n >= 2^31.  n == 0 delivers nothing (totals
 * may be NULL).
 * Both calls share every kernel but the formatter's. */
int  bk_coverage_runs(bk_ctx *ctx, const bk_cov_req *reqs, uint64_t n, bk_cov_run_sink sink, void *user, bk_cov_totals *totals);
int  bk_coverage_text(bk_ctx *ctx, const bk_cov_req *reqs, uint64_t n, bk_sam_sink sink, void *user, bk_cov_totals *totals);

/* ---- duplicate marking: FLAG 0x400 (--mark-duplicates) ---------------------------------------------------------------
 * Ours, as --sam-tags and --coverage are: the reference's -k removes reads, keys on start + strand + length and runs for single
 * ends only.  THE RULE.
 * Templates.  The participants are the accepted records (nar == BK_NAR_ACCEPTED, strand '+' or '-') of the FINAL record set, the
 * one the writers see.  A PAIR is one template of two records: under -U, both mates accepted and both carrying bk_hit.flags & 0x80
 * (on the lines as written: FLAG & 1 set, FLAG & 4 and FLAG & 8 clear).  Every other accepted record is a FRAGMENT: single-end
 * runs, orphan ends, ends "treated as SE" under -U3 / -U4.
 * Unclipped 5' position of a record, from the numbers put_cigar writes - the walk of --sam-tags and --coverage: the line is
 * [cL S] m M [cR S] [gap N|I|D m2 M] from POS; p = POS - 1 is the 0-based position of the first M base;
 * span = m + (N or D ? gap : 0) + (second segment ? m2 : 0); strand '+': pos5 = p - cL; strand '-': pos5 = p + span - 1 + cR.
 * pos5 is signed: it may be negative or lie beyond its sequence.
 * Key.  Fragment: (chrom, pos5, strand).  Pair: (chrom, pos5_a, strand_a, pos5_b, strand_b) with the two ends ordered so that
 * (pos5_a, strand_a) <= (pos5_b, strand_b), '+' < '-'; which end is PE1 is no part of the key (F1R2 and F2R1 at the same ends are
 * one molecule).  Pairs and fragments never share a group: Picard's "a fragment at a pair's end is a duplicate" is not part of
 * this version.
 * Keeper.  Within a group of equal keys exactly one template is kept: the one with the highest score - the M bases of its line(s)
 * as written, m + m2, summed over both mates of a pair - ties going to the template whose (first) read was loaded first.  Every
 * other template of the group is a duplicate.  Base qualities are not looked at; the score is the caller's number.
 * Effect.  Every record of a duplicate template gets 0x400 added to FLAG, in SAM and in BAM, and nothing else changes: duplicates
 * stay accepted, keep their place in the sort order, their --sam-tags, and their count in --coverage, the -O statistics, the SNP
 * calls and -8 (depth and SNPs still include duplicates).  Lines of unaccepted reads under -M6 never carry the bit.
 * The verdict reaches the writers as one byte per record (bk_sam_job.dup), not as a bit of bk_hit.flags: the low seven bits of
 * that field are not free - the engine leaves (AlignReads phase << 1) | 1 there, and the phase reaches 32 and more. */
typedef struct bk_dup_req {      /* one per TEMPLATE */
    uint32_t chrom_id;           /* EntryID                                                                   */
    int32_t  pos5;               /* unclipped 5' position of the (first) end                                  */
    int32_t  pos5_mate;          /* pairs: the other end's; ignored for a fragment                            */
    uint8_t  strand;             /* '+' | '-'                                                                 */
    uint8_t  strand_mate;        /* 0: fragment; '+' | '-': pair                                              */
    uint16_t score;
} bk_dup_req;                    /* 16 bytes */
typedef struct bk_dup_totals {
    uint64_t templates;          /* n                                                                         */
    uint64_t groups;             /* distinct keys among the requests that are not flagged                     */
    uint64_t duplicates;         /* templates - flagged - groups                                              */
    uint64_t max_group;          /* templates of the largest group                                            */
    uint64_t flagged;
} bk_dup_totals;
/* Host arrays, blocking, on the context's stream.  out[i]: 0 request i is kept, 1 it is a duplicate, 2 it is flagged.  The library
 * puts a pair's ends into canonical order itself (the caller hands them PE1 first); among equal scores the EARLIER REQUEST wins,
 * so a caller that submits its templates in load order gets the rule's tie-break.  The answer does not depend on how the device
 * schedules the requests.
 * A request is FLAGGED when its sequence does not exist, its strand is not '+' / '-' or its strand_mate is none of 0, '+', '-':
 * it takes part in no group, is counted in totals->flagged and harms no other request.
 * On the device: an open-addressing table of "dup_table_slots" slots of 16 bytes (owner, best, count), linear probing.  A lane per
 * request claims the first empty slot of its probe sequence with a compare-and-swap of its own index, or joins the slot whose
 * owner's FULL key equals its own (never a fingerprint), and there raises best = score << 32 | (0xFFFFFFFF - index) by an atomic
 * maximum; a second pass finds the slot again and keeps the request best names.  The grouping is global: all requests and the
 * table are resident at once - 100 M templates with the derived table take 1.6 GB of requests and 4.3 GB of table - and
 * BK_ERR_MEM says they do not fit.  Staging and table belong to the context and are made by the first call (a run without the
 * option allocates nothing; "dup_buf_bytes", read only, says what is held).
 * BK_ERR_PARAMS, before anything is launched: a NULL array with n > 0, n >= 2^32 - 1, a "dup_table_slots" that is set and is no
 * power of two or is smaller than n.  n == 0 does nothing (totals may be NULL).  The probe loops are bounded by the table's size:
 * a lane that finds neither its group nor an empty slot - which cannot happen - ends the call with BK_ERR_INTERNAL. */
int  bk_mark_duplicates(bk_ctx *ctx, const bk_dup_req *reqs, uint64_t n, uint8_t *out, bk_dup_totals *totals);

/* ---- splice junctions: the junction table and XS:A (--junctions, --splice-strand) ---------------------------------
 * Ours: the reference writes a BED line per spliced read ("<out>.jct") with the READ's strand and no optional field.  THE RULE.
 * Requests.  A junction request comes from an accepted record of the FINAL record set whose line as written has an N: the line is
 * [c5 S] m M [c3 S] gap N m2 M from POS.  start = POS - 1 + m, 0-based, the first intron base; end = start + gap, one past the
 * last intron base; overhang = min(m, m2); chrom_id = the EntryID of RNAME.
 * Motif of (sequence, start, end), from the sequence AS INDEXED (the codes a c g t n of the 4-bit target, nibble & 7, case gone),
 * d = the bases at start and start + 1, a = the bases at end - 2 and end - 1:
 *     1  GT..AG  +        2  CT..AC  -        3  GC..AG  +        4  CT..GC  -        5  AT..AC  +        6  GT..AT  -
 *     0  anything else, any n, or end - start < 4: no strand
 * The read's own strand plays no part.
 * Junction table.  Requests with equal (chrom_id, start, end) are one junction; it carries `reads`, the number of its requests,
 * `max_overhang`, the largest overhang among them, its motif and its strand ('+', '-' or '.').  Junctions leave the library sorted by
 * (sequence in INDEX order, start, end): the keys are unique, so the order is total and depends neither on how the device schedules
 * the requests nor on their order.
 * Flagged requests.  A request whose sequence does not exist, whose start is 0, whose end is <= start or >= the sequence's length, or
 * whose overhang is 0 is FLAGGED: its strand answer is 0, it counts in no junction and changes nothing for the other requests. */
typedef struct bk_junction_req {
    uint32_t chrom_id;           /* EntryID                                                                   */
    uint32_t start;              /* first intron base, 0-based                                                */
    uint32_t end;                /* one past the last intron base                                             */
    uint16_t overhang;           /* min(m, m2) of the line                                                    */
    uint16_t reserved;
} bk_junction_req;               /* 16 bytes */
typedef struct bk_junction {
    uint32_t chrom_id, start, end;
    uint32_t reads;              /* requests of this junction                                                 */
    uint16_t max_overhang;
    uint8_t  motif;              /* 0..6                                                                      */
    uint8_t  strand;             /* '+', '-' or '.'                                                           */
} bk_junction;                   /* 20 bytes */
typedef struct bk_junction_totals {
    uint64_t requests;           /* n                                                                         */
    uint64_t junctions;          /* distinct keys among the requests that are not flagged                     */
    uint64_t flagged;
    uint64_t max_reads;          /* requests of the junction that has most                                    */
    uint64_t by_motif[7];        /* junctions of motif 0..6                                                   */
} bk_junction_totals;
/* Host arrays, blocking, on the context's stream.  strand_out (n bytes, may be NULL): '+' or '-', the strand of request i's junction,
 * or 0 - its motif is 0, or the request is flagged.  out / cap: room for the table; *n_junctions (may be NULL) is the number of
 * junctions.  out == NULL with cap == 0 asks for strands and totals alone.  When cap is smaller than the junction count the call returns
 * BK_ERR_MEM with *n_junctions set and nothing else written, to be repeated with a larger array (n always suffices).
 * On the device: an open-addressing table of "junction_table_slots" slots of 16 bytes (owner, count, overhang, motif), linear probing.
 * A lane per request claims the first empty slot of its probe sequence with a compare-and-swap of its own index, or joins the slot
 * whose owner's FULL key equals its own, and there adds itself and raises the overhang by an atomic maximum.  Behind the kernel
 * boundary only the owner of a slot reads the target - two dinucleotides per junction, not per read - writes the motif into the slot
 * and emits the junction; a third pass hands every request its slot's strand.  The emitted junctions are ordered by two stable radix
 * sorts (on end, then on entry index << 32 | start) and gathered; the requests are never sorted.  All requests, the table and the
 * emitted junctions are resident at once: 53 bytes per request, 16 per slot and 48 per junction for the sorts.  Staging and table belong to the context and are made
 * by the first call (a run without the options allocates nothing; "junction_buf_bytes", read only, says what is held).
 * BK_ERR_PARAMS, before anything is launched: a NULL context, NULL reqs with n > 0, n >= 2^32 - 1, out == NULL with cap > 0, a
 * "junction_table_slots" that is set and is no power of two or is smaller than n.  n == 0 does nothing (totals, when given, are
 * zeroed).  The probe loops are bounded by the table's size: a lane that finds neither its junction nor an empty slot - which cannot
 * happen - ends the call with BK_ERR_INTERNAL. */
int  bk_junctions(bk_ctx *ctx, const bk_junction_req *reqs, uint64_t n, uint8_t *strand_out, bk_junction *out, uint64_t cap, uint64_t *n_junctions,
                  bk_junction_totals *totals);

/* ---- test hook: the search stage on its own ------------------------------------------------------------------------
 * LocateFirstExact / LocateLastExact (SfxArrayV2.cpp:7765-7876, :7914-8027) are two kernels here (k-mer table + key arrays, bk_search.hip); to
 * hold them to the reference's functions probe by probe, a context can be told to stop a batch behind the search of one phase of
 * AlignReads' schedule - bk_ctx_tune(ctx, "debug_stop_phase", p + 1), 0 = off; the batch's result records are then meaningless - and this call
 * returns what that search wrote for the reads still unaligned in that phase (one chunk: batches of at most "chunk_reads" reads):
 *   n_act, iv_cores   reads on the phase's list, cores per strand the records are numbered for
 *   act[n_act]        their numbers in the batch
 *   first / count     [(strand * iv_cores + core) * n_act + position in act]: the suffix array interval [first, first + (count & 0x3fffffff))
 *                     of the core's exact matches; bit 31 of count: a k-mer bucket of at most four suffixes handed on unverified
 *                     ("lazy_search" 1 - the extension drops the members whose core bases differ); bits 31 and 30: a bucket of ONE suffix
 *                     handed on as the suffix itself - `first` is its suffix array ELEMENT, the target position ("use_ktab2" 2: the k-mer
 *                     table's entry carries it, and the extension fetches the window without a trip to the suffix array); a core the
 *                     read does not have: count 0
 * act == NULL: only n_act and iv_cores.  cap_reads: what the arrays hold per plane. */
int  bk_debug_intervals(bk_ctx *ctx, uint32_t cap_reads, uint32_t *n_act, uint32_t *iv_cores, uint32_t *act, uint64_t *first, uint32_t *count);

/* ---- .sfx index construction (CSfxArrayV3::AddEntry/Finalise, kangax.cpp:774-926) ------------ */
/* Suffix-sorts `concat_len` bases resident in HBM (1 byte/base, EOS terminated entries) into
 * d_sa_out (sfx_el_size bytes/element) on the device: order = nibble-lexicographic exactly as
 * QSortSeqCmp32/40 (SfxArrayV2.cpp:9491-9542). */
int  bk_build_sa_device(const void *d_seq, uint64_t concat_len, void *d_sa_out, int sfx_el_size,
                        int device_id);

/* ---- contaminant (adaptor) overlaps of raw reads: `align -H` (CContaminants::MatchContaminants, Contaminants.cpp:1227-1309) ----
 * Independent of bk_ctx: a matcher needs a device, not an index, and can work while an index image is still on its way to the same device.
 * An entry is one (sequence, use) of a contaminants file as the reference keeps it: bases 0..3 a,c,g,t and 4 N, 4..200 of them, already reverse
 * complemented where the file asks for that; use 1 = 5' end of SE/PE1 reads, 2 = 5' of PE2, 3 = 3' of SE/PE1, 4 = 3' of PE2.  At most 1600.
 * bk_contam_match: for every read (1 byte/base as the loaders hold them - bits 0..2 the base, the rest ignored; offs == NULL: the reads lie back
 * to back) out[2i] / out[2i+1] = the bases the reference's loader would cut from its 5' / 3' end beyond the fixed trims: with L the largest
 * overlap length, trim + 1 <= L <= min(read, longest entry of the use), at which an entry of at least L bases differs in at most one
 * position from the read's first L bases (its own last L; 5') or the read's last L (its own first L; 3') - a read N always differs, an entry N never -
 * L - trim, and 0 without such an L, without entries of the use, and for reads shorter than 20 or longer than 2000 bases.  is_pe2: per read,
 * non-zero = a PE2 read (uses 2 and 4); NULL: all_pe2 (0 | 1) holds for every read.
 * The reads cross in chunks of at most 64 MB of bases / 2^20 reads through page-locked staging on a stream of the matcher's own, two in flight:
 * under 160 MB of device memory and as much page-locked host memory (allocated by the first match call) whatever the number of reads.
 * Calls on one matcher must not overlap.  BK_ERR_PARAMS: a NULL array, an entry outside the limits above, a negative trim, all_pe2 not 0 | 1. */
typedef struct bk_contam bk_contam;
typedef struct bk_contam_entry {
    const uint8_t *bases;
    uint32_t len;
    uint32_t use;
} bk_contam_entry;
int  bk_contam_create(bk_contam **out, int device_id, const bk_contam_entry *entries, uint32_t n_entries);
void bk_contam_destroy(bk_contam *c);
int  bk_contam_match(bk_contam *c, const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint64_t nreads, const uint8_t *is_pe2,
                     int all_pe2, int trim5, int trim3, uint16_t *out);

#ifdef __cplusplus
}
#endif
#endif
