// bk_ctx_int.h - internal: the context behind the C ABI (include/biokanga_amd.h), shared by bk_engine.cpp (batch driver)
// and bk_stream.cpp (overlapped host <-> device pipeline).  Not part of the boundary.
// Who owns what: every device allocation of a context is a bk::DevBuf and every page-locked one a bk::PinBuf, whose capacity is the
// buffer's own size (bk_devbuf.h).  The index image and the grow worker's tables are bk_ctx::image (ImageBufs, filled by bk_image.cpp), the
// small fixed buffers (counters, phase control, the SNP planes) bk_ctx::fixed (FixedBufs), the engine's scratch and what the batch entry
// points grow on demand bk_ctx::buf (BatchBufs); each request pass over finished alignments keeps its own staging (bk_stage.h: bk_ctx::snp,
// site, primer, samtag, cov, dup, jct).  bk_ctx_destroy frees nothing by name: release_image_buffers(), release_batch_buffers() and
// release_pinned_buffers() give the lot back.  POD structs that travel to kernels (DevIndex - set from the image by publish_index alone -
// HeavyScratch, DevBatch) carry raw pointers into them.
#pragma once
#include <atomic>
#include <thread>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "bk_device.h"
#include "bk_devbuf.h"
#include "bk_stage.h"

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess) {                                                                   \
            fprintf(stderr, "biokanga_amd: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return e__ == hipErrorOutOfMemory ? BK_ERR_MEM : BK_ERR_INTERNAL;                      \
        }                                                                                          \
    } while (0)
#define BK_TRY(expr) do { const int rc__ = (expr); if (rc__) return rc__; } while (0)      // a step that returns a BK_ code: anything but BK_OK ends the caller with it

namespace bk {
// the engine's scratch: the device buffers the batch driver and the batch entry points grow on demand (capacities in elements: DevBuf::cap)
struct BatchBufs {
    // batch scratch (ensure_batch_scratch: sized together by cap_reads / cap_wpr / cap_rd2w / cap_iv_cores of the context)
    DevBuf<uint64_t> rd4, rd2, iv_first;  // packed read rows (4 bit, 2 bit: DevBatch::rd4, rd2), interval records of an index beyond 2^32
    DevBuf<uint2> iv2, iv32;              // DevBatch::iv2, iv32
    DevBuf<uint32_t> iv_n, rmeta;         // DevBatch::iv_n, rmeta
    DevBuf<uint32_t> act[2], heavy, wave, wave_work;      // the phases' work lists (DevBatch::wave_work)
    DevBuf<uint32_t> stage[3], stripe_cnt;                // their striped forms (bk::StripeSet)
    DevBuf<uint32_t> slist, slist_stage;  // work list of the two-pass search and its striped form (ensure_slist)
    DevBuf<uint32_t> sort[3];             // keys in, keys out, list out of sort_work (ensure_sort_scratch)
    DevBuf<uint8_t> sort_tmp, scan_tmp;   // the sort's temporary; the offset scan's of packed batches
    DevBuf<bk_seg2> seg2;                 // -a / -A / -c: second segments of a chunk (ensure_seg2)
    // staging for host-buffer batches: the bases, the per-read group (ensure_in_reads), the packed form's words and exceptions
    DevBuf<uint8_t> in_bases;
    DevBuf<uint64_t> in_offs;
    DevBuf<uint32_t> in_lens;
    DevBuf<bk_hit> in_out;
    DevBuf<uint16_t> in_lens16;           // (packed batches only: empty, or as long as the rest of the group)
    DevBuf<uint32_t> in_words;
    DevBuf<bk_nbase> in_exc;
    DevBuf<uint8_t> chrom_accept;         // bk_ctx_set_chrom_filter: by sequence id, what the PE rules ask of the -Z / -z filters
    DevBuf<unsigned long long> htab;      // HeavyScratch::htab, slot_epoch (size_heavy_scratch)
    DevBuf<uint32_t> slot_epoch;
    DevBuf<uint2> plan;                   // DevBatch::plan: the plan table (bk_plan_table.h; bk_engine.cpp, plan_table_for)
};
// the index image in HBM, one owner per allocation; bk::publish_index (bk_image.cpp) sets the pointers of DevIndex from them
struct ImageBufs {
    DevBuf<uint64_t> tgt4, tgt2, tgt2s;   // packed target, 4 bit/base; its 2 bit/base copy, the same stored 32 bytes later (DevIndex::tgt2, tgt2s)
    DevBuf<uint32_t> sa_lo, isa;          // suffix array (low 32 bits of every element), inverse suffix array
    DevBuf<uint8_t> sa_hi, nflag;         // fifth byte of an index's 5-byte elements (empty otherwise); N/EOS block bitmap beside tgt2
    DevBuf<uint64_t> ent_start, ent_end;  // entry table
    DevBuf<uint32_t> ent_id, id2idx;
    DevBuf<uint8_t> ktab;                 // k-mer table, in bytes: it has four views (DevIndex::ktab32 / ktab64 / ktab_hi + ktab32 / ktab2)
    DevBuf<uint64_t> ktab_hi;             // .. a 64-bit start per 2^16 codes where the table is 32-bit offsets from those ("ktab_wide" 1; every group spans < 2^32 suffixes)
    DevBuf<uint32_t> k2, kx[kMoreKeys];   // second-level search keys; third-, fourth-level (DevIndex::k2, kx)
    DevBuf<uint8_t> swin;                 // suffix-ordered window array (DevIndex::swin), built when the first batch it serves arrives
    DevBuf<uint32_t> swmap;               // .. and which blocks of the suffix array it holds (DevIndex::swmap; empty: all of them)
    DevBuf<uint32_t> grow_kx[kMoreKeys];  // BK_CTX_GROW_IMAGE: what the worker has made - its thread's alone until the batches' thread has
    DevBuf<uint8_t> grow_ktab2;           // .. joined it or acquire-loaded grow_state - and the batches' thread has not yet taken in
};
// The words of FixedBufs::small (zeroed by whoever is about to use one; bk_ctx::h_small mirrors them).  kSmCount: length of the list a pass
// is making - reads with several loci, reads for the indel / chimeric search, PE orphans, SNP sites; kSmCursor: the wave-per-read kernel's
// cursor over that list (launch_pe takes the two as neighbours); kSmReplayErr: reads whose loci replay disagreed with LowHitInstances;
// kSmBestCursor: -N, launch_best's cursor; kSmMaxLen: longest read of a batch; kSmMinLenInv: ~(shortest read) (min_len_of reads it)
enum SmallWord : uint32_t { kSmCount = 0, kSmCursor = 1, kSmReplayErr = 2, kSmBestCursor = 4, kSmMaxLen = 5, kSmMinLenInv = 6, kSmallWords = 16 };
// the context's small device buffers of fixed size
struct FixedBufs {
    DevBuf<uint32_t> small;               // kSmallWords words, by SmallWord (3 and 7 .. 15: nobody's)
    DevBuf<PhaseCtl> ctl;                 // kCtlLines lines: the counts of a chunk's phases and the batch's line (bk_device.h)
    DevBuf<unsigned long long> seq_counts, ctr, ctr_aux, snp_tot;
    DevBuf<unsigned long long> seq_global;        // bk_seq_counts_allreduce: the counts summed over every context of the run
    DevBuf<uint32_t> snp_planes;          // SNP pile-up: 6 count planes over the concatenated target
};
}  // namespace bk

struct bk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bk_align_params params{};
    bk::DevAlignCfg cfg{};
    bk::DevIndex ix{};
    bk::ImageBufs image;                  // owned device allocations of the index image
    bk::FixedBufs fixed;                  // .. and the small fixed buffers
    void release_image_buffers() { image = bk::ImageBufs{}; fixed = bk::FixedBufs{}; }
    uint64_t n_tgt4_words = 0;
    uint32_t cap_rd2w = 0;
    int use_tgt2 = 2;        // 0: 4-bit windows only, 1: 2-bit copy, 2: 2-bit copy stored twice (32 bytes apart)
    int sort_lists = 7;      // bit 0: search work list grouped by index position; bit 1: wave list sorted, by index position or (bit 2) longest read first
    bool sort_lists_set = false;   // .. as the caller's knob left it; else bit 0 follows the index: off where it has third-level keys (tables_end)
    int sort_shift = 0;      // keys = suffix array index >> sort_shift (fits 32 bits)
    int search_split = 1;    // pass B in two launches: the key levels, then - dense - the items they do not settle (k_search_deep)
    bool search_split_set = false; // .. as the caller's knob left it; else on where the work list is not grouped (bit 0 of sort_lists clear), off where it is
    int use_k2 = 1;
    int use_k3 = bk::kMoreKeys;  // key arrays behind the second-level keys (DevIndex::kx): at most this many, where the HBM has the room
    // BK_CTX_GROW_IMAGE: the tables that only pay over long runs (key arrays behind the second-level keys, k-mer table entries with their
    // bucket's first key) are made by a thread of their own once the context has aligned grow_after reads, and taken in between two batches
    bool grow_enabled = false, grow_wait = false;
    uint64_t grow_after = 5 * BK_POLICY_MIN_READS, grow_seen = 0;      // (a context that was started lean for a short job and turned out to run a long one)
    std::atomic<int> grow_state{0};          // 0 not started, 1 being made, 2 made, 3 nothing made (no room / not in order), 4 taken in
    std::thread grow_thread;
    bk::DevIndex grow_ix{};                  // the index as it was when the worker started (its own copy: the batches' thread goes on changing ix - the window array)
    bool grow_want_ktab2 = false;
    bool grow_elem = false, grow_want_elem = false;        // the worker's k-mer table of pairs carries suffix array elements for buckets of one suffix ("use_ktab2" 2)
    int use_ktab2 = 1;       // k-mer table entries of two words (DevIndex::ktab2): 1 - a bucket of one suffix carries its second-level key; 2 - its suffix array element (DevIndex::ktab2_elem: the search hands the suffix on, kElemFlag - measured slower, round 6: the buckets whose key the search would have turned down reach the extension as candidates)
    bool ktab_is2 = false;
    int use_iv32 = 1;        // phase 0 leaves the interval of a read's first k + 16 bases for the offset-0 cores of the later phases
    uint32_t wave_waves = 256u * 8u * 4u;   // resident waves the wave kernel is launched with
    int wave_len_spec = 1;   // 1: a batch whose reads all have the same number of 16-base dwords gets the wave kernel's form compiled for it; 0: the generic form always
    int use_isa = 1;         // 0: no inverse suffix array - the wave kernel dedupes with its hash set (as it does for 5-byte indexes)
    int use_swin = 1;         // 0: none; 1: the part of the suffix array the wave kernel's long walks visit; 2: the same, whatever the batch's read lengths; 3: every suffix
    uint64_t swin_budget = 0; // most bytes the partial array may take (0: by the free memory)
    int swin_skip_short = 0;  // the coverage rule leaves out this many of the reads' shortest core lengths
    int swin_w = 0;           // the core length the partial array's coverage was made for
    uint64_t swin_bytes = 0;  // what array and map occupy
    double swin_setup_s = 0;  // .. and what making them took (allocation included)
    double swin_covered = 0;  // .. share of the suffix array it holds
    bool swin_denied = false; // it did not fit beside a batch's scratch when first asked for
    bool swin_rebuilt = false; // a batch has already made the partial array again for its own core lengths (maybe_build_swin does that once)
    int prep_search0 = 1;    // the fused read preparation also runs phase 0's pass A where it can (prep_search0_on, bk_engine_int.h)
    int iv_poison = 0;       // test hook: the interval records a phase can use are filled with ones in front of its search (a slot read but not written shows)
    int use_wave = 1;        // 1: k_light / k_wave for reads <= 256 bp, 0: k_extend / k_heavy only
    int lazy_search = 1;     // 1: small k-mer buckets are handed to the extend kernels unverified
    bool ktab64 = false;
    int ktab_wide = 0;                    // "ktab_wide": 0 bucket starts of 64 bits only where the index needs them; 1 always, packed as ktab_hi + offsets; 2 always, unpacked (tests)
    int k_req = -1;          // requested k (-1 auto)
    int use_ktab = 1;
    uint32_t el_size = 4;
    uint64_t tot_seq_len = 0;
    std::string dataset;
    std::vector<bk_entry_info> entries;
    bk::BatchBufs buf;                    // the engine's scratch, grown on demand
    // the request passes' staging and chunk knobs (bk_stage.h; SNP pile-up: the count planes are fixed.snp_planes)
    bk::SnpStage snp;
    bk::SiteStage site;
    bk::PrimerStage primer;
    bk::SamtagStage samtag;
    bk::CovStage cov;
    bk::DupStage dup;
    bk::JunctionStage jct;
    void release_batch_buffers()
    {
        buf = bk::BatchBufs{}; snp = bk::SnpStage{}; site = bk::SiteStage{}; primer = bk::PrimerStage{}; samtag = bk::SamtagStage{}; cov = bk::CovStage{};
        dup = bk::DupStage{}; jct = bk::JunctionStage{};
    }
    // what the batch scratch was sized for (scratch_bytes_per_read, maybe_build_swin)
    uint32_t cap_reads = 0, cap_wpr = 0, cap_iv_cores = 0;
    bk::PinBuf<uint32_t> h_small;         // pinned mirror of fixed.small
    bk::PinBuf<bk::PhaseCtl> h_line;      // pinned, two lines: a phase's counts and the next one's, where the phase loop reads them back
    bk::PinBuf<bk::PhaseCtl> h_ctl;       // pinned: the last chunk's counts (fixed.ctl), copied behind its kernels
    hipEvent_t ev_ctl = nullptr;
    bool ctl_pending = false, hist_valid = false;
    uint32_t ctl_pending_reads = 0, ctl_pending_maxlen = 0;
    int ctl_pending_phases = 0;
    double hist_slist[bk::kMaxPhases] = {0}, hist_wave[bk::kMaxPhases] = {0};      // per phase: pass B items / wave-kernel reads per read of the chunk
    int async_error = 0;     // what take_phase_history found wrong with a batch of bk_align_batch_device_async (reported by the next call)
    int async_phases = 1;    // 1: the main path's phase loop launches without reading counts back (see align_chunk)
    bool force_rccl = false;                      // bk_seq_counts_allreduce goes through RCCL even on one device ("force_rccl")
    uint64_t rccl_allreduces = 0;                 // .. how many of this context's reductions went through RCCL, the ranks of the last one's communicator
    int rccl_ranks = 0;
    // the plan table (buf.plan): what it was made for - the longest read, the configuration fields make_plan reads - and the pinned
    // copy it is uploaded from (the host's own look-ups go there too).  Made again when a batch has a longer read or a field has changed.
    bk::PinBuf<uint2> h_plan;
    uint32_t plan_maxlen = 0;
    int plan_key[4] = {-1, -1, -1, -1};   // max_subs, mm_delta, min_core_len, slides_per100
    hipEvent_t ev_plan = nullptr;         // behind the last upload: the pinned copy is not written before it has been read
    // heavy path scratch (owned by buf.htab, buf.slot_epoch)
    bk::HeavyScratch hs{};
    int max_read_len = 500;
    uint32_t last_maxlen = 0;    // longest read of the last align call
    // test hook (bk_debug_intervals): batches stop behind the search of this phase and leave its interval records in the scratch
    int dbg_stop_phase = -1, dbg_phase = 0, dbg_cur = 0;
    uint32_t dbg_n = 0, dbg_ivc = 0;
    bool dbg_valid = false;
    bool dbg_by_read = false;       // the stopped phase's interval slots go by read number (bk_iv_slot.h)
    bool debug = false;      // BK_DEBUG in the environment when the context was created: per-phase counts on stderr
    uint32_t chunk_reads = 64u << 20;
    uint64_t constraint_chunk = 4u << 20; // bk_constraints_check stages this many requests at a time ("constraint_chunk"; the staging is the set's)

    hipEvent_t ev_wait = nullptr;         // an event the caller's thread sleeps on (bk_wait.h)
    bool entries_set = false, tgt2_built = false;     // .. and so do the entry table / the 2-bit target (made early for a window array that is made behind the upload too)
    bool tables_built = false;            // k-mer table, second-level keys, inverse suffix array exist (made behind the suffix array's upload)
    bool tables_under_way = false;        // .. are being made (tables_begin .. tables_end): publish_index leaves their pointers null
    bk::PinBuf<char> sam_text[2];         // bk_sam_format's page-locked text buffers, kept for the next call (giving page-locked memory back costs 0.1 s per GB)
    void release_pinned_buffers() { h_small.reset(); h_line.reset(); h_ctl.reset(); h_plan.reset(); sam_text[0].reset(); sam_text[1].reset(); }
    uint32_t n_chrom_accept = 0;          // entries of buf.chrom_accept (bk_ctx_set_chrom_filter)
    bk_timing timing{};
    std::vector<hipEvent_t> ev_pool;
    // multi-loci modes: loci lists of the last align call (host side, see bk_batch_loci)
    std::vector<uint64_t> loci_offs;
    std::vector<bk_loci> loci;
    std::vector<bk_loci_trims> loci_trims;   // -c with the multi-loci modes: one per locus
    std::vector<bk_seg2> seg2;           // -a: second segments of the last align call, one per read
};


namespace bk {
// a batch of reads resident in HBM, in either form the boundary takes
struct DevReads {
    const uint8_t *bases = nullptr;       // 1 byte/base form: the bases, offs[i] = start of read i in them
    const uint64_t *offs = nullptr;       //   (packed form: first word of read i in `words`)
    const uint32_t *lens = nullptr;
    const uint32_t *words = nullptr;      // packed form (bk_align_batch_packed): 2 bit/base words, then bases == nullptr
    const bk_nbase *exc = nullptr;        //   + the bases that are not a,c,g,t
    uint64_t n_exc = 0;
};
// batch driver entry points of bk_engine.cpp used by the stream pipeline (all blocking on `s`: the phase loop reads the
// active counts back between phases)
// maxlen_known / minlen_known: the longest and the shortest read where the caller has looked (0: not; the shortest only counts beside the longest)
int engine_align_device(bk_ctx *c, const DevReads &in, uint32_t nreads, bk_hit *d_out, hipStream_t s, uint32_t maxlen_known = 0, uint32_t minlen_known = 0);
void release_swin(bk_ctx *c);
void drop_swin(bk_ctx *c);
int engine_pair_device(bk_ctx *c, const DevReads &in, uint32_t n_pairs, bk_hit *d_hits, uint32_t maxlen, const bk_pe_params *pe, hipStream_t s,
                       bk_seg2 *seg2_host = nullptr, bk_seg2 *seg2_dev = nullptr);
// packed batches: lens16 -> d_lens32, word offsets of the reads -> d_offs (scan), the batch checked (word count, read lengths,
// exception list); *maxlen = longest read, *minlen = shortest.  Blocking on `s`.
int engine_prepare_packed(bk_ctx *c, const uint16_t *d_lens16, uint32_t nreads, uint64_t n_words, const bk_nbase *d_exc, uint64_t n_exc,
                          uint32_t *d_lens32, uint64_t *d_offs, uint32_t *maxlen, uint32_t *minlen, hipStream_t s);
}  // namespace bk

namespace bk {
// bk::dev_malloc_bytes (bk_devbuf.h) is the hipMalloc for everything the library owns.  BK_POISON=<byte> (debugging aid) fills every allocation
// with that byte, so a kernel that reads device memory nobody wrote meets the same bytes on every box, not whatever the previous process left in HBM.
hipError_t dev_zero_now(void *p, size_t bytes);
// Host -> device copy that runs near PCIe rate whatever the kind of host memory: pinned sources are DMA'd directly; pageable
// ones (file mappings, std::vector) are copied by a few host threads into a pool of pinned staging buffers, each thread feeding
// its own HIP stream, so that the DRAM / page-cache reads and the DMAs of different slices overlap (a plain hipMemcpy stages
// through one thread: 6-8 GB/s).  Returns when the bytes are on the device.  bk_upload.cpp
int upload_host(void *d_dst, const void *h_src, size_t bytes, int device);
int upload_file(void *d_dst, int fd, uint64_t file_ofs, size_t bytes, int device);       // the same from a file range, read() into the staging buffers
bool host_is_pinned(const void *p);

// what the request passes share (bk_requests.cpp)
std::vector<uint32_t> seq_len_by_id(const bk_ctx *c);       // by sequence id; 0: no such sequence
// part(lo, hi) over [0, n) on the caller's thread when the bytes to move are below 8 MB, else in slices on min(8, effective_cpus()) threads
void gather_split(uint64_t total_bytes, uint32_t n, const std::function<void(uint32_t, uint32_t)> &part);
// reads t = 0 .. n - 1 of `src`, where span_of(t) gives read t's offset and length in it, back to back into dst: read t at dst_ofs[t]
// (~0: not this one); total_bytes is what moves
template <class SpanOf> inline void gather_reads(uint8_t *dst, const uint64_t *dst_ofs, const uint8_t *src, uint64_t total_bytes, uint32_t n, SpanOf span_of)
{
    gather_split(total_bytes, n, [&](uint32_t lo, uint32_t hi) {
        for (uint32_t t = lo; t < hi; t++) {
            if (dst_ofs[t] == ~0ULL) continue;
            const std::pair<uint64_t, uint32_t> sp = span_of(t);
            memcpy(dst + dst_ofs[t], src + sp.first, sp.second);
        }
    });
}
}  // namespace bk
