// bk_engine.cpp - the batch driver behind the C ABI in include/biokanga_amd.h: batch scratch, the phase loop of CSfxArrayV3::AlignReads over
// whole batches (libbiokanga/SfxArrayV2.cpp:7666-7760), the paired-end pass, the packed and device-resident batch forms, counters, timing.
// Compiled with hipcc; device code lives in the kernel files (bk_prep / bk_search / bk_extend / bk_wave / bk_heavy / bk_rescue .hip); the index
// image and the context's life are bk_image.cpp, knobs bk_tune.cpp, the exchange step bk_exchange.cpp.  No CPU fallback exists: every
// compute entry point needs a HIP device and fails with BK_ERR_NODEVICE otherwise.
// Ownership: every buffer this file grows is a bk::DevBuf of bk_ctx::buf (bk_devbuf.h, bk_ctx_int.h) and is grown by one ensure_* function
// here; a chunk's temporaries are local DevBufs, so an early return frees them.  Nothing here frees device memory by hand.
#include "bk_engine_int.h"
#include "bk_iv_slot.h"
#include "bk_wave_form.h"

namespace bk {
int size_heavy_scratch(bk_ctx *c)
{
    // worst-case inserts per strand pass = min(node cap, cores(max_read_len) * MaxIter)
    int slides = std::max(1, (c->cfg.slides_per100 * c->max_read_len + 99) / 100);
    uint64_t worst = c->cfg.max_iter ? (uint64_t)slides * (uint64_t)c->cfg.max_iter : kNodeCap;
    if (worst > kNodeCap) worst = kNodeCap;
    uint32_t ts = 1024;
    while (ts < 2 * worst) ts <<= 1;
    uint32_t slots = 4096;                  // one per resident wave of the hash-set forms (four blocks of four waves a CU: 40 KB of LDS each) when they fit in 16 GB
    while ((uint64_t)slots * ts * 8 > (16ULL << 30) && slots > 64) slots >>= 1;
    if (c->hs.htab && c->hs.tab_size == ts && c->hs.n_slots == slots) return BK_OK;
    BatchBufs &m = c->buf;
    m.htab.reset();
    m.slot_epoch.reset();
    c->hs = HeavyScratch{};
    HIP_TRY(m.htab.ensure((size_t)slots * ts));
    HIP_TRY(m.slot_epoch.ensure(slots));
    launch_fill_u64(m.htab.get(), (uint64_t)slots * ts, 0ULL, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(m.slot_epoch.get(), 0, (size_t)slots * 4, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->hs = HeavyScratch{m.htab.get(), m.slot_epoch.get(), ts, slots};
    return BK_OK;
}


// (all of the scratch is freed before any of it is allocated: the old and the new never lie in HBM side by side)
int ensure_batch_scratch(bk_ctx *c, uint32_t n_reads, uint32_t wpr, uint32_t rd2w, uint32_t iv_cores)
{
    if (n_reads <= c->cap_reads && wpr <= c->cap_wpr && rd2w <= c->cap_rd2w && iv_cores <= c->cap_iv_cores) return BK_OK;
    const size_t nr = std::max(n_reads, c->cap_reads), w = std::max(wpr, c->cap_wpr), w2 = std::max(rd2w, c->cap_rd2w);
    const size_t ivc = std::max(iv_cores, c->cap_iv_cores);
    BatchBufs &m = c->buf;
    m.rd4.reset(); m.iv_first.reset(); m.iv_n.reset(); m.rd2.reset(); m.iv2.reset(); m.rmeta.reset();
    m.act[0].reset(); m.act[1].reset(); m.heavy.reset(); m.wave.reset(); m.iv32.reset(); m.wave_work.reset();
    for (auto &st : m.stage) st.reset();
    c->cap_reads = 0;
    HIP_TRY(m.rd4.ensure(nr * 2 * w));
    if (w2) HIP_TRY(m.rd2.ensure(nr * 2 * w2 + 8));        // (+ the words a 32-base fetch at a row's end runs into)
    HIP_TRY(m.rmeta.ensure((nr + 2) / 2 * 2));
    if (c->image.sa_hi.get() == nullptr && c->ix.n < (1ULL << 32))
        HIP_TRY(m.iv2.ensure(nr * 2 * ivc));
    else {
        HIP_TRY(m.iv_first.ensure(nr * 2 * ivc));
        HIP_TRY(m.iv_n.ensure(nr * 2 * ivc));
    }
    HIP_TRY(m.act[0].ensure(nr));
    HIP_TRY(m.act[1].ensure(nr));
    HIP_TRY(m.heavy.ensure(nr));
    HIP_TRY(m.wave.ensure(nr));
    for (auto &st : m.stage) HIP_TRY(st.ensure(nr + (kListStripes + 2) * 1024));      // striped forms of the lists (StripedList)
    if (!m.stripe_cnt.get()) {
        HIP_TRY(m.stripe_cnt.ensure((size_t)2 * kListStripes * 16));
        HIP_TRY(dev_zero_now(m.stripe_cnt.get(), (size_t)2 * kListStripes * 16 * 4));
    }
    if (m.iv2.get()) HIP_TRY(m.iv32.ensure(nr * 2));
    HIP_TRY(m.wave_work.ensure(nr));
    c->cap_reads = (uint32_t)nr;
    c->cap_wpr = (uint32_t)w;
    c->cap_rd2w = (uint32_t)w2;
    c->cap_iv_cores = (uint32_t)ivc;
    return BK_OK;
}

// The groups below grow together: every member is freed before any is allocated, and the member allocated last speaks for the group (it
// is there only when the ones before it are).
// pass B's work list (at most one item per read, strand and core) and its striped form (StripeSet)
int ensure_slist(bk_ctx *c, uint64_t lanes, hipStream_t s)
{
    BatchBufs &m = c->buf;
    if (m.slist_stage.get() && lanes <= m.slist.cap()) return BK_OK;
    HIP_TRY(hipStreamSynchronize(s));
    m.slist.reset();
    m.slist_stage.reset();
    HIP_TRY(m.slist.ensure(lanes));
    HIP_TRY(m.slist_stage.ensure(lanes + (kListStripes + 2) * 1024));
    return BK_OK;
}

// The plan table (bk_plan_table.h) for reads of up to maxlen bases, in HBM and in its pinned copy: kept from batch to batch, made again
// only when a batch has a longer read than the table covers or when one of the configuration fields the derivation reads differs from
// what the table was made with (bk_ctx_set_params -> derive_cfg is their only writer; comparing the fields themselves leaves no setter
// to forget).  A shorter batch reads the longer table.  The upload goes on the batch's stream and nothing waits for it; making the table
// again first waits for the previous upload to have left the pinned copy, and growing it for the stream (ensure_slist's rule).  Those
// waits and allocations belong to the blocking calls and to bk_ctx_reserve, which makes the table for its max_read_len as it sizes the
// rest of the scratch: the call that only enqueues asks plan_table_covers and refuses a batch the table does not serve as it stands.
// (The two early returns are unreachable through derive_cfg, which hands out mm_delta 1 or 2 and at most 9 slides per 100 bases - 180
// cores at 2000 bases against the 1023 the packing holds; they keep a future parameter from becoming a division by zero or a
// truncated field.)
bool plan_table_covers(const bk_ctx *c, uint32_t maxlen)
{
    const int key[4] = {c->cfg.max_subs, c->cfg.mm_delta, c->cfg.min_core_len, c->cfg.slides_per100};
    return c->buf.plan.get() != nullptr && maxlen <= c->plan_maxlen && std::equal(key, key + 4, c->plan_key);
}

int plan_table_for(bk_ctx *c, uint32_t maxlen, hipStream_t s)
{
    const int key[4] = {c->cfg.max_subs, c->cfg.mm_delta, c->cfg.min_core_len, c->cfg.slides_per100};
    if (plan_table_covers(c, maxlen)) return BK_OK;
    if (c->cfg.mm_delta < 1 || maxlen > (uint32_t)kMaxReadLenAbs) return BK_ERR_PARAMS;
    const uint32_t cover = std::max(maxlen, std::equal(key, key + 4, c->plan_key) ? c->plan_maxlen : 0u);
    const int rows = plan_table_rows(c->cfg, (int)cover);
    if (rows > kMaxPhases + 1) return BK_ERR_INTERNAL;
    const size_t n = (size_t)rows * (cover + 1);
    if (!c->ev_plan) HIP_TRY(hipEventCreateWithFlags(&c->ev_plan, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(c->ev_plan));
    c->plan_maxlen = 0;
    HIP_TRY(c->h_plan.ensure(n));
    if (n > c->buf.plan.cap()) {
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(c->buf.plan.ensure(n));
    }
    if (!plan_table_fill(c->cfg, (int)cover, rows, c->h_plan.get())) return BK_ERR_INTERNAL;
    HIP_TRY(hipMemcpyAsync(c->buf.plan.get(), c->h_plan.get(), n * sizeof(uint2), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev_plan, s));
    std::copy(key, key + 4, c->plan_key);
    c->plan_maxlen = cover;
    return BK_OK;
}

// the per-read group of a host batch: offsets, lengths, result records, and for a packed batch the 16-bit lengths
int ensure_in_reads(bk_ctx *c, uint32_t n, bool packed)
{
    BatchBufs &m = c->buf;
    if (n > m.in_out.cap()) {
        m.in_offs.reset(); m.in_lens.reset(); m.in_out.reset(); m.in_lens16.reset();
        HIP_TRY(m.in_offs.ensure(n));
        HIP_TRY(m.in_lens.ensure(n));
        HIP_TRY(m.in_out.ensure(n));
    }
    if (packed) HIP_TRY(m.in_lens16.ensure(m.in_out.cap()));
    return BK_OK;
}

HostExtent host_extent(const uint64_t *offs, const uint32_t *lens, uint32_t nreads)
{
    HostExtent x;
    for (uint32_t i = 0; i < nreads; i++) {
        x.lo = std::min(x.lo, offs[i]);
        x.hi = std::max(x.hi, offs[i] + lens[i]);
        x.maxlen = std::max(x.maxlen, lens[i]);
    }
    x.rel.resize(nreads);
    for (uint32_t i = 0; i < nreads; i++) x.rel[i] = offs[i] - x.lo;
    return x;
}

// a host batch into the context's staging buffers: bases of the extent, relative offsets, lengths - enqueued on the context's stream
// (x.rel is their source until the caller has synchronised)
static int stage_host_batch(bk_ctx *c, const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint32_t nreads, HostExtent &x, DevReads &in)
{
    x = host_extent(offs, lens, nreads);
    if (x.maxlen > (uint32_t)kMaxReadLenAbs) return BK_ERR_PARAMS;
    const uint64_t nbytes = x.hi - x.lo;
    BatchBufs &m = c->buf;
    HIP_TRY(m.in_bases.ensure(nbytes + 16));
    BK_TRY(ensure_in_reads(c, nreads, false));
    HIP_TRY(hipMemcpyAsync(m.in_bases.get(), bases + x.lo, nbytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(m.in_offs.get(), x.rel.data(), (size_t)nreads * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(m.in_lens.get(), lens, (size_t)nreads * 4, hipMemcpyHostToDevice, c->stream));
    in.bases = m.in_bases.get(); in.offs = m.in_offs.get(); in.lens = m.in_lens.get();
    return BK_OK;
}

// the DevBatch of reads first .. first + n of `in` over the scratch ensure_batch_scratch has sized; what only the phase loop uses (rd2,
// wave_work, iv32, nw, iv_stride, act) is left empty
static DevBatch make_batch(bk_ctx *c, const DevReads &in, uint32_t first, uint32_t n, uint32_t wpr, uint32_t iv_cores, bk_hit *d_out)
{
    const BatchBufs &m = c->buf;
    DevBatch b{};
    b.bases = in.bases; b.offs = in.offs + first; b.lens = in.lens + first;
    b.pk_words = in.words; b.pk_exc = in.exc; b.pk_nexc = in.words ? in.n_exc : 0; b.pk_read0 = first;
    b.rd4 = m.rd4.get(); b.iv_first = m.iv_first.get(); b.iv_n = m.iv_n.get(); b.iv2 = m.iv2.get();
    b.rmeta = m.rmeta.get();
    b.out = d_out; b.seq_counts = c->fixed.seq_counts.get(); b.ctr = c->fixed.ctr.get();
    b.wpr = wpr; b.n_reads = n; b.iv_cores = iv_cores;
    return b;
}

enum class Span { Search, Extend, Heavy, Other, SearchA, SearchSort, SearchB, Prep };      // what a timed span counts into (align_device)

struct EvTimer {
    bk_ctx *c;
    bool on = true;                     // off: no events (a call that returns before its kernels have run cannot read them)
    std::vector<std::pair<Span, std::pair<hipEvent_t, hipEvent_t>>> spans;   // kind, (start, stop)
    size_t next_ev = 0;
    hipEvent_t get()
    {
        if (!on) return nullptr;
        if (next_ev == c->ev_pool.size()) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            c->ev_pool.push_back(e);
        }
        return c->ev_pool[next_ev++];
    }
    hipEvent_t begin(hipStream_t s)
    {
        hipEvent_t e = get();
        if (e) (void)hipEventRecord(e, s);
        return e;
    }
    void end(Span kind, hipEvent_t b, hipStream_t s)
    {
        hipEvent_t e = get();
        if (!e) return;
        (void)hipEventRecord(e, s);
        spans.push_back({kind, {b, e}});
    }
};

// one chunk of reads, all phases.  Blocking (host reads back the active counts between phases).
// Work-list grouping.  A list is reordered so that items touching the same part of the index (same k-mer
// bucket / same core interval: reads from one repeat family) sit next to each other: neighbouring lanes then
// walk the same bisection path (their loads coalesce) and neighbouring waves fetch the same target windows
// (L2 hits instead of HBM misses).  Results do not depend on the order.
int ensure_sort_scratch(bk_ctx *c, uint32_t n, hipStream_t s)
{
    BatchBufs &m = c->buf;
    if (m.sort_tmp.get() && n <= m.sort[2].cap()) return BK_OK;
    HIP_TRY(hipStreamSynchronize(s));
    for (auto &p : m.sort) p.reset();
    m.sort_tmp.reset();
    const uint64_t cap = (uint64_t)n + n / 4;
    for (auto &p : m.sort) HIP_TRY(p.ensure(cap));
    size_t tb = 0;
    if (sort_list_by_key(nullptr, nullptr, nullptr, nullptr, (uint32_t)cap, nullptr, &tb, s)) return BK_ERR_INTERNAL;
    HIP_TRY(m.sort_tmp.ensure(tb));
    return BK_OK;
}

// keys are expected in buf.sort[0]; returns the reordered list (buf.sort[2])
int sort_work(bk_ctx *c, const uint32_t *list, uint32_t n, hipStream_t s, const uint32_t **out)
{
    const BatchBufs &m = c->buf;
    size_t tb = m.sort_tmp.cap();
    if (sort_list_by_key(m.sort[0].get(), m.sort[1].get(), list, m.sort[2].get(), n, m.sort_tmp.get(), &tb, s)) return BK_ERR_INTERNAL;
    *out = m.sort[2].get();
    return BK_OK;
}

// What the multi-loci modes share: per-read counts -> offsets (scan) -> the chunk's loci appended to the context's host vectors.
// begin() makes the zeroed counts, which the caller's kernels fill; scan() leaves the offsets on the device and the host, `total`, and
// room for that many loci, which the caller's kernels fill (and `trims`, when it allocated them); finish() appends them.
struct LociChunk {
    bk_ctx *c;
    uint32_t n;
    hipStream_t s;
    DevBuf<unsigned long long> cnt, offs;
    DevBuf<uint8_t> tmp;
    DevBuf<bk_loci> loci;
    DevBuf<bk_loci_trims> trims;
    size_t base = 0;                    // reads of earlier chunks
    uint64_t loci_base = 0, total = 0;
    int begin()
    {
        HIP_TRY(cnt.ensure((size_t)n + 1));
        HIP_TRY(offs.ensure((size_t)n + 1));
        HIP_TRY(hipMemsetAsync(cnt.get(), 0, ((size_t)n + 1) * 8, s));
        return BK_OK;
    }
    int scan()
    {
        size_t tb = 0;
        if (scan_counts_u64(nullptr, nullptr, n + 1, nullptr, &tb, s)) return BK_ERR_INTERNAL;
        HIP_TRY(tmp.ensure(tb ? tb : 16));
        if (scan_counts_u64(cnt.get(), offs.get(), n + 1, tmp.get(), &tb, s)) return BK_ERR_INTERNAL;
        base = c->loci_offs.empty() ? 0 : c->loci_offs.size() - 1;
        loci_base = c->loci.size();
        if (c->loci_offs.empty()) c->loci_offs.push_back(0);
        c->loci_offs.resize(base + n + 1);
        HIP_TRY(hipMemcpyAsync(c->loci_offs.data() + base, offs.get(), ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        total = c->loci_offs[base + n];
        HIP_TRY(loci.ensure((size_t)total));
        return BK_OK;
    }
    int finish()
    {
        if (total) {
            c->loci.resize(loci_base + total);
            HIP_TRY(hipMemcpyAsync(c->loci.data() + loci_base, loci.get(), (size_t)total * sizeof(bk_loci), hipMemcpyDeviceToHost, s));
            if (trims.get()) {
                c->loci_trims.resize(loci_base + total);
                HIP_TRY(hipMemcpyAsync(c->loci_trims.data() + loci_base, trims.get(), (size_t)total * sizeof(bk_loci_trims), hipMemcpyDeviceToHost, s));
            }
            HIP_TRY(hipStreamSynchronize(s));
        }
        if (loci_base)
            for (size_t i = 0; i <= n; i++) c->loci_offs[base + i] += loci_base;
        return BK_OK;
    }
};

// Multi-loci modes: the loci lists of one chunk (reads whose AlignReads returned eHRhits own LowHitInstances
// entries each).  Counts -> offsets (scan) -> single loci copied from the result records, the others replayed
// by the ENUM form of the wave-per-read kernel; appended to the context's host vectors.
int collect_loci(bk_ctx *c, const DevBatch &b, uint32_t n, uint32_t maxlen, hipStream_t s)
{
    bk_seg2 *d_seg2 = c->params.min_chimeric_len > 0 ? c->buf.seg2.get() : nullptr;       // there: every locus carries its end trims
    LociChunk lc{c, n, s};
    BK_TRY(lc.begin());
    launch_loci_count(b.out, n, c->params.clamp_ml ? c->cfg.max_hits : 0, lc.cnt.get(), s);
    BK_TRY(lc.scan());
    uint32_t n_multi = 0;
    if (lc.total) {
        uint32_t *sm = c->fixed.small.get();
        if (d_seg2) {
            HIP_TRY(lc.trims.ensure((size_t)lc.total));
            HIP_TRY(clear_dev(lc.trims.get(), (size_t)lc.total * sizeof(bk_loci_trims), s));
        }
        HIP_TRY(hipMemsetAsync(sm, 0, kSmallWords * 4, s));
        uint32_t *list = c->buf.act[0].get();          // the phase work lists are free by now
        launch_loci_single(b.out, n, lc.offs.get(), lc.loci.get(), list, sm + kSmCount, d_seg2, lc.trims.get(), s);
        HIP_TRY(hipMemcpyAsync(c->h_small.get(), sm, kSmallWords * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        n_multi = c->h_small.get()[kSmCount];
        if (n_multi) {
            BK_TRY(size_heavy_scratch(c));
            launch_loci_enum(c->ix, c->cfg, b, c->hs, list, n_multi, sm + kSmCursor, lc.offs.get(), lc.loci.get(), sm + kSmReplayErr, d_seg2 ? c->params.min_chimeric_len : 0,
                             maxlen > 512 ? 1 : 0, d_seg2, lc.trims.get(), s);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(c->h_small.get(), sm, kSmallWords * 4, hipMemcpyDeviceToHost, s));
        }
    }
    BK_TRY(lc.finish());
    if (n_multi && c->h_small.get()[kSmReplayErr] != 0) {               // a replay that did not reproduce LowHitInstances: never ignore
        fprintf(stderr, "bk: loci replay disagreed with LowHitInstances for %u reads\n", c->h_small.get()[kSmReplayErr]);
        return BK_ERR_INTERNAL;
    }
    return BK_OK;
}

// -N (LocateBestMatches): one wave-per-read pass over the reads the N policy let through, dense rows of MaxHits
// loci per read compacted into the same host-side lists the other multi-loci modes return
int best_matches_chunk(bk_ctx *c, const DevBatch &b, uint32_t n, const uint32_t *d_list, uint32_t n_list, hipStream_t s)
{
    const uint32_t width = (uint32_t)c->cfg.max_hits;
    DevBuf<bk_loci> dense;
    LociChunk lc{c, n, s};
    BK_TRY(lc.begin());
    HIP_TRY(dense.ensure((size_t)n * width));
    BK_TRY(size_heavy_scratch(c));
    uint32_t *sm = c->fixed.small.get();
    HIP_TRY(hipMemsetAsync(sm + kSmBestCursor, 0, 4, s));
    launch_best(c->ix, c->cfg, b, c->hs, d_list, n_list, sm + kSmBestCursor, lc.cnt.get(), dense.get(), s);
    HIP_TRY(hipGetLastError());
    BK_TRY(lc.scan());
    if (lc.total) {
        launch_loci_compact(dense.get(), width, lc.offs.get(), n, lc.loci.get(), s);
        HIP_TRY(hipGetLastError());
    }
    return lc.finish();
}

// ---- one chunk of reads, all phases ---------------------------------------------------------------------------------------
// The phases' counts stay in device memory (PhaseCtl).  The main path launches the whole schedule from bounds and reads nothing back;
// the other configurations read the counts back, which sizes their launches exactly.  phase_counts alone knows which of the two runs.
// PhaseCounts: a phase's counts as the host uses them - read back, or the bounds that stand in for them - and how much of a list a sort takes
struct PhaseCounts { uint32_t n_act = 0; int cmax = 0; uint64_t n_slist = 0; uint32_t n_wave = 0, n_heavy = 0, sort_slist = 0, sort_wave = 0; };
enum class Behind { Prep, PassA, Extend, Wave };

// batch scratch; the window array is a luxury: it goes before a batch is refused for want of memory
static int batch_scratch_or_release_swin(bk_ctx *c, uint32_t n_reads, uint32_t wpr, uint32_t rd2w, uint32_t ivc)
{
    const int rc = ensure_batch_scratch(c, n_reads, wpr, rd2w, ivc);
    if (!rc || !c->image.swin.get()) return rc;
    (void)hipGetLastError();
    bk::release_swin(c);
    return ensure_batch_scratch(c, n_reads, wpr, rd2w, ivc);
}

struct ChunkRun {                       // what a chunk's run works over: made by chunk_setup, handed from stage to stage
    bk_ctx *c;
    hipStream_t s;
    EvTimer &tm;                        // (off: a call that only enqueues - its caller named the longest read, nobody has looked)
    uint32_t n, maxlen, minlen;         // reads of the chunk; longest and shortest read of the call (minlen 0: nobody has looked)
    DevBatch b{}; PhaseLists l{};
    ChunkBounds cb{};                   // phases and cores a read of up to maxlen bases can have
    PhaseCtl *ctl = nullptr;            // fixed.ctl: the chunk's lines of counts
    int act_cur = 0, nw16 = 0, nstr = 1, lazy = 0;      // l.act_in is buf.act[act_cur]; window words of the kernel family (0: not the register-window path), strand passes, lazy search
    bool reg_path = false, search0 = false, no_readback = false;
    // scratch, the batch, the plan table and the bounds it gives, which schedule runs and whether the preparation searches phase 0
    int chunk_setup(const DevReads &in, uint32_t first, bk_hit *d_out)
    {
        const uint32_t wpr = words_per_read(maxlen), rd2w = rd2_words(c, maxlen), ivc = iv_cores_for(c, maxlen);
        nw16 = c->use_wave ? window_words_for(maxlen) : 0, reg_path = nw16 != 0;
        BK_TRY(batch_scratch_or_release_swin(c, n, wpr, rd2w, ivc));
        BatchBufs &m = c->buf;
        l = PhaseLists{m.act[0].get(), m.act[1].get(), m.wave.get(), m.heavy.get(), nullptr, nullptr, {m.stage[0].get(), m.stage[1].get(), m.stage[2].get()}, m.stripe_cnt.get()};
        b = make_batch(c, in, first, n, wpr, ivc, d_out);
        b.rd2 = rd2w ? m.rd2.get() : nullptr;
        // (the wave list's job sizes come from k_flat only when every read on that list went through it)
        b.wave_work = (reg_path && c->cfg.heavy_thresh <= 100) ? m.wave_work.get() : nullptr;
        b.iv32 = (c->use_iv32 && c->ix.k2) ? m.iv32.get() : nullptr;      // (written by k_search_a_ilp and pass B in phase 0)
        b.nw = (uint32_t)nw16;                   // the fused prep kernel packs reads of the register-kernel path
        b.iv_stride = n;                         // interval records: a plane per (strand, core), a record per read of the chunk in each
        nstr = c->cfg.align_strand == 0 ? 2 : 1, lazy = (reg_path && c->lazy_search) ? 1 : 0;
        ctl = c->fixed.ctl.get();
        HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(PhaseCtl) * kCtlLines, s));
        BK_TRY(plan_table_for(c, maxlen, s));    // (make_plan / phase_params / core_offsets of every length and phase, kept between batches)
        b.plan = m.plan.get(), b.plan_stride = c->plan_maxlen + 1, b.plan_n = maxlen + 1;
        cb = chunk_bounds(c->h_plan.get(), b.plan_stride, maxlen);
        if (cb.max_phases > kMaxPhases) return BK_ERR_INTERNAL;
        no_readback = reg_path && main_path_common(c->use_wave != 0, c->cfg.heavy_thresh, c->ix.k2 != nullptr, c->debug, c->async_phases != 0) &&
                        cb.cores_fit && !c->params.best_matches;
        search0 = bk::prep_search0_on(c, reg_path, cb.cores_fit, cb.cmax_bound[0]);
        return BK_OK;
    }
    // pass B's work list for `lanes` items (growing it moves it), then - "iv_poison" - ones into the interval slots the phase of line
    // `cur` can use, so that a slot read without having been written shows (cur null: slots by read; skip: pass A has filled them)
    int slist_and_poison(uint64_t lanes, const PhaseCtl *cur, uint32_t n_bound, int cmax, bool skip)
    {
        const int rc = ensure_slist(c, lanes, s), as = c->cfg.align_strand;
        l.slist = c->buf.slist.get(), l.slist_stage = c->buf.slist_stage.get();
        if (!rc && !skip && c->iv_poison) launch_clear_iv(b, cur, n_bound, cmax, as == 2 ? 1 : 0, as == 1 ? 0 : 1, 0xFFFFFFFFu, s);
        return rc;
    }
    // the read preparation: rows, the first active list and its counts in ctl[0] - and phase 0's pass A where search0 says so
    int prepare_reads()
    {
        if (!tm.on) launch_max_len(b.lens, n, ctl_longest_read(ctl), s);
        b.iv_by_read = search0 ? 1u : 0u;
        if (search0) BK_TRY(slist_and_poison((uint64_t)n * (uint64_t)nstr, nullptr, n, 1, false));
        const PrepSearch0 ps0{&c->ix, lazy, l.slist, &ctl[0].n_slist, l.slist_stage};
        hipEvent_t e0 = tm.begin(s);
        launch_prep(c->cfg, b, l.act_in, &ctl[0].n_act, &ctl[0].cmax, l.stage[0], l.stripe_cnt, s, search0 ? &ps0 : nullptr);
        HIP_TRY(hipGetLastError());
        tm.end(Span::Prep, e0, s);
        return BK_OK;
    }
    // The counts of `phase` the host goes on with: behind the preparation (n_act, cmax of phase 0), behind pass A (n_slist), behind the
    // extension (n_wave, n_heavy), behind the wave and general kernels (n_act, cmax of the NEXT phase).  Without read-backs: the bounds of
    // the chunk's size and the plan table, sort_prefix's guess for a sort; else the lines read back (h_line), a sort takes the whole list.
    int phase_counts(int phase, Behind at, PhaseCounts &k)
    {
        if (no_readback) {
            if (at == Behind::Prep && c->ix.isa == nullptr) BK_TRY(size_heavy_scratch(c));      // the wave kernel's hash-set dedupe, sized before the schedule starts: nothing allocates or waits in the middle of it
            k.n_act = k.n_wave = n;                                // (any read of the chunk may still be active, and may go to the wave kernel)
            k.n_heavy = 0;                                           // (the core bound rules the general kernel out: take_phase_history checks)
            k.cmax = cb.cmax_bound[at == Behind::Wave ? phase + 1 : phase];
            k.n_slist = (uint64_t)n * (uint64_t)(k.cmax * nstr);
            const uint64_t cap = c->buf.sort[2].cap();               // (no growing - it waits for the stream - for a guess)
            if (at == Behind::PassA) k.sort_slist = sort_prefix(c->hist_valid, c->hist_slist[phase], 0.30, n, k.n_slist, cap, kSortCeiling);
            if (at == Behind::Extend) k.sort_wave = sort_prefix(c->hist_valid, c->hist_wave[phase], 0.25, n, k.n_wave, cap, kNoCeiling);
            return BK_OK;
        }
        PhaseCtl *h = c->h_line.get();                               // h[0]: this phase, h[1]: the next
        if (at == Behind::PassA) {
            HIP_TRY(hipMemcpyAsync(&h[0].n_slist, &ctl[phase].n_slist, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            k.n_slist = h[0].n_slist;
            k.sort_slist = h[0].n_slist >= 4096 ? h[0].n_slist : 0;
            return BK_OK;
        }
        if (at != Behind::Wave || k.n_wave || k.n_heavy) {           // (behind kernels that did not run the lines are as the extension left them)
            HIP_TRY(hipMemcpyAsync(h, ctl + phase, 2 * sizeof(PhaseCtl), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        if (at == Behind::Extend) {
            k.n_heavy = h[0].n_heavy, k.n_wave = h[0].n_wave;
            k.sort_wave = k.n_wave >= 4096 ? k.n_wave : 0;
            return BK_OK;
        }
        if (at == Behind::Wave && c->debug)
            fprintf(stderr, "bk: phase %d n_act %u cmax %d n_heavy %u n_wave %u -> next n_act %u cmax %u\n", phase, k.n_act, k.cmax, k.n_heavy, k.n_wave, h[1].n_act, h[1].cmax);
        k.n_act = h[at == Behind::Wave].n_act, k.cmax = (int)h[at == Behind::Wave].cmax;
        return BK_OK;
    }
    // The search of a phase - LocateFirstExact / LocateLastExact of every core of every active read, into the interval records.  With
    // second-level keys: pass A (unless the preparation ran it), pass B's work list grouped by k-mer bucket, pass B; else one kernel.
    int search_phase(int phase, PhaseCounts &k)
    {
        PhaseCtl *cur = ctl + phase;
        if (k.cmax <= 0) return BK_OK;
        hipEvent_t e1 = tm.begin(s);
        if (c->ix.k2) {
            // (the interval records are not cleared: launch_clear_iv, bk_search.hip)
            BK_TRY(slist_and_poison((uint64_t)k.n_act * (uint64_t)(k.cmax * nstr), cur, k.n_act, k.cmax, b.iv_by_read != 0));
            if (!b.iv_by_read) {                     // (by read: pass A of this phase ran inside the read preparation)
                hipEvent_t ea = tm.begin(s);
                launch_search_a(c->ix, c->cfg, b, l, cur, k.n_act, phase, k.cmax, nstr, lazy, s);
                HIP_TRY(hipGetLastError());
                tm.end(Span::SearchA, ea, s);
            }
            BK_TRY(phase_counts(phase, Behind::PassA, k));
            const uint32_t *sorted = nullptr;
            const uint32_t n_sort = (c->sort_lists & 1) ? k.sort_slist : 0;
            if (n_sort) {
                BK_TRY(ensure_sort_scratch(c, n_sort, s));
                hipEvent_t es = tm.begin(s);
                launch_keys_search(b, l, cur, n_sort, c->sort_shift, c->buf.sort[0].get(), s);
                BK_TRY(sort_work(c, l.slist, n_sort, s, &sorted));
                tm.end(Span::SearchSort, es, s);
            }
            if (k.n_slist) {
                // ("search_split": a second, dense launch finishes the items the key levels do not settle - launch_search_b; both are pass B's time)
                hipEvent_t eb = tm.begin(s);
                launch_search_b(c->ix, c->cfg, b, l, cur, phase, lazy, sorted, n_sort, k.n_slist, bk::search_split_on(c), s);
                tm.end(Span::SearchB, eb, s);
            }
        } else
            launch_search(c->ix, c->cfg, b, l.act_in, k.n_act, phase, k.cmax, nstr, lazy, s);
        HIP_TRY(hipGetLastError());
        tm.end(Span::Search, e1, s);
        return BK_OK;
    }
    // The extension of a phase: k_flat on the register-window path, else the lane-per-read kernel.  5-byte indexes: the reference's seen-target set is keyed by the target start truncated to 32 bits (SfxArrayV2.cpp:5932), a rule that
    // depends on every earlier candidate of the strand pass.  k_flat and the hash-set kernels reproduce it; the lane-per-read kernels
    // dedupe on exact starts, so on an index of more than 2^32 bases they only finish the calls without candidates and hand every other
    // one to the hash-set kernels.
    int extend_phase(int phase, const PhaseCounts &k)
    {
        PhaseCtl *cur = ctl + phase;
        DevAlignCfg cfg_lane = c->cfg;
        if (c->ix.n > (1ULL << 32)) cfg_lane.heavy_thresh = 0;            // (below that the truncated keys are the exact ones)
        hipEvent_t e2 = tm.begin(s);
        if (k.n_act == 0) {}
        else if (reg_path && c->cfg.heavy_thresh <= 100)
            launch_flat(c->ix, c->cfg, b, l, cur, cur + 1, k.n_act, phase, nstr * std::max(k.cmax, 1), nw16, s);
        else
            launch_extend(c->ix, cfg_lane, b, l, cur, cur + 1, k.n_act, phase, s);
        HIP_TRY(hipGetLastError());
        tm.end(Span::Extend, e2, s);
        return BK_OK;
    }
    // the reads the extension handed on: the wave kernel over its list (sorted by index position or job size where that pays), the general kernel over its own
    int wave_phase(int phase, const PhaseCounts &k)
    {
        PhaseCtl *cur = ctl + phase;
        if (k.n_wave) {
            hipEvent_t e3 = tm.begin(s);
            const uint32_t *wsorted = nullptr;
            const uint32_t n_sort = (c->sort_lists & 2) ? k.sort_wave : 0;
            if (n_sort) {
                BK_TRY(ensure_sort_scratch(c, n_sort, s));
                launch_keys_wave(c->cfg, b, phase, l, cur, n_sort, (c->sort_lists & 4) ? -1 : c->sort_shift, c->buf.sort[0].get(), b.wave_work, s);
                BK_TRY(sort_work(c, l.wave, n_sort, s, &wsorted));
            }
            if (c->ix.isa == nullptr) BK_TRY(size_heavy_scratch(c));      // hash-set dedupe (where no count is read back: sized already, nothing to do)
            launch_wave(c->ix, c->cfg, b, c->hs, l, cur, cur + 1, wsorted, n_sort, k.n_wave, phase, nw16, c->wave_waves,
                        c->wave_len_spec ? uniform_dwords(minlen, maxlen) : 0, s);
            HIP_TRY(hipGetLastError());
            tm.end(Span::Heavy, e3, s);
        }
        if (k.n_heavy) {
            hipEvent_t e3 = tm.begin(s);
            BK_TRY(size_heavy_scratch(c));
            launch_heavy(c->ix, c->cfg, b, c->hs, l, cur, cur + 1, k.n_heavy, phase, s);
            HIP_TRY(hipGetLastError());
            tm.end(Span::Heavy, e3, s);
        }
        return BK_OK;
    }
    // test hook, bk_debug_intervals: the interval records the search of `phase` wrote stay where they are; nothing of the phase's extension
    // or of the phases behind it runs, so the batch's result records are not to be used
    void debug_stop(int phase, bool by_read)
    {
        c->dbg_n = n; c->dbg_ivc = b.iv_cores; c->dbg_cur = act_cur; c->dbg_phase = phase; c->dbg_by_read = by_read; c->dbg_valid = true;
    }
    // AlignReads' branches for what is still unaligned (SfxArrayV2.cpp:7722-7757): microInDels, then splice junctions, then the chimeric
    // (end-trimmed) placement; the chunk's second segments appended to the context's
    int second_segments()
    {
        const bk_align_params &p = c->params;
        uint32_t *sm = c->fixed.small.get(), *hm = c->h_small.get(), *list = c->buf.act[0].get();      // (the phase work lists are free by now)
        hipEvent_t ei = tm.begin(s);
        BK_TRY(ensure_seg2(c, n));
        bk_seg2 *d_seg2 = c->buf.seg2.get();
        hipError_t eh = clear_dev(d_seg2, (size_t)n * sizeof(bk_seg2), s);
        int rc2 = BK_OK;
        if (eh == hipSuccess && (p.micro_indel_len > 0 || p.splice_junct_len > 0)) {
            eh = hipMemsetAsync(sm, 0, kSmallWords * 4, s);
            if (eh == hipSuccess) {
                launch_indel(c->ix, c->cfg, b, n, p.micro_indel_len, p.splice_junct_len, p.min_chimeric_len > 0 ? 1 : 0, list, sm + kSmCount, hm + kSmCount, sm + kSmCursor, d_seg2, s);
                eh = hipGetLastError();
            }
        }
        if (eh == hipSuccess && p.min_chimeric_len > 0 && (rc2 = size_heavy_scratch(c)) == BK_OK) {
            eh = hipMemsetAsync(sm, 0, kSmallWords * 4, s);
            if (eh == hipSuccess) {
                launch_unaligned_list(b.out, n, list, sm + kSmCount, s);
                eh = hipMemcpyAsync(hm + kSmCount, sm + kSmCount, 4, hipMemcpyDeviceToHost, s);
            }
            if (eh == hipSuccess) eh = hipStreamSynchronize(s);
            if (eh == hipSuccess && hm[kSmCount]) {
                launch_chimeric(c->ix, c->cfg, b, c->hs, list, hm[kSmCount], p.min_chimeric_len, maxlen > 512 ? 1 : 0, sm + kSmCursor, d_seg2, s);
                eh = hipGetLastError();
            }
        }
        const size_t at = c->seg2.size();
        c->seg2.resize(at + n);
        if (eh == hipSuccess && rc2 == BK_OK) eh = hipMemcpyAsync(c->seg2.data() + at, d_seg2, (size_t)n * sizeof(bk_seg2), hipMemcpyDeviceToHost, s);
        if (eh == hipSuccess) eh = hipStreamSynchronize(s);
        if (rc2 != BK_OK) return rc2;
        if (eh != hipSuccess) return BK_ERR_INTERNAL;
        if (p.min_chimeric_len > 0 && c->cfg.max_hits > 1)          // (the chimeric call's note to the loci replay, see k_heavy)
            for (size_t i = at; i < at + n; i++)
                if (c->seg2[i].flags == 0x40) c->seg2[i] = bk_seg2{};
        tm.end(Span::Heavy, ei, s);
        return BK_OK;
    }
};

// One chunk of reads through AlignReads' schedule, until no read is active - or, where no count is read back, for as many
// phases as a read of maxlen bases can have
int align_chunk(bk_ctx *c, const DevReads &in, uint32_t first, uint32_t n, uint32_t maxlen, uint32_t minlen, bk_hit *d_out, hipStream_t s, EvTimer &tm)
{
    HIP_TRY(hipMemsetAsync(c->fixed.small.get(), 0, kSmallWords * 4, s));
    ChunkRun r{c, s, tm, n, maxlen, minlen};
    BK_TRY(r.chunk_setup(in, first, d_out));
    BK_TRY(r.prepare_reads());
    PhaseCounts k;
    BK_TRY(r.phase_counts(0, Behind::Prep, k));
    if (c->params.best_matches) {
        hipEvent_t eb = tm.begin(s);
        BK_TRY(best_matches_chunk(c, r.b, n, r.l.act_in, k.n_act, s));
        tm.end(Span::Heavy, eb, s);
        k.n_act = 0;
    }
    for (int phase = 0; r.no_readback ? phase < r.cb.max_phases : k.n_act > 0; phase++) {
        static_assert((kMaxPhases - 1) + 1 < kCtlBatchLine && kCtlBatchLine + 1 == kCtlLines, "line phase + 1 of the last phase, kMaxPhases - 1 by the guard below, lies below the batch's line, the array's last");
        r.b.act = r.l.act_in;
        r.b.iv_by_read = (r.search0 && phase == 0) ? 1u : 0u;      // (pass A ran inside the read preparation; every later phase: by position in its active list)
        BK_TRY(r.search_phase(phase, k));
        if (phase == c->dbg_stop_phase) { r.debug_stop(phase, r.b.iv_by_read != 0); break; }
        BK_TRY(r.extend_phase(phase, k));
        BK_TRY(r.phase_counts(phase, Behind::Extend, k));
        BK_TRY(r.wave_phase(phase, k));
        BK_TRY(r.phase_counts(phase, Behind::Wave, k));
        std::swap(r.l.act_in, r.l.act_out), r.act_cur ^= 1;
        if (phase + 1 > kMaxPhases - 1) return BK_ERR_INTERNAL;
    }
    if (c->dbg_stop_phase >= 0 && !c->dbg_valid) r.debug_stop(kMaxPhases, false);       // (no read reached that phase: an empty list - ctl[kMaxPhases] is never written)
    if (r.no_readback) {
        // what the phases needed goes to the host on its own time: the next chunk's sort sizes, reads left for the general kernel (take_phase_history)
        HIP_TRY(hipMemcpyAsync(c->h_ctl.get(), r.ctl, sizeof(PhaseCtl) * kCtlLines, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(c->ev_ctl, s));
        c->ctl_pending = true, c->ctl_pending_reads = n, c->ctl_pending_phases = r.cb.max_phases, c->ctl_pending_maxlen = tm.on ? 0 : maxlen;
    }
    if (c->params.micro_indel_len > 0 || c->params.splice_junct_len > 0 || c->params.min_chimeric_len > 0) BK_TRY(r.second_segments());
    hipEvent_t e4 = tm.begin(s);
    launch_count_seqs(d_out, n, c->image.id2idx.get(), c->ix.n_ent, c->fixed.seq_counts.get(), s);
    HIP_TRY(hipGetLastError());
    tm.end(Span::Other, e4, s);
    if (c->cfg.max_hits > 1 && !c->params.best_matches) return collect_loci(c, r.b, n, maxlen, s);
    return BK_OK;
}


// What the last chunk that ran without read-backs needed, once its counts have arrived in h_ctl (the copy was enqueued behind its
// kernels): work items of pass B and reads for the wave kernel per phase, as fractions of the chunk - the sizes of the next chunk's
// sorts.  wait: block until they are there.  A read on a general-kernel list would mean the core bound of align_chunk was wrong.
int take_phase_history(bk_ctx *c, bool wait)
{
    if (!c->ctl_pending) return BK_OK;
    if (wait) HIP_TRY(bk::wait_event(c->ev_ctl));
    else if (hipEventQuery(c->ev_ctl) != hipSuccess) { (void)hipGetLastError(); return BK_OK; }
    c->ctl_pending = false;
    PhaseCtl *h = c->h_ctl.get();
    const double n = (double)std::max<uint32_t>(c->ctl_pending_reads, 1);
    for (int ph = 0; ph < kMaxPhases; ph++) {
        c->hist_slist[ph] = ph < c->ctl_pending_phases ? (double)h[ph].n_slist / n : 0.0;
        c->hist_wave[ph] = ph < c->ctl_pending_phases ? (double)h[ph].n_wave / n : 0.0;
        if (h[ph].n_heavy) {
            fprintf(stderr, "biokanga_amd: %u reads of phase %d were left for the general kernel by a schedule that does not run it\n", h[ph].n_heavy, ph);
            c->async_error = BK_ERR_INTERNAL;
        }
    }
    // (bk_align_batch_device_async: the longest read its caller promised against the longest the batch really held)
    if (c->ctl_pending_maxlen && *ctl_longest_read(h) > c->ctl_pending_maxlen) {
        fprintf(stderr, "biokanga_amd: a batch held a read of %u bases, its caller had promised at most %u\n", *ctl_longest_read(h), c->ctl_pending_maxlen);
        c->async_error = BK_ERR_PARAMS;
    }
    c->hist_valid = true;
    if (c->async_error && wait) { const int e = c->async_error; c->async_error = 0; return e; }
    return BK_OK;
}

// enqueue_only: everything is launched on `s` and the call returns without waiting for any of it (bk_align_batch_device_async): the
// caller has named the longest read, the scratch is in place (bk_ctx_reserve) and the configuration is one whose phase loop reads
// nothing back - else BK_ERR_PARAMS, before anything is launched.
int align_device(bk_ctx *c, const DevReads &in, uint32_t nreads, bk_hit *d_out, hipStream_t s, uint32_t maxlen_known, bool enqueue_only, uint32_t minlen_known)
{
    grow_tick(c, nreads);                      // (BK_CTX_GROW_IMAGE: the long-run tables are started, or taken in, between batches)
    const uint32_t *d_lens = in.lens;
    if (enqueue_only) {
        const uint32_t ml = maxlen_known;
        const bool plain = c->cfg.max_hits == 1 && !c->params.best_matches && !c->params.micro_indel_len && !c->params.splice_junct_len && !c->params.min_chimeric_len;
        const bool fits = ml >= 1 && window_words_for(ml) != 0 && nreads <= c->cap_reads && nreads <= c->chunk_reads && words_per_read(ml) <= c->cap_wpr &&
                          iv_cores_for(c, ml) <= c->cap_iv_cores && rd2w_for(ml) <= c->cap_rd2w &&
                          (uint64_t)nreads * iv_cores_for(c, ml) * (c->cfg.align_strand == 0 ? 2u : 1u) <= c->buf.slist.cap() && (c->ix.isa != nullptr || c->hs.htab != nullptr) &&
                          plan_table_covers(c, ml);         // (made by bk_ctx_reserve; making it here would allocate and wait)
        const bool main_path = main_path_common(c->use_wave != 0, c->cfg.heavy_thresh, c->ix.k2 != nullptr, c->debug, c->async_phases != 0) && c->ix.tgt2 != nullptr;
        if (!plain || !fits || !main_path) return BK_ERR_PARAMS;
    }
    EvTimer tm{c};
    tm.on = !enqueue_only;
    hipEvent_t t0 = tm.begin(s);
    c->loci_offs.clear();
    c->loci.clear();
    c->loci_trims.clear();
    c->seg2.clear();
    // longest read of the call -> row width of the packed reads and the kernel family used (the pipeline knows it already)
    // .. and the shortest beside it, where the caller has looked or this call looks anyway: 0, not known, for a call that only enqueues
    uint32_t maxlen = maxlen_known, minlen = maxlen_known ? minlen_known : 0;
    if (!maxlen) {
        HIP_TRY(hipMemsetAsync(c->fixed.small.get(), 0, kSmallWords * 4, s));
        launch_max_len(d_lens, nreads, c->fixed.small.get() + kSmMaxLen, s);
        launch_min_len(d_lens, nreads, c->fixed.small.get() + kSmMinLenInv, s);
        HIP_TRY(hipMemcpyAsync(c->h_small.get(), c->fixed.small.get(), kSmallWords * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        maxlen = c->h_small.get()[kSmMaxLen];
        minlen = min_len_of(c->h_small.get()[kSmMinLenInv]);
    }
    if (maxlen > (uint32_t)kMaxReadLenAbs) return BK_ERR_PARAMS;
    c->last_maxlen = maxlen;
    (void)take_phase_history(c, false);
    if ((int)maxlen > c->max_read_len) {
        c->max_read_len = (int)maxlen;
    }
    if (!enqueue_only) { int rw = maybe_build_swin(c, maxlen, nreads, s); if (rw) return rw; }      // (the window array is used when it is there)
    // chunk size: as many reads as the knob allows and as fit in about half of the HBM still free
    // (the phase kernels run better the more reads they see: fewer launches, shorter tails)
    uint32_t chunk = c->chunk_reads;
    // (a batch the scratch already holds needs no look at the free memory)
    if (!(std::min(chunk, nreads) <= c->cap_reads && words_per_read(maxlen) <= c->cap_wpr && iv_cores_for(c, maxlen) <= c->cap_iv_cores &&
          rd2w_for(maxlen) <= std::max(c->cap_rd2w, 1u) && !c->params.best_matches)) {
        const uint64_t per_read = scratch_bytes_per_read(words_per_read(maxlen), rd2w_for(maxlen), iv_cores_for(c, maxlen));
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const uint64_t have = (uint64_t)c->cap_reads * scratch_bytes_per_read(c->cap_wpr, c->cap_rd2w, c->cap_iv_cores);
        uint64_t fit = ((uint64_t)free_b + have) / 4 * 3 / per_read;
        if (fit < 65536) fit = 65536;
        if (fit < chunk) chunk = (uint32_t)fit;
        if (chunk > (1u << 27)) chunk = 1u << 27;       // 32 interval slots per read are indexed with 32 bits
        if (c->params.best_matches) {                   // dense rows of MaxHits loci per read: keep them within 4 GB
            const uint64_t lim = std::max<uint64_t>(1024, (4ULL << 30) / (sizeof(bk_loci) * (uint64_t)c->cfg.max_hits));
            if (lim < chunk) chunk = (uint32_t)lim;
        }
    }
    for (uint32_t done = 0; done < nreads;) {
        uint32_t n = std::min(chunk, nreads - done);
        BK_TRY(align_chunk(c, in, done, n, maxlen, minlen, d_out + done, s, tm));
        done += n;
    }
    if (enqueue_only) return BK_OK;          // (the chunk's counts reach the host behind its kernels: take_phase_history of the next call)
    hipEvent_t t1 = tm.begin(s);
    HIP_TRY(bk::wait_stream(s, c->ev_wait));             // (asleep: the caller's thread leaves its CPU to others meanwhile)
    BK_TRY(take_phase_history(c, true));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, t0, t1);
    c->timing.ms_total += ms;
    for (auto &sp : tm.spans) {
        float m = 0;
        (void)hipEventElapsedTime(&m, sp.second.first, sp.second.second);
        switch (sp.first) {
        case Span::Search: c->timing.ms_search += m; c->timing.n_search_launches++; break;
        case Span::Extend: c->timing.ms_extend += m; c->timing.n_extend_launches++; break;
        case Span::Heavy: c->timing.ms_heavy += m; c->timing.n_heavy_launches++; break;
        case Span::SearchA: c->timing.ms_search_a += m; break;           // (inside a span of Span::Search)
        case Span::SearchSort: c->timing.ms_search_sort += m; break;
        case Span::SearchB: c->timing.ms_search_b += m; c->timing.n_search_b_launches++; break;
        case Span::Prep: c->timing.ms_prep += m; c->timing.ms_other += m; break;
        case Span::Other: c->timing.ms_other += m; break;
        }
    }
    return BK_OK;
}


}  // namespace bk

using namespace bk;

int bk::engine_align_device(bk_ctx *c, const DevReads &in, uint32_t nreads, bk_hit *d_out, hipStream_t s, uint32_t maxlen_known, uint32_t minlen_known)
{
    return align_device(c, in, nreads, d_out, s, maxlen_known, false, minlen_known);
}

namespace {
struct CastU64 {
    __host__ __device__ unsigned long long operator()(const uint32_t &v) const { return (unsigned long long)v; }
};
}

int bk::engine_prepare_packed(bk_ctx *c, const uint16_t *d_lens16, uint32_t nreads, uint64_t n_words, const bk_nbase *d_exc, uint64_t n_exc,
                              uint32_t *d_lens32, uint64_t *d_offs, uint32_t *maxlen, uint32_t *minlen, hipStream_t s)
{
    // words per read -> exclusive scan in place = first word of every read
    launch_widen_lens(d_lens16, nreads, d_lens32, (unsigned long long *)d_offs, s);
    HIP_TRY(hipGetLastError());
    size_t need = 0;
    HIP_TRY(bk::prim::exclusive_sum(nullptr, need, (unsigned long long *)d_offs, (unsigned long long *)d_offs, (size_t)nreads, s));
    if (need > c->buf.scan_tmp.cap()) {
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(c->buf.scan_tmp.ensure(need + 256));
    }
    size_t tb = c->buf.scan_tmp.cap();
    HIP_TRY(bk::prim::exclusive_sum(c->buf.scan_tmp.get(), tb, (unsigned long long *)d_offs, (unsigned long long *)d_offs, (size_t)nreads, s));
    // [0] max over reads of (first word + words) = the batch's word count, [1] longest read; exceptions in range and ascending; [3] shortest read (launch_min_len's word)
    HIP_TRY(hipMemsetAsync(c->fixed.ctr_aux.get(), 0, 32, s));
    launch_packed_extent(d_offs, d_lens32, nreads, c->fixed.ctr_aux.get(), s);
    launch_check_exc(d_exc, n_exc, d_lens32, nreads, reinterpret_cast<uint32_t *>(c->fixed.ctr_aux.get() + 2), s);
    launch_min_len(d_lens32, nreads, reinterpret_cast<uint32_t *>(c->fixed.ctr_aux.get() + 3), s);
    HIP_TRY(hipGetLastError());
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, c->fixed.ctr_aux.get(), 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h[0] != n_words || h[1] > (unsigned long long)kMaxReadLenAbs || (uint32_t)h[2] != 0) return BK_ERR_PARAMS;
    *maxlen = (uint32_t)h[1];
    *minlen = min_len_of((uint32_t)h[3]);
    return BK_OK;
}

// ------------------------------------------------------------------------------------------------
// K4 on buffers resident in HBM (shared by bk_pair_batch, bk_pair_batch_device and the stream pipeline).  seg2_host / seg2_dev: the
// bk_seg2 records of these reads (one of the two, or neither) - required when the context trims chimeric reads (-c), whose pair rules
// look at the trimmed loci and whose orphan recovery may place the partner end-trimmed; updated in place
int bk::engine_pair_device(bk_ctx *c, const DevReads &in, uint32_t n_pairs, bk_hit *d_hits, uint32_t maxlen, const bk_pe_params *pe, hipStream_t s,
                           bk_seg2 *seg2_host, bk_seg2 *seg2_dev)
{
    const uint32_t nreads = 2 * n_pairs;
    const uint32_t wpr = words_per_read(maxlen);
    // (launch_pe never touches the interval records: the slots keep whatever core count the SE pass sized them for)
    const uint32_t ivc = c->cap_iv_cores ? c->cap_iv_cores : iv_cores_for(c, maxlen);
    BK_TRY(batch_scratch_or_release_swin(c, nreads, wpr, 0, ivc));
    const DevBatch b = make_batch(c, in, 0, nreads, wpr, c->cap_iv_cores, d_hits);
    if (c->params.min_chimeric_len > 0 && !seg2_host && !seg2_dev) return BK_ERR_PARAMS;
    bk_seg2 *d_seg2 = seg2_dev;
    if (!d_seg2 && seg2_host) {
        BK_TRY(ensure_seg2(c, nreads));
        d_seg2 = c->buf.seg2.get();
        HIP_TRY(hipMemcpyAsync(d_seg2, seg2_host, (size_t)nreads * sizeof(bk_seg2), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemsetAsync(c->fixed.small.get(), 0, kSmallWords * 4, s));
    launch_pe(c->ix, c->cfg, b, pe->pe_mode, pe->pair_min_len, pe->pair_max_len, pe->pair_strand ? 1 : 0, d_hits, n_pairs,
              c->buf.heavy.get(), c->fixed.small.get() + kSmCount, c->h_small.get() + kSmCount, d_seg2, c->params.min_chimeric_len, maxlen > 512 ? 1 : 0, c->buf.chrom_accept.get(), c->n_chrom_accept, s);
    HIP_TRY(hipGetLastError());
    if (seg2_host && !seg2_dev) HIP_TRY(hipMemcpyAsync(seg2_host, d_seg2, (size_t)nreads * sizeof(bk_seg2), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return BK_OK;
}


extern "C" {


int bk_batch_seg2(bk_ctx *c, const bk_seg2 **seg2, uint64_t *n)
{
    if (!c || !seg2 || !n) return BK_ERR_PARAMS;
    *seg2 = c->seg2.empty() ? nullptr : c->seg2.data();
    *n = c->seg2.size();
    return BK_OK;
}

int bk_batch_loci(bk_ctx *c, const uint64_t **offs, const bk_loci **loci, uint64_t *n_loci)
{
    if (!c || !offs || !loci || !n_loci) return BK_ERR_PARAMS;
    if (c->loci_offs.empty()) { *offs = nullptr; *loci = nullptr; *n_loci = 0; return BK_OK; }
    *offs = c->loci_offs.data();
    *loci = c->loci.data();
    *n_loci = c->loci.size();
    return BK_OK;
}

int bk_batch_loci_trims(bk_ctx *c, const bk_loci_trims **trims, uint64_t *n_loci)
{
    if (!c || !trims || !n_loci) return BK_ERR_PARAMS;
    *trims = c->loci_trims.empty() ? nullptr : c->loci_trims.data();
    *n_loci = c->loci_trims.size();
    return BK_OK;
}


const char *bk_version(void) { return "biokanga_amd 0.1 (gfx950; reference biokanga 4.4.2)"; }

const char *bk_strerror(int rc)
{
    switch (rc) {
    case BK_OK: return "success";
    case BK_ERR_INTERNAL: return "internal processing error (HIP failure or inconsistency)";
    case BK_ERR_NODEVICE: return "no usable HIP device - this library has no CPU fallback";
    case BK_ERR_PARAMS: return "parameter error";
    case BK_ERR_MEM: return "unable to allocate memory";
    case BK_ERR_NOTBIOSEQ: return "file exists but is not a biokanga suffix array file";
    case BK_ERR_OPNFILE: return "unable to open file";
    case BK_ERR_CREATEFILE: return "unable to create file";
    case BK_ERR_FILEVER: return "file version error";
    case BK_ERR_FILEACCESS: return "file access (seek/read/write) failed";
    default: return "error";
    }
}

int bk_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}


int bk_align_batch_device(bk_ctx *c, const void *d_bases, const void *d_offs, const void *d_lens, uint32_t nreads,
                          void *d_out, void *stream, int sync)
{
    (void)sync;   // the phase loop reads active counts back, so the call always completes before returning
    if (!c || (nreads && (!d_bases || !d_offs || !d_lens || !d_out))) return BK_ERR_PARAMS;
    if (!nreads) return BK_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    DevReads in;
    in.bases = (const uint8_t *)d_bases; in.offs = (const uint64_t *)d_offs; in.lens = (const uint32_t *)d_lens;
    return align_device(c, in, nreads, (bk_hit *)d_out, s);
}

int bk_align_batch_device_async(bk_ctx *c, const void *d_bases, const void *d_offs, const void *d_lens, uint32_t nreads, uint32_t max_read_len,
                                void *d_out, void *stream)
{
    if (!c || !max_read_len || (nreads && (!d_bases || !d_offs || !d_lens || !d_out))) return BK_ERR_PARAMS;
    if (!nreads) return BK_OK;
    HIP_TRY(hipSetDevice(c->device));
    BK_TRY(take_phase_history(c, false));       // (also: what an earlier call of this kind found wrong with its batch)
    if (c->async_error) { const int e = c->async_error; c->async_error = 0; return e; }
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    DevReads in;
    in.bases = (const uint8_t *)d_bases; in.offs = (const uint64_t *)d_offs; in.lens = (const uint32_t *)d_lens;
    return align_device(c, in, nreads, (bk_hit *)d_out, s, max_read_len, true);
}

int bk_align_batch(bk_ctx *c, const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint32_t nreads, bk_hit *out)
{
    if (!c || (nreads && (!bases || !offs || !lens || !out))) return BK_ERR_PARAMS;
    if (!nreads) return BK_OK;
    HIP_TRY(hipSetDevice(c->device));
    HostExtent x;
    DevReads in;
    BK_TRY(stage_host_batch(c, bases, offs, lens, nreads, x, in));
    HIP_TRY(hipStreamSynchronize(c->stream));
    bk_hit *d_out = c->buf.in_out.get();
    BK_TRY(align_device(c, in, nreads, d_out, c->stream));
    HIP_TRY(hipMemcpy(out, d_out, (size_t)nreads * sizeof(bk_hit), hipMemcpyDeviceToHost));
    return BK_OK;
}

uint64_t bk_packed_words(const uint32_t *lens, uint32_t nreads)
{
    uint64_t n = 0;
    if (lens) for (uint32_t i = 0; i < nreads; i++) n += ((uint64_t)lens[i] + 15) >> 4;
    return n;
}

namespace {
// 16 bases (bytes, bits 0-2 = the code) -> one packed word, when none of them is above 3: the two low bits of every byte gathered with the
// bit-extract instruction (first base into the top bits: the bytes are swapped first).  *clean = every code was 0..3.
__attribute__((target("bmi2"))) inline uint32_t pack16_bmi2(const uint8_t *s, bool *clean)
{
    uint64_t a, b;
    memcpy(&a, s, 8);
    memcpy(&b, s + 8, 8);
    *clean = ((a | b) & 0x0404040404040404ULL) == 0;
    const uint64_t m = 0x0303030303030303ULL;
    return (uint32_t)(__builtin_ia32_pext_di(__builtin_bswap64(a), m) << 16) | (uint32_t)__builtin_ia32_pext_di(__builtin_bswap64(b), m);
}
inline uint32_t pack16_plain(const uint8_t *s, bool *clean)
{
    uint32_t v = 0, bad = 0;
    for (uint32_t k = 0; k < 16; k++) { const uint32_t code = s[k] & 7u; bad |= code & 4u; v |= (code & 3u) << (30 - 2 * k); }
    *clean = bad == 0;
    return v;
}
}  // namespace

int bk_pack_reads(const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint32_t nreads, uint32_t *words, uint16_t *lens16,
                  bk_nbase *exc, uint64_t exc_cap, uint64_t *n_exc)
{
    static const bool have_bmi2 = __builtin_cpu_supports("bmi2");
    if (!n_exc || (nreads && (!bases || !lens || !words || !lens16)) || (exc_cap && !exc)) return BK_ERR_PARAMS;
    *n_exc = 0;
    if (!nreads) return BK_OK;
    // slices of reads, one thread each: first word and first base of every slice, then pack; exceptions are collected per slice
    // and laid behind each other afterwards (ascending by read and position as the slices are)
    unsigned nt = (unsigned)std::max(1, std::min(16, bk::effective_cpus()));         // (affinity mask and cgroup quota, not the host's hardware threads)
    if (nreads < 65536) nt = 1;
    std::vector<uint64_t> w0(nt + 1, 0), b0(nt + 1, 0);
    std::vector<uint32_t> r0(nt + 1);
    for (unsigned t = 0; t <= nt; t++) r0[t] = (uint32_t)((uint64_t)nreads * t / nt);
    bool too_long = false;
    {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++)
            th.emplace_back([&, t]() {
                uint64_t w = 0, bsum = 0;
                for (uint32_t i = r0[t]; i < r0[t + 1]; i++) { w += ((uint64_t)lens[i] + 15) >> 4; bsum += lens[i]; if (lens[i] > (uint32_t)kMaxReadLenAbs) too_long = true; }
                w0[t + 1] = w;
                b0[t + 1] = bsum;
            });
        for (auto &x : th) x.join();
    }
    if (too_long) return BK_ERR_PARAMS;
    for (unsigned t = 0; t < nt; t++) { w0[t + 1] += w0[t]; b0[t + 1] += b0[t]; }
    std::vector<std::vector<bk_nbase>> found(nt);
    {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++)
            th.emplace_back([&, t]() {
                uint32_t *wp = words + w0[t];
                uint64_t at = b0[t];
                for (uint32_t i = r0[t]; i < r0[t + 1]; i++) {
                    const uint32_t len = lens[i];
                    const uint8_t *s = bases + (offs ? offs[i] : at);
                    at += len;
                    lens16[i] = (uint16_t)len;
                    for (uint32_t j0 = 0; j0 < len; j0 += 16) {
                        const uint32_t cnt = std::min<uint32_t>(16, len - j0);
                        if (cnt == 16) {                       // a whole word of a, c, g, t: sixteen bytes at once
                            bool clean;
                            const uint32_t w16 = have_bmi2 ? pack16_bmi2(s + j0, &clean) : pack16_plain(s + j0, &clean);
                            if (clean) { *wp++ = w16; continue; }
                        }
                        uint32_t v = 0;
                        for (uint32_t k = 0; k < cnt; k++) {
                            const uint32_t code = s[j0 + k] & 7u;
                            if (code > 3) {
                                std::vector<bk_nbase> &f = found[t];
                                if (!f.empty() && f.back().read == i && f.back().code == code && f.back().run < 255 &&
                                    (uint32_t)f.back().pos + f.back().run + 1 == j0 + k)
                                    f.back().run++;
                                else
                                    f.push_back(bk_nbase{i, (uint16_t)(j0 + k), (uint8_t)code, 0});
                            } else
                                v |= code << (30 - 2 * k);
                        }
                        *wp++ = v;
                    }
                }
            });
        for (auto &x : th) x.join();
    }
    uint64_t total = 0;
    for (unsigned t = 0; t < nt; t++) {
        for (const bk_nbase &e : found[t]) { if (total < exc_cap) exc[total] = e; total++; }
    }
    *n_exc = total;
    return total > exc_cap ? BK_ERR_MEM : BK_OK;
}

int bk_align_batch_packed(bk_ctx *c, const uint32_t *words, uint64_t n_words, const uint16_t *lens, uint32_t nreads, const bk_nbase *exc,
                          uint64_t n_exc, bk_hit *out)
{
    if (!c || (nreads && (!lens || !out)) || (n_words && !words) || (n_exc && !exc)) return BK_ERR_PARAMS;
    if (!nreads) return BK_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    // (k_prep_fused<NW, PACKED> loads NW words from a read's first one whatever its length - up to kNwLongest for a batch whose
    // longest read has 257 .. 512 bases - so the buffer is padded by that many words behind the last read)
    static_assert(kPackedPadWords >= kNwLongest, "packed read words must be padded by the widest register-window family");
    BatchBufs &m = c->buf;
    HIP_TRY(m.in_words.ensure(n_words + kPackedPadWords));
    HIP_TRY(m.in_exc.ensure(n_exc));
    BK_TRY(ensure_in_reads(c, nreads, true));
    if (n_words) HIP_TRY(hipMemcpyAsync(m.in_words.get(), words, n_words * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(m.in_lens16.get(), lens, (size_t)nreads * 2, hipMemcpyHostToDevice, s));
    if (n_exc) HIP_TRY(hipMemcpyAsync(m.in_exc.get(), exc, n_exc * sizeof(bk_nbase), hipMemcpyHostToDevice, s));
    uint32_t maxlen = 0, minlen = 0;
    BK_TRY(engine_prepare_packed(c, m.in_lens16.get(), nreads, n_words, m.in_exc.get(), n_exc, m.in_lens.get(), m.in_offs.get(), &maxlen, &minlen, s));
    DevReads in;
    in.offs = m.in_offs.get(); in.lens = m.in_lens.get(); in.words = m.in_words.get(); in.exc = m.in_exc.get(); in.n_exc = n_exc;
    BK_TRY(align_device(c, in, nreads, m.in_out.get(), s));
    HIP_TRY(hipMemcpy(out, m.in_out.get(), (size_t)nreads * sizeof(bk_hit), hipMemcpyDeviceToHost));
    return BK_OK;
}

int bk_pair_batch(bk_ctx *c, const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint32_t n_pairs, bk_hit *hits,
                  const bk_pe_params *pe)
{
    return bk_pair_batch_seg2(c, bases, offs, lens, n_pairs, hits, nullptr, pe);
}

int bk_pair_batch_seg2(bk_ctx *c, const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint32_t n_pairs, bk_hit *hits,
                       bk_seg2 *seg2, const bk_pe_params *pe)
{
    if (!c || !pe || (n_pairs && (!bases || !offs || !lens || !hits))) return BK_ERR_PARAMS;
    if (c->params.min_chimeric_len > 0 && n_pairs && !seg2) return BK_ERR_PARAMS;
    if (pe->pe_mode < 1 || pe->pe_mode > 4 || pe->pair_min_len < 1 || pe->pair_max_len < pe->pair_min_len) return BK_ERR_PARAMS;
    if (!n_pairs) return BK_OK;
    if (n_pairs > 0x7fffffffu) return BK_ERR_PARAMS;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t nreads = 2 * n_pairs;
    HostExtent x;
    DevReads in;
    BK_TRY(stage_host_batch(c, bases, offs, lens, nreads, x, in));
    hipStream_t s = c->stream;
    bk_hit *d_hits = c->buf.in_out.get();
    HIP_TRY(hipMemcpyAsync(d_hits, hits, (size_t)nreads * sizeof(bk_hit), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    BK_TRY(engine_pair_device(c, in, n_pairs, d_hits, x.maxlen, pe, s, seg2, nullptr));
    HIP_TRY(hipMemcpy(hits, d_hits, (size_t)nreads * sizeof(bk_hit), hipMemcpyDeviceToHost));
    return BK_OK;
}

// device-resident form: reads and their bk_hit records (the output of bk_align_batch_device for exactly these
// reads, interleaved PE1, PE2) already in HBM; hits are updated in place
int bk_pair_batch_device(bk_ctx *c, const void *d_bases, const void *d_offs, const void *d_lens, uint32_t n_pairs, void *d_hits,
                         const bk_pe_params *pe)
{
    return bk_pair_batch_seg2_device(c, d_bases, d_offs, d_lens, n_pairs, d_hits, nullptr, pe);
}

int bk_pair_batch_seg2_device(bk_ctx *c, const void *d_bases, const void *d_offs, const void *d_lens, uint32_t n_pairs, void *d_hits,
                              void *d_seg2, const bk_pe_params *pe)
{
    if (!c || !pe || (n_pairs && (!d_bases || !d_offs || !d_lens || !d_hits))) return BK_ERR_PARAMS;
    if (c->params.min_chimeric_len > 0 && n_pairs && !d_seg2) return BK_ERR_PARAMS;
    if (pe->pe_mode < 1 || pe->pe_mode > 4 || pe->pair_min_len < 1 || pe->pair_max_len < pe->pair_min_len) return BK_ERR_PARAMS;
    if (!n_pairs) return BK_OK;
    if (n_pairs > 0x7fffffffu) return BK_ERR_PARAMS;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t nreads = 2 * n_pairs;
    hipStream_t s = c->stream;
    HIP_TRY(hipMemsetAsync(c->fixed.small.get(), 0, kSmallWords * 4, s));
    launch_max_len((const uint32_t *)d_lens, nreads, c->fixed.small.get() + kSmMaxLen, s);
    HIP_TRY(hipMemcpyAsync(c->h_small.get(), c->fixed.small.get(), kSmallWords * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t maxlen = c->h_small.get()[kSmMaxLen];
    if (maxlen > (uint32_t)kMaxReadLenAbs) return BK_ERR_PARAMS;
    DevReads in;
    in.bases = (const uint8_t *)d_bases; in.offs = (const uint64_t *)d_offs; in.lens = (const uint32_t *)d_lens;
    return engine_pair_device(c, in, n_pairs, (bk_hit *)d_hits, maxlen, pe, s, nullptr, (bk_seg2 *)d_seg2);
}


// Test hook for the search stage (tests/test_gpu_search_stage.py): what LocateFirstExact / LocateLastExact's device form left for every
// (read, strand, core) of the phase named with "debug_stop_phase", as the kernels behind it would have read it
int bk_debug_intervals(bk_ctx *c, uint32_t cap_reads, uint32_t *n_act, uint32_t *iv_cores, uint32_t *act, uint64_t *first, uint32_t *count)
{
    if (!c || !n_act || !iv_cores) return BK_ERR_PARAMS;
    if (!c->dbg_valid) return BK_ERR_PARAMS;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    PhaseCtl ctl{};
    HIP_TRY(hipMemcpy(&ctl, c->fixed.ctl.get() + c->dbg_phase, sizeof(PhaseCtl), hipMemcpyDeviceToHost));
    *n_act = ctl.n_act;
    *iv_cores = c->dbg_ivc;
    if (!act && !first && !count) return BK_OK;
    if (!act || !first || !count || ctl.n_act > cap_reads || ctl.n_act > c->dbg_n) return BK_ERR_PARAMS;
    const uint32_t na = ctl.n_act, stride = c->dbg_n, planes = 2 * c->dbg_ivc;
    HIP_TRY(hipMemcpy(act, c->buf.act[c->dbg_cur].get(), (size_t)na * 4, hipMemcpyDeviceToHost));
    // cores of every listed read in that phase: the search writes no slot beyond them, and like the kernels behind it this reads none
    std::vector<uint32_t> meta(c->dbg_n), nc(na);
    HIP_TRY(hipMemcpy(meta.data(), c->buf.rmeta.get(), (size_t)c->dbg_n * 4, hipMemcpyDeviceToHost));
    for (uint32_t a = 0; a < na; a++) {
        if (act[a] >= c->dbg_n) return BK_ERR_INTERNAL;
        const int len = (int)(meta[act[a]] & kReadLenMask);
        const int n = plan_geo_direct(len, c->dbg_phase, c->cfg).nc;
        nc[a] = n <= kMaxCoresFast ? (uint32_t)n : 0u;
    }
    // (a phase whose slots go by read - bk_iv_slot.h; 4-byte indexes only - is handed out by position all the same)
    const bool by_read = c->dbg_by_read && c->buf.iv2.get() != nullptr;
    std::vector<uint2> h2;
    if (c->buf.iv2.get()) h2.resize(by_read ? stride : na);
    for (uint32_t pl = 0; pl < planes; pl++) {
        uint64_t *f = first + (size_t)pl * na;
        uint32_t *q = count + (size_t)pl * na;
        if (c->buf.iv2.get()) {
            HIP_TRY(hipMemcpy(h2.data(), c->buf.iv2.get() + (size_t)pl * stride, h2.size() * 8, hipMemcpyDeviceToHost));
            for (uint32_t a = 0; a < na; a++) { const uint2 v = h2[iv_index(by_read, a, act[a])]; f[a] = v.x; q[a] = v.y; }
        } else {
            HIP_TRY(hipMemcpy(f, c->buf.iv_first.get() + (size_t)pl * stride, (size_t)na * 8, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(q, c->buf.iv_n.get() + (size_t)pl * stride, (size_t)na * 4, hipMemcpyDeviceToHost));
        }
        for (uint32_t a = 0; a < na; a++)
            if (pl % c->dbg_ivc >= nc[a]) { f[a] = 0; q[a] = 0; }
    }
    return BK_OK;
}


int bk_get_counters(bk_ctx *c, bk_counters *out, int reset)
{
    if (!c || !out) return BK_ERR_PARAMS;
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long hs[kCtrStripes * 8], h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpy(hs, c->fixed.ctr.get(), sizeof(hs), hipMemcpyDeviceToHost));
    for (int i = 0; i < kCtrStripes * 8; i++) h[i & 7] += hs[i];
    memset(out, 0, sizeof(*out));
    out->n_search = h[0]; out->n_cand = h[1]; out->n_lcm_calls = h[2]; out->n_heavy = h[3]; out->n_cand_heavy = h[4]; out->reserved[0] = h[5]; out->reserved[1] = h[6];
    if (reset) HIP_TRY(dev_zero_now(c->fixed.ctr.get(), sizeof(hs)));
    return BK_OK;
}

int bk_get_timing(bk_ctx *c, bk_timing *out, int reset)
{
    if (!c || !out) return BK_ERR_PARAMS;
    *out = c->timing;
    if (reset) c->timing = bk_timing{};
    return BK_OK;
}


int bk_build_sa_device(const void *d_seq, uint64_t concat_len, void *d_sa_out, int sfx_el_size, int device_id)
{
    if (!d_seq || !d_sa_out || !concat_len || (sfx_el_size != 4 && sfx_el_size != 5)) return BK_ERR_PARAMS;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return BK_ERR_NODEVICE;
    if (device_id < 0 || device_id >= ndev) return BK_ERR_PARAMS;
    HIP_TRY(hipSetDevice(device_id));
    return build_sa_device((const uint8_t *)d_seq, concat_len, d_sa_out, sfx_el_size, nullptr);
}


}  // extern "C"
