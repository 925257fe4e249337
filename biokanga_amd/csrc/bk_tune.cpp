// bk_tune.cpp - a context's parameters and knobs (include/biokanga_amd.h: bk_ctx_reserve, bk_ctx_set_chrom_filter, bk_ctx_set_params,
// bk_ctx_tune, the index's descriptive getters).  Results never depend on a knob: the test-suite runs independent implementations of the
// same step against each other through them.
#include "bk_engine_int.h"

using namespace bk;

extern "C" {

int bk_ctx_reserve(bk_ctx *c, uint32_t max_batch_reads, uint32_t max_read_len)
{
    if (!c || !max_batch_reads || !max_read_len || max_read_len > (uint32_t)kMaxReadLenAbs) return BK_ERR_PARAMS;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t n = std::min(max_batch_reads, c->chunk_reads);
    const uint32_t wpr = words_per_read(max_read_len);
    const uint32_t ivc = iv_cores_for(c, max_read_len);
    BK_TRY(ensure_batch_scratch(c, n, wpr, rd2_words(c, max_read_len), ivc));
    // pass B's work list: at most one item per (read, strand, core)
    if (c->ix.k2) BK_TRY(ensure_slist(c, (uint64_t)n * ivc * (c->cfg.align_strand == 0 ? 2u : 1u), c->stream));
    if (c->sort_lists) BK_TRY(ensure_sort_scratch(c, n, c->stream));      // (grown when a phase's list is longer)
    if (c->use_wave && c->ix.isa == nullptr) BK_TRY(size_heavy_scratch(c));     // hash-set dedupe of the wave kernel
    // the plan table for reads of up to max_read_len bases under the parameters as they stand, in HBM when the call returns: a batch on
    // any stream may read it, and the call that only enqueues never makes it
    BK_TRY(plan_table_for(c, max_read_len, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BK_OK;
}

int bk_ctx_set_chrom_filter(bk_ctx *c, const uint8_t *accept, uint32_t n)
{
    if (!c || (n && !accept)) return BK_ERR_PARAMS;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->buf.chrom_accept.reset();
    c->n_chrom_accept = 0;
    if (!n) return BK_OK;
    HIP_TRY(c->buf.chrom_accept.ensure(n));
    HIP_TRY(hipMemcpy(c->buf.chrom_accept.get(), accept, n, hipMemcpyHostToDevice));
    c->n_chrom_accept = n;
    return BK_OK;
}

int bk_ctx_set_params(bk_ctx *c, const bk_align_params *p)
{
    if (!c || !p) return BK_ERR_PARAMS;
    bk_align_params old = c->params;
    c->params = *p;
    if (c->params.max_ml == 0) c->params.max_ml = 1;
    int rc = derive_cfg(c);
    if (rc) { c->params = old; derive_cfg(c); return rc; }
    (void)hipSetDevice(c->device);
    return BK_OK;
}

int64_t bk_ctx_tune(bk_ctx *c, const char *name, int64_t value)
{
    if (!c || !name) return BK_ERR_PARAMS;
    (void)hipSetDevice(c->device);
    std::string n(name);
    if (n == "heavy_thresh") {
        int64_t old = c->cfg.heavy_thresh;
        if (value < 0 || value > 100) return BK_ERR_PARAMS;
        c->cfg.heavy_thresh = (int)value;     // 0 routes every call with a non-empty interval to k_heavy
        return old;
    }
    // the chunk knobs: a plain number within bounds, no side effect; the old value comes back
    const struct { const char *name; uint32_t *p32; uint64_t *p64; int64_t lo, hi; } chunk_knobs[] = {
        {"chunk_reads", &c->chunk_reads, nullptr, 1, 1LL << 30},                  // reads per pass over the phases
        {"site_chunk", nullptr, &c->site.chunk, 1, 1LL << 30},                    // requests bk_site_octamers stages at a time
        {"primer_chunk", nullptr, &c->primer.chunk, 1, 1LL << 30},                // .. bk_primer_correct
        {"constraint_chunk", nullptr, &c->constraint_chunk, 1, 1LL << 30},        // .. bk_constraints_check
        {"samtag_chunk", nullptr, &c->samtag.chunk, 1, 1LL << 30},                // .. bk_samtags
        {"coverage_req_chunk", nullptr, &c->cov.req_chunk, 1, 1LL << 30},         // .. bk_coverage_*
        {"coverage_slice_bases", nullptr, &c->cov.slice_bases, 0, INT64_MAX},     // target bases per slice; 0 (the default): the next call derives it from the free memory
        {"coverage_run_chunk", nullptr, &c->cov.run_chunk, 1, 1LL << 26},         // runs per sink call
        {"dup_table_slots", nullptr, &c->dup.table_slots, 0, 1LL << 40},          // slots of bk_mark_duplicates' table; 0 (the default): derived per call.  The call checks a set value against its requests
        {"junction_table_slots", nullptr, &c->jct.table_slots, 0, 1LL << 40},     // .. of bk_junctions' table, the same way
        {"wave_waves", &c->wave_waves, nullptr, 64, 65536},                     // resident waves the wave kernel is launched with
    };
    for (const auto &k : chunk_knobs) {
        if (n != k.name) continue;
        const int64_t old = k.p32 ? (int64_t)*k.p32 : (int64_t)*k.p64;
        if (value < k.lo || value > k.hi) return BK_ERR_PARAMS;
        if (k.p32) *k.p32 = (uint32_t)value;
        else *k.p64 = (uint64_t)value;
        return old;
    }
    // (read only) what a request pass's staging holds now, device and page-locked: 0 until its first call
    if (n == "samtag_buf_bytes") return (int64_t)c->samtag.bytes();
    if (n == "coverage_buf_bytes") return (int64_t)c->cov.bytes();
    if (n == "dup_buf_bytes") return (int64_t)c->dup.bytes();
    if (n == "junction_buf_bytes") return (int64_t)c->jct.bytes();
    if (n == "primer_buf_bytes") return (int64_t)c->primer.bytes();
    if (n == "kmer_bits" || n == "use_ktab") {
        int64_t old = n == "use_ktab" ? c->use_ktab : c->ix.k;
        if (n == "use_ktab") c->use_ktab = value ? 1 : 0;
        else { if (value < 2 || value > 16) return BK_ERR_PARAMS; c->k_req = (int)value; }
        int rc = build_tables(c);
        return rc ? rc : old;
    }
    if (n == "ktab_wide") {                // the k-mer table of an index beyond 2^32 suffixes on any index (tests): 1 packed (ktab_hi + 32-bit offsets), 2 plain 64-bit starts
        int64_t old = c->ktab_wide;
        c->ktab_wide = value < 0 ? 0 : (value > 2 ? 2 : (int)value);
        int rc = build_tables(c);
        return rc ? rc : old;
    }
    if (n == "ktab_packed") return c->ix.ktab_hi != nullptr;       // (read only)
    if (n == "use_k3") {                   // how many key arrays behind the second-level keys (rebuilt with the tables)
        int64_t old = c->use_k3;
        c->use_k3 = value < 0 ? 0 : (value > kMoreKeys ? kMoreKeys : (int)value);
        int rc = build_tables(c);
        return rc ? rc : old;
    }
    if (n == "k3_resident") return (c->ix.kx[0] != nullptr) + (c->ix.kx[1] != nullptr);
    if (n == "ktab2_resident") return c->ix.ktab2 != nullptr;
    if (n == "ktab2_elem") return c->ix.ktab2 != nullptr && c->ix.ktab2_elem;      // (read only) .. and its buckets of one suffix carry suffix array elements
    if (n == "grow_after_reads") { int64_t old = (int64_t)c->grow_after; if (value > 0) c->grow_after = (uint64_t)value; return old; }
    if (n == "grow_state") return c->grow_enabled ? c->grow_state.load() : 5;          // (0 .. 4: bk_ctx_int.h; 5: not a growing context)
    if (n == "image_wait") {               // BK_CTX_GROW_IMAGE: make the long-run tables now if they are not under way, wait for them, take them in
        if (c->grow_enabled) {
            grow_tick(c, 0, true);
            if (c->grow_state.load() != 4 && c->grow_state.load() != 0) grow_take_in(c);
        }
        return (c->ix.kx[0] != nullptr) + (c->ix.kx[1] != nullptr) + (c->ix.ktab2 != nullptr ? 4 : 0);
    }
    if (n == "use_ktab2") {                // k-mer table entries of two words: 0 no, 1 a bucket of one suffix carries its key, 2 its suffix array element (rebuilt with the tables)
        int64_t old = c->use_ktab2;
        c->use_ktab2 = value < 0 ? 0 : (value > 2 ? 2 : (int)value);
        c->grow_elem = c->use_ktab2 == 2;
        int rc = build_tables(c);
        return rc ? rc : old;
    }
    if (n == "sort_lists") {
        int64_t old = c->sort_lists;
        c->sort_lists = (int)value & 7;
        c->sort_lists_set = true;
        return old;
    }
    if (n == "search_split") {             // host only: pass B as one launch (0) or as key levels + a dense launch of the tails (1); the same records either way
        int64_t old = search_split_on(c) ? 1 : 0;
        c->search_split = value ? 1 : 0;
        c->search_split_set = true;
        return old;
    }
    if (n == "prep_search0") {             // host only: phase 0's pass A inside the read preparation (1) or as its own launch (0); the same records either way
        int64_t old = c->prep_search0;
        c->prep_search0 = value ? 1 : 0;
        return old;
    }
    if (n == "use_tgt2") {
        int64_t old = c->use_tgt2;
        c->use_tgt2 = value < 0 ? 0 : (value > 2 ? 2 : (int)value);
        int rc = build_tgt2(c);
        return rc ? rc : old;
    }
    if (n == "wave_len_spec") {            // host only: which form of the wave kernel is launched, never what it computes
        int64_t old = c->wave_len_spec;
        c->wave_len_spec = value ? 1 : 0;
        return old;
    }
    if (n == "async_phases") {             // 0: the phase loop reads its counts back between launches (exact launch sizes), as every other configuration does
        int64_t old = c->async_phases;
        c->async_phases = value ? 1 : 0;
        return old;
    }
    if (n == "swin_resident") return c->image.swin.get() != nullptr ? 1 : 0;      // (read only: whether the window array is in HBM right now)
    if (n == "use_swin") {
        int64_t old = c->use_swin;
        c->use_swin = value < 0 ? 0 : (value > 3 ? 3 : (int)value);
        c->swin_denied = false;
        if (c->image.swin.get() && (!c->use_swin || (c->use_swin == 3) != (c->image.swmap.get() == nullptr))) {
            if (c->stream) (void)hipStreamSynchronize(c->stream);      // (order: the stream that reads the array has ended before it is given back)
            drop_swin(c);
        }
        return old;
    }
    if (n == "swin_skip_short") {           // the partial window array's rule without the reads' this many shortest core lengths; applies to the next build
        int64_t old = c->swin_skip_short;
        c->swin_skip_short = value < 0 ? 0 : (int)std::min<int64_t>(value, kSwLevels - 1);
        return old;
    }
    if (n == "swin_budget_kb") {            // most the partial window array may take (0: what the free memory allows); applies to the next build
        int64_t old = (int64_t)(c->swin_budget >> 10);
        c->swin_budget = value > 0 ? (uint64_t)value << 10 : 0;
        return old;
    }
    // (read only) what the window array occupies, what making it took, how much of the suffix array it holds
    if (n == "swin_mbytes") return (int64_t)(c->swin_bytes >> 20);
    if (n == "swin_setup_us") return (int64_t)(c->swin_setup_s * 1e6);
    if (n == "swin_covered_ppm") return c->image.swin.get() ? (int64_t)(c->swin_covered * 1e6) : 0;
    if (n == "swin_core_lens") return c->image.swmap.get() ? c->swin_w : 0;      // shortest | longest << 8 | levels << 16 of the core lengths its coverage was made for
    if (n == "use_isa") {
        int64_t old = c->use_isa;
        c->use_isa = value ? 1 : 0;
        int rc = build_tables(c);
        return rc ? rc : old;
    }
    if (n == "use_k2") {
        int64_t old = c->use_k2;
        c->use_k2 = value ? 1 : 0;
        int rc = build_tables(c);
        return rc ? rc : old;
    }
    if (n == "use_iv32") {
        int64_t old = c->use_iv32;
        c->use_iv32 = value ? 1 : 0;
        return old;
    }
    if (n == "lazy_search") {
        int64_t old = c->lazy_search;
        c->lazy_search = value ? 1 : 0;
        return old;
    }
    if (n == "iv_poison") {               // test hook: every phase's interval records are filled with ones in front of its search
        int64_t old = c->iv_poison;
        c->iv_poison = value ? 1 : 0;
        return old;
    }
    if (n == "use_wave") {
        int64_t old = c->use_wave;
        c->use_wave = value ? 1 : 0;
        int rc = build_tables(c);
        return rc ? rc : old;
    }
    if (n == "force_rccl") {              // bk_seq_counts_allreduce goes through RCCL even when every context sits on one device
        int64_t old = c->force_rccl ? 1 : 0;
        c->force_rccl = value != 0;
        return old;
    }
    if (n == "rccl_allreduces") return (int64_t)c->rccl_allreduces;      // (read only) reductions of this context that went through RCCL
    if (n == "rccl_ranks") return (int64_t)c->rccl_ranks;                // (read only) .. and the ranks of the last one's communicator
    if (n == "debug_stop_phase") {        // test hook: the next batches stop behind the search of phase value - 1 (bk_debug_intervals); 0: off
        int64_t old = c->dbg_stop_phase + 1;
        c->dbg_stop_phase = value <= 0 ? -1 : (int)value - 1;
        c->dbg_valid = false;
        return old;
    }
    if (n == "max_read_len") {
        int64_t old = c->max_read_len;
        if (value < 16 || value > kMaxReadLenAbs) return BK_ERR_PARAMS;
        c->max_read_len = (int)value;
        return old;
    }
    return BK_ERR_PARAMS;
}


uint32_t bk_num_entries(const bk_ctx *c) { return c ? (uint32_t)c->entries.size() : 0; }
int bk_get_entry(const bk_ctx *c, uint32_t idx, bk_entry_info *out)
{
    if (!c || !out || idx >= c->entries.size()) return BK_ERR_PARAMS;
    *out = c->entries[idx];
    return BK_OK;
}
const char *bk_dataset_name(const bk_ctx *c) { return c ? c->dataset.c_str() : ""; }
uint64_t bk_concat_len(const bk_ctx *c) { return c ? c->ix.n : 0; }
int bk_sfx_el_size(const bk_ctx *c) { return c ? (int)c->el_size : 0; }
int bk_min_core_len(const bk_ctx *c) { return c ? c->cfg.min_core_len : 0; }


}  // extern "C"
