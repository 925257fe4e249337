// bk_snp_host.cpp - SNP pile-up and screening entry points (include/biokanga_amd.h: bk_snp_*; CAligner::ProcessSNPs, Aligner.cpp:7609-8071);
// the kernels are in bk_snp.hip.
#include "bk_engine_int.h"

using namespace bk;

extern "C" {

// ---- SNP pile-up and screening (see include/biokanga_amd.h) -------------------------------------
int bk_snp_reset(bk_ctx *c)
{
    if (!c) return BK_ERR_PARAMS;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->ix.n * 6 * sizeof(uint32_t);
    if (!c->fixed.snp_planes.get()) HIP_TRY(c->fixed.snp_planes.ensure((size_t)c->ix.n * 6));
    if (!c->fixed.snp_tot.get()) HIP_TRY(c->fixed.snp_tot.ensure(4));
    HIP_TRY(clear_dev(c->fixed.snp_planes.get(), bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BK_OK;
}

int bk_snp_pileup(bk_ctx *c, const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint32_t nreads, const bk_snp_aln *alns,
                  uint64_t n_alns)
{
    if (!c || (n_alns && (!bases || !offs || !lens || !alns || !nreads))) return BK_ERR_PARAMS;
    if (!c->fixed.snp_planes.get()) return BK_ERR_PARAMS;                      // bk_snp_reset() first
    if (!n_alns) return BK_OK;
    uint32_t max_id = 0;
    for (const auto &e : c->entries) max_id = std::max(max_id, e.entry_id);
    for (uint64_t i = 0; i < n_alns; i++) {
        const bk_snp_aln &a = alns[i];
        if (a.read_idx >= nreads || (uint32_t)a.read_ofs + a.len > lens[a.read_idx] || (a.strand != '+' && a.strand != '-')) return BK_ERR_PARAMS;
        if (a.chrom_id == 0 || a.chrom_id > max_id) return BK_ERR_PARAMS;
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const HostExtent x = host_extent(offs, lens, nreads);
    DevBuf<uint8_t> d_bases;
    DevBuf<uint64_t> d_offs;
    DevBuf<bk_snp_aln> d_alns;
    HIP_TRY(d_bases.ensure(x.hi - x.lo + 16));
    HIP_TRY(d_offs.ensure(nreads));
    HIP_TRY(d_alns.ensure(n_alns));
    // (an early return frees the buffers - which waits for the device - before x.rel, the source of a copy, goes)
    HIP_TRY(hipMemcpyAsync(d_bases.get(), bases + x.lo, x.hi - x.lo, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_offs.get(), x.rel.data(), (size_t)nreads * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_alns.get(), alns, (size_t)n_alns * sizeof(bk_snp_aln), hipMemcpyHostToDevice, s));
    launch_snp_pileup(c->ix, d_bases.get(), d_offs.get(), c->image.id2idx.get(), d_alns.get(), n_alns, c->fixed.snp_planes.get(), s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return BK_OK;
}

int bk_snp_pileup_device(bk_ctx *c, const void *d_bases, const void *d_offs, uint32_t nreads, const void *d_alns, uint64_t n_alns, int sync)
{
    if (!c || (n_alns && (!d_bases || !d_offs || !d_alns || !nreads))) return BK_ERR_PARAMS;
    if (!c->fixed.snp_planes.get()) return BK_ERR_PARAMS;
    if (!n_alns) return BK_OK;
    HIP_TRY(hipSetDevice(c->device));
    launch_snp_pileup(c->ix, (const uint8_t *)d_bases, (const uint64_t *)d_offs, c->image.id2idx.get(), (const bk_snp_aln *)d_alns, n_alns, c->fixed.snp_planes.get(), c->stream);
    HIP_TRY(hipGetLastError());
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
    return BK_OK;
}

int bk_snp_counts(bk_ctx *c, uint32_t chrom_id, uint32_t loci, uint32_t n, uint32_t *out)
{
    if (!c || !out || !c->fixed.snp_planes.get()) return BK_ERR_PARAMS;
    const bk_entry_info *ent = nullptr;
    for (const auto &e : c->entries) if (e.entry_id == chrom_id) { ent = &e; break; }
    if (!ent || (uint64_t)loci + n > ent->seq_len) return BK_ERR_PARAMS;
    if (!n) return BK_OK;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<uint32_t> d_out;
    HIP_TRY(d_out.ensure((size_t)n * 7));
    launch_snp_gather(c->ix, c->fixed.snp_planes.get(), ent->start_ofs + loci, n, d_out.get(), c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out.get(), (size_t)n * 7 * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BK_OK;
}

int bk_snp_centroid_insts(bk_ctx *c, uint32_t chrom_id, int32_t min_reads, uint32_t *num_insts)
{
    if (!c || !num_insts || min_reads < 1 || !c->fixed.snp_planes.get()) return BK_ERR_PARAMS;
    const bk_entry_info *ent = nullptr;
    for (const auto &e : c->entries) if (e.entry_id == chrom_id) { ent = &e; break; }
    if (!ent) return BK_ERR_PARAMS;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<uint32_t> d_hist;
    HIP_TRY(d_hist.ensure(BK_SNP_CENTROIDS));
    std::vector<uint32_t> h(BK_SNP_CENTROIDS);
    HIP_TRY(hipMemsetAsync(d_hist.get(), 0, BK_SNP_CENTROIDS * 4, c->stream));
    launch_snp_centroids(c->ix, c->fixed.snp_planes.get(), ent->start_ofs, (uint32_t)ent->seq_len, (uint32_t)min_reads, d_hist.get(), c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h.data(), d_hist.get(), BK_SNP_CENTROIDS * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < BK_SNP_CENTROIDS; i++) num_insts[i] += h[i];
    return BK_OK;
}

int bk_snp_sites(bk_ctx *c, uint32_t chrom_id, int32_t min_reads, double min_nonref_prop, const bk_snp_site **sites, uint64_t *n_sites,
                 bk_snp_chrom *totals)
{
    if (!c || !sites || !n_sites || !totals || min_reads < 1 || !(min_nonref_prop >= 0.0)) return BK_ERR_PARAMS;
    if (!c->fixed.snp_planes.get()) return BK_ERR_PARAMS;
    const bk_entry_info *ent = nullptr;
    for (const auto &e : c->entries) if (e.entry_id == chrom_id) { ent = &e; break; }
    if (!ent) return BK_ERR_PARAMS;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevBuf<bk_snp_site> &d_sites = c->snp.d_sites;
    if (!d_sites.cap()) HIP_TRY(d_sites.ensure(1u << 20));
    unsigned long long h_tot[4] = {0, 0, 0, 0};
    uint32_t n = 0;
    for (;;) {                                                        // second pass only when the list outgrew its buffer
        HIP_TRY(hipMemsetAsync(c->fixed.small.get(), 0, kSmallWords * 4, s));
        HIP_TRY(hipMemsetAsync(c->fixed.snp_tot.get(), 0, 4 * 8, s));
        launch_snp_sites(c->ix, c->fixed.snp_planes.get(), ent->start_ofs, (uint32_t)ent->seq_len, (uint32_t)min_reads, min_nonref_prop, d_sites.get(),
                         (uint32_t)d_sites.cap(), c->fixed.small.get() + kSmCount, c->fixed.snp_tot.get(), s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&n, c->fixed.small.get() + kSmCount, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h_tot, c->fixed.snp_tot.get(), sizeof(h_tot), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (n <= d_sites.cap()) break;
        HIP_TRY(d_sites.ensure(n));
    }
    c->snp.sites.resize(n);
    if (n) HIP_TRY(hipMemcpy(c->snp.sites.data(), d_sites.get(), (size_t)n * sizeof(bk_snp_site), hipMemcpyDeviceToHost));
    std::sort(c->snp.sites.begin(), c->snp.sites.end(), [](const bk_snp_site &a, const bk_snp_site &b) { return a.loci < b.loci; });
    *sites = n ? c->snp.sites.data() : nullptr;
    *n_sites = n;
    totals->tot_match = h_tot[0]; totals->tot_mismatch = h_tot[1]; totals->loci_covered = h_tot[2]; totals->bases_coverage = h_tot[3];
    return BK_OK;
}

}  // extern "C"
