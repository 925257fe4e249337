// bk_requests.cpp - what the request passes over finished alignments share, once: the sequence lengths by id their validation looks up,
// the threaded gather of read bases (bk_constraints_check, bk_samtags), and the chunk loop of the two plain passes - requests up, one
// kernel, results down - with the passes themselves: the start-site octamer gather (bk_site_*; bk_sites.hip) and the 5' primer artefact
// correction (bk_primer_*; bk_primer.hip).  The loci constraints, the SAM tags and the coverage have loops of their own
// (bk_constraints_host.cpp, bk_samtags.hip, bk_coverage.hip).
#include "bk_engine_int.h"

using namespace bk;

namespace bk {
std::vector<uint32_t> seq_len_by_id(const bk_ctx *c)
{
    std::vector<uint32_t> len_of;
    for (const auto &e : c->entries) { if (e.entry_id >= len_of.size()) len_of.resize((size_t)e.entry_id + 1, 0); len_of[e.entry_id] = e.seq_len; }
    return len_of;
}

void gather_split(uint64_t total_bytes, uint32_t n, const std::function<void(uint32_t, uint32_t)> &part)
{
    const uint32_t nt = total_bytes < (8u << 20) ? 1u : (uint32_t)std::max(1, std::min(8, effective_cpus()));
    std::vector<std::thread> th;
    for (uint32_t k = 1; k < nt; k++) th.emplace_back(part, (uint32_t)((uint64_t)n * k / nt), (uint32_t)((uint64_t)n * (k + 1) / nt));
    part(0, (uint32_t)((uint64_t)n / nt));
    for (auto &x : th) x.join();
}
}  // namespace bk

namespace {
// The chunk loop of a plain pass: at most `chunk_knob` requests at a time travel to d_reqs, launch(m) runs the pass's kernel over them,
// their results come back from d_res, the stream is waited for.  BK_TIMING=1: the kernel's own time, between two events, beside the
// staging copies' - on stderr like the other stage clocks.
template <class Req, class Res, class Launch>
int run_chunks(bk_ctx *c, DevBuf<Req> &d_reqs, DevBuf<Res> &d_res, uint64_t chunk_knob, const Req *reqs, uint64_t n, Res *out, Launch launch, const char *what, const char *unit,
               const char *kernel)
{
    hipStream_t s = c->stream;
    const uint64_t chunk = std::min<uint64_t>(n, chunk_knob);
    HIP_TRY(d_reqs.ensure(chunk));
    HIP_TRY(d_res.ensure(chunk));
    const bool timing = bk::env::timing();
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (timing) { HIP_TRY(hipEventCreate(&ev[0])); HIP_TRY(hipEventCreate(&ev[1])); }
    float ms_kernel = 0.f;
    int rc = BK_OK;
    auto one = [&](uint64_t at, uint64_t m) -> int {
        HIP_TRY(hipMemcpyAsync(d_reqs.get(), reqs + at, m * sizeof(Req), hipMemcpyHostToDevice, s));
        if (timing) HIP_TRY(hipEventRecord(ev[0], s));
        launch(m);
        HIP_TRY(hipGetLastError());
        if (timing) HIP_TRY(hipEventRecord(ev[1], s));
        HIP_TRY(hipMemcpyAsync(out + at, d_res.get(), m * sizeof(Res), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (timing) { float ms = 0.f; HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1])); ms_kernel += ms; }
        return BK_OK;
    };
    for (uint64_t at = 0; at < n && !rc; at += chunk) rc = one(at, std::min(chunk, n - at));
    if (timing) {
        (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
        if (!rc) fprintf(stderr, "bk timing: %s: %llu %s, %s %.3f ms in %llu launches\n", what, (unsigned long long)n, unit, kernel, ms_kernel, (unsigned long long)((n + chunk - 1) / chunk));
    }
    return rc;
}
}  // namespace

extern "C" {

// ---- start-site octamers (see include/biokanga_amd.h) ------------------------------------------
int bk_site_octamers(bk_ctx *c, const bk_site_req *reqs, uint64_t n, int32_t rel_ofs, bk_site_res *out)
{
    if (!c || rel_ofs < -BK_SITE_MAX_OFS || rel_ofs > BK_SITE_MAX_OFS || (n && (!reqs || !out))) return BK_ERR_PARAMS;
    if (!n) return BK_OK;
    const std::vector<uint32_t> len_of = seq_len_by_id(c);                   // (0: no such sequence)
    for (uint64_t i = 0; i < n; i++) {
        const bk_site_req &r = reqs[i];
        if (r.chrom_id >= len_of.size() || !len_of[r.chrom_id] || (r.strand != '+' && r.strand != '-')) return BK_ERR_PARAMS;
    }
    HIP_TRY(hipSetDevice(c->device));
    bk::SiteStage &st = c->site;
    return run_chunks(c, st.reqs, st.res, st.chunk, reqs, n, out, [&](uint64_t m) { launch_site_octamers(c->ix, st.reqs.get(), m, rel_ofs, st.res.get(), c->stream); },
                      "site octamers", "alignments", "k_site_octamers");
}

int bk_site_octamers_device(bk_ctx *c, const void *d_reqs, uint64_t n, int32_t rel_ofs, void *d_out, int sync)
{
    if (!c || rel_ofs < -BK_SITE_MAX_OFS || rel_ofs > BK_SITE_MAX_OFS || (n && (!d_reqs || !d_out)) || ((uintptr_t)d_out & 7)) return BK_ERR_PARAMS;
    if (!n) return BK_OK;
    HIP_TRY(hipSetDevice(c->device));
    launch_site_octamers(c->ix, (const bk_site_req *)d_reqs, n, rel_ofs, (bk_site_res *)d_out, c->stream);
    HIP_TRY(hipGetLastError());
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
    return BK_OK;
}

// ---- 5' primer artefact correction (see include/biokanga_amd.h) ---------------------------------
int bk_primer_correct(bk_ctx *c, const bk_primer_req *reqs, uint64_t n, bk_primer_res *out)
{
    if (!c || (n && (!reqs || !out))) return BK_ERR_PARAMS;
    if (!n) return BK_OK;
    const std::vector<uint32_t> len_of = seq_len_by_id(c);                   // (0: no such sequence)
    for (uint64_t i = 0; i < n; i++) {
        const bk_primer_req &r = reqs[i];
        if (r.chrom_id >= len_of.size() || !len_of[r.chrom_id] || (r.strand != '+' && r.strand != '-') || r.match_len < BK_PRIMER_KLEN ||
            (uint64_t)r.match_loci + r.match_len > len_of[r.chrom_id])
            return BK_ERR_PARAMS;
    }
    HIP_TRY(hipSetDevice(c->device));
    bk::PrimerStage &st = c->primer;
    return run_chunks(c, st.reqs, st.res, st.chunk, reqs, n, out, [&](uint64_t m) { launch_primer_correct(c->ix, st.reqs.get(), m, st.res.get(), c->stream); },
                      "primer correction", "requests", "k_primer_correct");
}

int bk_primer_correct_device(bk_ctx *c, const void *d_reqs, uint64_t n, void *d_out, int sync)
{
    if (!c || (n && (!d_reqs || !d_out)) || ((uintptr_t)d_reqs & 7) || ((uintptr_t)d_out & 15)) return BK_ERR_PARAMS;
    if (!n) return BK_OK;
    HIP_TRY(hipSetDevice(c->device));
    launch_primer_correct(c->ix, (const bk_primer_req *)d_reqs, n, (bk_primer_res *)d_out, c->stream);
    HIP_TRY(hipGetLastError());
    if (sync) HIP_TRY(hipStreamSynchronize(c->stream));
    return BK_OK;
}

}  // extern "C"
