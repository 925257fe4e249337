// bk_samtags.hip - NM:i / MD:Z for callers that format their own SAM or BAM records (bk_samtags of include/biokanga_amd.h): requests of
// 32 bytes and the reads' bases up, one lane per request sets its walk, the wave walks its 64 requests in turn (bk_samtags.h), a prefix
// sum places the MD texts, a second launch writes them.  The same two passes the formatter of bk_sam.hip makes, which carries the tags
// inside its own lines.
#include <hip/hip_runtime.h>
#include "bk_prim.h"

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "bk_ctx_int.h"
#include "bk_env.h"
#include "bk_wait.h"
#include "bk_samtags.h"

namespace {
using namespace bk;

// request j as the walk of its lane: the 32-byte record in two 16-byte loads, fields from the registers.  gofs: where the request's read
// starts in the gathered bases (~0: the read lies outside the caller's bases - no tags)
__device__ __forceinline__ void req_walk(const DevIndex &ix, const uint4 *__restrict__ reqs, const uint64_t *__restrict__ gofs, uint32_t j, TagWalk &w)
{
    const uint4 a = reqs[2 * (size_t)j], b = reqs[2 * (size_t)j + 1];
    const uint32_t chrom_id = a.z, pos = a.w, read_len = b.x & 0xffffu, strand = (b.x >> 16) & 0xffu, gop = b.x >> 24;
    const uint32_t c5 = b.y & 0xffffu, m = b.y >> 16, c3 = b.z & 0xffffu, m2 = b.z >> 16;
    const int gap = (int)b.w;
    const uint64_t at = gofs[j];
    const uint32_t e = chrom_id <= ix.max_id ? ix.id2idx[chrom_id] : 0xffffffffu;
    if (e >= ix.n_ent || at == ~0ULL || (strand != '+' && strand != '-')) return;
    const uint64_t g0 = ix.ent_start[e];
    if (!tag_walk_set(w, read_len, c5, m, c3, gop, (long)gap, m2, strand == '-', pos, ix.ent_end[e] - g0 + 1)) return;
    w.rd_at = at;
    w.g0 = g0 + pos;
}

__global__ void __launch_bounds__(256) k_samtags_measure(DevIndex ix, const uint4 *__restrict__ reqs, uint32_t n, const uint8_t *__restrict__ gbases,
                                                         const uint64_t *__restrict__ gofs, uint16_t *__restrict__ nm, unsigned long long *__restrict__ md_len)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    TagWalk w{};
    if (j < n) req_walk(ix, reqs, gofs, j, w);
    const TagReads rs{gbases, nullptr, nullptr, 0};
    uint32_t my_nm, my_len;
    wave_tags<false>(ix.tgt4, rs, w, nullptr, my_nm, my_len);
    if (j < n) { nm[j] = (uint16_t)my_nm; md_len[j] = my_nm == kTagNone ? 0u : my_len; }
}

// ofs: where every request's text starts in the whole text; this launch's text buffer starts at `base` of it
__global__ void __launch_bounds__(256) k_samtags_write(DevIndex ix, const uint4 *__restrict__ reqs, uint32_t n, const uint8_t *__restrict__ gbases,
                                                       const uint64_t *__restrict__ gofs, const uint16_t *__restrict__ nm, const uint64_t *__restrict__ ofs, uint64_t base,
                                                       char *__restrict__ text)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    TagWalk w{};
    char *dst = nullptr;
    if (j < n && nm[j] != kTagNone) { req_walk(ix, reqs, gofs, j, w); dst = text + (ofs[j] - base); }
    const TagReads rs{gbases, nullptr, nullptr, 0};
    uint32_t my_nm, my_len;
    wave_tags<true>(ix.tgt4, rs, w, dst, my_nm, my_len);
}

}  // namespace

extern "C" int bk_samtags(bk_ctx *c, const bk_samtag_req *reqs, uint64_t n, const uint8_t *bases, uint64_t n_bases, uint16_t *nm_out, uint64_t *md_ofs, char *md_text,
                          uint64_t md_cap, uint64_t *md_needed)
{
    if (!c || (n && (!reqs || !nm_out)) || (n_bases && !bases) || (md_ofs == nullptr) != (md_text == nullptr)) return BK_ERR_PARAMS;
    for (uint64_t i = 0; i < n; i++)
        if (reqs[i].strand != '+' && reqs[i].strand != '-') return BK_ERR_PARAMS;
    const bool want_md = md_ofs != nullptr;
    if (md_needed) *md_needed = 0;
    if (!n) { if (want_md) md_ofs[0] = 0; return BK_OK; }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    bk::SamtagStage &B = c->samtag;
    const uint64_t chunk = std::min<uint64_t>(n, B.chunk);
    HIP_TRY(B.reqs.ensure(chunk));
    HIP_TRY(B.gofs.ensure(chunk));
    HIP_TRY(B.nm.ensure(chunk));
    HIP_TRY(B.len.ensure(chunk + 1));
    HIP_TRY(B.at.ensure(chunk + 1));
    size_t tb = 0;
    HIP_TRY(bk::prim::exclusive_sum(nullptr, tb, B.len.get(), B.at.get(), (size_t)chunk + 1, s));
    HIP_TRY(B.tmp.ensure(tb + 256));
    const bool timing = bk::env::timing();
    const double t_start = bk::now_s();
    // a chunk's requests and the bases of their reads, back to back in request order, on the device
    std::vector<uint64_t> gofs(chunk);
    std::vector<uint8_t> gathered;
    auto stage = [&](uint64_t at, uint32_t m) -> int {
        uint64_t total = 0;
        for (uint32_t t = 0; t < m; t++) {
            const bk_samtag_req &q = reqs[at + t];
            if (q.read_ofs > n_bases || q.read_len > n_bases - q.read_ofs) { gofs[t] = ~0ULL; continue; }
            gofs[t] = total;
            total += q.read_len;
        }
        gathered.resize(total);
        bk::gather_reads(gathered.data(), gofs.data(), bases, total, m, [&](uint32_t t) { return std::make_pair(reqs[at + t].read_ofs, reqs[at + t].read_len); });
        HIP_TRY(B.bases.ensure(std::max<uint64_t>(total, 1) + 16));
        if (bk::upload_host(B.reqs.get(), reqs + at, (size_t)m * sizeof(bk_samtag_req), c->device) ||
            bk::upload_host(B.gofs.get(), gofs.data(), (size_t)m * 8, c->device) || (total && bk::upload_host(B.bases.get(), gathered.data(), total, c->device)))
            return BK_ERR_INTERNAL;
        return BK_OK;
    };
    // pass 1: NM and the length of every MD text.  The answers wait in arrays of the call's own until the text is known to fit.
    std::vector<uint16_t> nm_tmp;
    std::vector<uint64_t> ofs_tmp;
    if (want_md) { nm_tmp.resize(n); ofs_tmp.resize(n + 1); }
    uint64_t total = 0;
    for (uint64_t at = 0; at < n; at += chunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - at);
        if (const int rc = stage(at, m)) return rc;
        HIP_TRY(hipMemsetAsync(B.len.get() + m, 0, 8, s));
        hipLaunchKernelGGL(k_samtags_measure, dim3((m + 255) / 256), dim3(256), 0, s, c->ix, reinterpret_cast<const uint4 *>(B.reqs.get()), m, B.bases.get(),
                           B.gofs.get(), B.nm.get(), B.len.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync((want_md ? nm_tmp.data() : nm_out) + at, B.nm.get(), (size_t)m * 2, hipMemcpyDeviceToHost, s));
        if (want_md) {
            size_t t2 = tb + 256;
            HIP_TRY(bk::prim::exclusive_sum(B.tmp.get(), t2, B.len.get(), B.at.get(), (size_t)m + 1, s));
            HIP_TRY(hipMemcpyAsync(ofs_tmp.data() + at, B.at.get(), ((size_t)m + 1) * 8, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        if (want_md) {
            for (uint64_t t = at; t <= at + m; t++) ofs_tmp[t] += total;
            total = ofs_tmp[at + m];
        }
    }
    if (md_needed) *md_needed = total;
    if (!want_md) return BK_OK;
    if (total > md_cap) return BK_ERR_MEM;
    memcpy(nm_out, nm_tmp.data(), n * 2);
    memcpy(md_ofs, ofs_tmp.data(), (n + 1) * 8);
    // pass 2: the texts (a call of one chunk still has its requests and reads on the device)
    for (uint64_t at = 0; at < n; at += chunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - at);
        const uint64_t bytes = md_ofs[at + m] - md_ofs[at];
        if (!bytes) continue;
        if (n > chunk) { if (const int rc = stage(at, m)) return rc; }
        HIP_TRY(B.text.ensure(bytes));
        HIP_TRY(hipMemcpyAsync(B.nm.get(), nm_out + at, (size_t)m * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(B.at.get(), md_ofs + at, ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_samtags_write, dim3((m + 255) / 256), dim3(256), 0, s, c->ix, reinterpret_cast<const uint4 *>(B.reqs.get()), m, B.bases.get(),
                           B.gofs.get(), B.nm.get(), reinterpret_cast<const uint64_t *>(B.at.get()), md_ofs[at], B.text.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(md_text + md_ofs[at], B.text.get(), bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (timing) fprintf(stderr, "bk timing: SAM tags: %llu requests in %llu chunks, %llu bytes of MD text, %.1f ms\n", (unsigned long long)n, (unsigned long long)((n + chunk - 1) / chunk),
                        (unsigned long long)total, 1e3 * (bk::now_s() - t_start));
    return BK_OK;
}
