// bk_coverage.hip - per-base depth of the accepted records as runs or as a bedGraph (bk_coverage_runs / bk_coverage_text of
// include/biokanga_amd.h, where THE RULE is stated: the depth at a target position is the number of accepted records whose line as written
// has an M base there).  The target is taken in slices of whole sequences, one int32 per base and one more behind every sequence that
// stays 0 - so no M run, no run of equal depth and no carry crosses a sequence or a slice.  Per slice: a lane per request adds +1 at the
// first base of each of its M runs and -1 one past the last (k_cov_mark), an in-place inclusive sum makes the depth, a wave per tile of
// kCovTile positions counts the run starts (depth non-zero and other than the position before) and the run ends (.. than the position
// behind) and the totals (k_cov_count), two exclusive sums give every tile the number of its first start and of its first end - the k-th
// start and the k-th end are the same run's - and k_cov_emit walks the tiles a chunk of runs lies in again and writes the chunk.  The
// text calls format every chunk with a lane per line: measure, exclusive sum, write - the formatter's two passes in small.
#include <hip/hip_runtime.h>
#include "bk_prim.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "bk_ctx_int.h"
#include "bk_env.h"
#include "bk_wait.h"
#include "bk_samtags.h"

namespace {
using namespace bk;

constexpr int kCovBlock = 256;                                       // threads per block of every kernel here
constexpr uint32_t kCovWaves = kCovBlock / 64;
constexpr uint32_t kCovTileSteps = 32;                               // a wave takes its tile 64 positions at a time
constexpr uint32_t kCovTile = 64 * kCovTileSteps;                    // positions per tile: 2048
constexpr uint32_t kCovNameStride = 81;                              // bytes per sequence name on the device, the terminator among them

// Request j of a chunk: validated (flags[j], where the caller wants them: 1 = flagged), and - when its sequence is one of the slice's,
// ent_lo <= entry < ent_hi - its M runs marked in the slice's deltas.  Same-address adds are plain atomics: see DESIGN.md.
__global__ void __launch_bounds__(kCovBlock) k_cov_mark(DevIndex ix, const uint64_t *__restrict__ ent_ofs, const uint4 *__restrict__ reqs, uint32_t n, uint32_t ent_lo,
                                                        uint32_t ent_hi, int32_t *__restrict__ deltas, uint8_t *__restrict__ flags)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint4 q = reqs[j];
    const uint32_t chrom_id = q.x, pos = q.y, m = q.z & 0xffffu, m2 = q.z >> 16;
    const int gap = (int)q.w;
    const uint32_t e = chrom_id <= ix.max_id ? ix.id2idx[chrom_id] : 0xffffffffu;
    bool bad = e >= ix.n_ent || !m || gap < 0;
    if (!bad) {
        const uint64_t len = ix.ent_end[e] - ix.ent_start[e] + 1;
        bad = (uint64_t)pos + m > len || (m2 && (uint64_t)pos + m + (uint32_t)gap + m2 > len);
    }
    if (flags) flags[j] = bad ? 1 : 0;
    if (bad || e < ent_lo || e >= ent_hi) return;
    int32_t *d = deltas + (ent_ofs[e] - ent_ofs[ent_lo] + pos);         // (the last index written is the position behind the sequence)
    atomicAdd(d, 1);
    if (m2 && !gap) { atomicAdd(d + m + m2, -1); return; }              // behind an I: one unbroken run
    atomicAdd(d + m, -1);
    if (m2) { atomicAdd(d + m + (uint32_t)gap, 1); atomicAdd(d + m + (uint32_t)gap + m2, -1); }
}

// One step of a wave over its tile: lane q looks at position p = the step's first + q.  d: the depth there (0 beyond the slice), st / en:
// a run starts / ends there.  carry: the depth in front of the step's first position (wave-uniform; the caller's before the first step).
__device__ __forceinline__ void cov_step(const int32_t *__restrict__ depth, uint64_t len, uint64_t p, int lane, int32_t &carry, int32_t &d, bool &st, bool &en)
{
    d = p < len ? depth[p] : 0;
    int32_t prev = __shfl_up(d, 1), next = __shfl_down(d, 1);
    if (lane == 0) prev = carry;
    if (lane == 63) next = p + 1 < len ? depth[p + 1] : 0;
    carry = __shfl(d, 63);
    st = d != 0 && d != prev;
    en = d != 0 && d != next;
}

__device__ __forceinline__ uint64_t cov_wave_sum(uint64_t v)
{
#pragma unroll
    for (int k = 32; k; k >>= 1) v += tag_shfl64(v, (int)((threadIdx.x & 63) ^ (unsigned)k));
    return v;
}

// tile t of the slice: n_start[t] / n_end[t] = the run starts / run ends among its positions; tot[0] += positions with depth > 0,
// tot[1] += sum of depth, tot[2] = max(depth): reduced over the block, one atomic each per block that has something to add
__global__ void __launch_bounds__(kCovBlock) k_cov_count(const int32_t *__restrict__ depth, uint64_t len, uint32_t *__restrict__ n_start, uint32_t *__restrict__ n_end,
                                                         unsigned long long *__restrict__ tot)
{
    __shared__ unsigned long long s_cov[kCovWaves], s_sum[kCovWaves], s_max[kCovWaves];
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const uint64_t tile = (uint64_t)blockIdx.x * kCovWaves + (uint32_t)wv, p0 = tile * kCovTile;
    uint32_t ns = 0, ne = 0, cov = 0, mx = 0;
    uint64_t sum = 0;
    if (p0 < len) {
        int32_t carry = p0 ? depth[p0 - 1] : 0;
        for (uint32_t step = 0; step < kCovTileSteps && p0 + 64 * step < len; step++) {
            int32_t d;
            bool st, en;
            cov_step(depth, len, p0 + 64 * step + (uint32_t)lane, lane, carry, d, st, en);
            ns += (uint32_t)__popcll(__ballot(st));
            ne += (uint32_t)__popcll(__ballot(en));
            cov += (uint32_t)__popcll(__ballot(d != 0));
            sum += (uint32_t)d;
            mx = max(mx, (uint32_t)d);
        }
        if (lane == 0) { n_start[tile] = ns; n_end[tile] = ne; }
    }
    sum = cov_wave_sum(sum);
#pragma unroll
    for (int k = 32; k; k >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, k));
    if (lane == 0) { s_cov[wv] = cov; s_sum[wv] = sum; s_max[wv] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long c = 0, s = 0, x = 0;
        for (uint32_t w = 0; w < kCovWaves; w++) { c += s_cov[w]; s += s_sum[w]; x = max(x, s_max[w]); }
        if (c) { atomicAdd(&tot[0], c); atomicAdd(&tot[1], s); atomicMax(&tot[2], x); }
    }
}

// the entry of [lo, hi) that slice position x (counted from ent_ofs[0]) lies in
__device__ __forceinline__ uint32_t cov_entry_of(const uint64_t *__restrict__ ent_ofs, uint32_t lo, uint32_t hi, uint64_t x)
{
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ent_ofs[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// The runs [run_lo, run_hi) of the slice into runs[0 ..): the tiles t_lo .. t_hi - from the one run_lo starts in to the one run_hi - 1
// ends in - are walked again, a wave each; the lane at a start writes chrom_id, start and depth of the run of that number, the lane at
// an end writes its end.  at_start / at_end: the exclusive sums of k_cov_count's counts.
__global__ void __launch_bounds__(kCovBlock) k_cov_emit(DevIndex ix, const uint64_t *__restrict__ ent_ofs, uint32_t ent_lo, uint32_t ent_hi, const int32_t *__restrict__ depth,
                                                        uint64_t len, const unsigned long long *__restrict__ at_start, const unsigned long long *__restrict__ at_end, uint64_t t_lo,
                                                        uint64_t t_hi, uint64_t run_lo, uint64_t run_hi, bk_cov_run *__restrict__ runs)
{
    const int lane = (int)(threadIdx.x & 63);
    const uint64_t tile = t_lo + (uint64_t)blockIdx.x * kCovWaves + (threadIdx.x >> 6);
    if (tile > t_hi) return;
    const uint64_t p0 = tile * kCovTile, below = (1ULL << lane) - 1, base = ent_ofs[ent_lo];
    uint64_t rs = at_start[tile], re = at_end[tile];
    if ((at_start[tile + 1] <= run_lo && at_end[tile + 1] <= run_lo) || (rs >= run_hi && re >= run_hi)) return;
    int32_t carry = p0 ? depth[p0 - 1] : 0;
    for (uint32_t step = 0; step < kCovTileSteps && p0 + 64 * step < len && (rs < run_hi || re < run_hi); step++) {
        const uint64_t p = p0 + 64 * step + (uint32_t)lane;
        int32_t d;
        bool st, en;
        cov_step(depth, len, p, lane, carry, d, st, en);
        const uint64_t bs = __ballot(st), be = __ballot(en);
        const uint64_t ks = rs + (uint32_t)__popcll(bs & below), ke = re + (uint32_t)__popcll(be & below);
        if (st && ks >= run_lo && ks < run_hi) {
            const uint32_t e = cov_entry_of(ent_ofs, ent_lo, ent_hi, base + p);
            bk_cov_run &r = runs[ks - run_lo];
            r.chrom_id = ix.ent_id[e];
            r.start = (uint32_t)(base + p - ent_ofs[e]);
            r.depth = (uint32_t)d;
        }
        if (en && ke >= run_lo && ke < run_hi) {
            const uint32_t e = cov_entry_of(ent_ofs, ent_lo, ent_hi, base + p);
            runs[ke - run_lo].end = (uint32_t)(base + p - ent_ofs[e]) + 1;
        }
        rs += (uint32_t)__popcll(bs);
        re += (uint32_t)__popcll(be);
    }
}

__device__ __forceinline__ const char *cov_name(const DevIndex &ix, const char *__restrict__ names, uint32_t chrom_id) { return names + (size_t)ix.id2idx[chrom_id] * kCovNameStride; }

// line j of a chunk: name<TAB>start<TAB>end<TAB>depth<LF>
__global__ void __launch_bounds__(kCovBlock) k_cov_text_measure(DevIndex ix, const char *__restrict__ names, const bk_cov_run *__restrict__ runs, uint32_t n,
                                                                unsigned long long *__restrict__ line_len)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const bk_cov_run r = runs[j];
    const char *nm = cov_name(ix, names, r.chrom_id);
    uint32_t nl = 0;
    while (nm[nl]) nl++;
    line_len[j] = nl + 4u + (uint32_t)(tag_digits(r.start) + tag_digits(r.end) + tag_digits(r.depth));
}

__global__ void __launch_bounds__(kCovBlock) k_cov_text_write(DevIndex ix, const char *__restrict__ names, const bk_cov_run *__restrict__ runs, uint32_t n,
                                                              const unsigned long long *__restrict__ line_at, char *__restrict__ text)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const bk_cov_run r = runs[j];
    const char *nm = cov_name(ix, names, r.chrom_id);
    char *w = text + line_at[j];
    for (; *nm; nm++) *w++ = *nm;
    const uint32_t v[3] = {r.start, r.end, r.depth};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int nd = tag_digits(v[k]);
        *w++ = '\t';
        tag_put_num(w, v[k], nd);
        w += nd;
    }
    *w = '\n';
}

struct CovSinks {
    bk_cov_run_sink runs;
    bk_sam_sink text;
    void *user;
};

int coverage(bk_ctx *c, const bk_cov_req *reqs, uint64_t n, const CovSinks &sink, bk_cov_totals *totals)
{
    if (!c || (n && !reqs) || (!sink.runs && !sink.text) || n >= (1ULL << 31)) return BK_ERR_PARAMS;
    if (totals) *totals = bk_cov_totals{};
    if (!n) return BK_OK;
    const uint32_t n_ent = (uint32_t)c->entries.size();
    if (!n_ent || !c->ix.id2idx) return BK_ERR_PARAMS;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    bk::CovStage &B = c->cov;
    const bool timing = bk::env::timing();
    const double t_start = bk::now_s();
    enum { T_UP, T_MARK, T_SCAN, T_COUNT, T_EMIT, T_TEXT, T_OUT, T_N };
    double t_acc[T_N] = {0}, t_last = t_start;
    auto lap = [&](int what) -> hipError_t {                    // (BK_TIMING only: the stage is waited for and its time booked)
        if (!timing) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(s);
        const double t = bk::now_s();
        t_acc[what] += t - t_last;
        t_last = t;
        return e;
    };

    // every sequence followed by one position of its own
    std::vector<uint64_t> ent_ofs((size_t)n_ent + 1);
    ent_ofs[0] = 0;
    for (uint32_t e = 0; e < n_ent; e++) ent_ofs[e + 1] = ent_ofs[e] + c->entries[e].seq_len + 1;
    if (!B.slice_bases) {
        // a budget, not a measured optimum: three quarters of what is free now for the slice's int32s, the rest for the staging
        // below (some hundred MB at the default chunks), the tile tables (24 bytes per 2048 positions) and whatever comes later
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        B.slice_bases = std::max<uint64_t>((uint64_t)(free_b - free_b / 4) / 4, 1u << 16);
    }
    std::vector<uint32_t> slice_first;                          // the slices: entries [slice_first[k], slice_first[k + 1])
    uint64_t max_len = 0;
    for (uint32_t e = 0; e < n_ent;) {
        uint32_t z = e + 1;
        while (z < n_ent && ent_ofs[z + 1] - ent_ofs[e] <= B.slice_bases) z++;
        slice_first.push_back(e);
        max_len = std::max(max_len, ent_ofs[z] - ent_ofs[e]);
        e = z;
    }
    slice_first.push_back(n_ent);
    const uint64_t max_tiles = (max_len + kCovTile - 1) / kCovTile;
    const uint32_t req_chunk = (uint32_t)std::min<uint64_t>(n, B.req_chunk), run_chunk = (uint32_t)B.run_chunk;

    if (!B.ent_ofs.cap()) {
        HIP_TRY(B.ent_ofs.ensure((size_t)n_ent + 1));
        HIP_TRY(hipMemcpyAsync(B.ent_ofs.get(), ent_ofs.data(), ((size_t)n_ent + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (sink.text && !B.names.cap()) {
        std::vector<char> names((size_t)n_ent * kCovNameStride, 0);
        for (uint32_t e = 0; e < n_ent; e++) { memcpy(&names[(size_t)e * kCovNameStride], c->entries[e].name, kCovNameStride); names[(size_t)e * kCovNameStride + kCovNameStride - 1] = 0; }
        HIP_TRY(B.names.ensure(names.size()));
        HIP_TRY(hipMemcpyAsync(B.names.get(), names.data(), names.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    HIP_TRY(B.reqs.ensure(req_chunk));
    HIP_TRY(B.flags.ensure(req_chunk));
    HIP_TRY(B.depth.ensure(max_len));
    for (int k = 0; k < 2; k++) { HIP_TRY(B.tile_n[k].ensure(max_tiles + 1)); HIP_TRY(B.tile_at[k].ensure(max_tiles + 1)); }
    HIP_TRY(B.tot.ensure(3));
    HIP_TRY(B.runs.ensure(run_chunk));
    if (sink.text) { HIP_TRY(B.len.ensure((size_t)run_chunk + 1)); HIP_TRY(B.at.ensure((size_t)run_chunk + 1)); }
    size_t tb = 0, tb1 = 0;
    HIP_TRY(bk::prim::inclusive_sum(nullptr, tb1, B.depth.get(), B.depth.get(), (size_t)max_len, s));
    tb = std::max(tb, tb1);
    HIP_TRY(bk::prim::exclusive_sum(nullptr, tb1, B.tile_n[0].get(), B.tile_at[0].get(), (size_t)max_tiles + 1, s));
    tb = std::max(tb, tb1);
    if (sink.text) {
        HIP_TRY(bk::prim::exclusive_sum(nullptr, tb1, B.len.get(), B.at.get(), (size_t)run_chunk + 1, s));
        tb = std::max(tb, tb1);
    }
    HIP_TRY(B.tmp.ensure(tb + 256));
    const uint64_t host_need = std::max<uint64_t>((uint64_t)run_chunk * sizeof(bk_cov_run), 256);
    HIP_TRY(B.host.ensure(host_need));
    const uint64_t host_piece = host_need;                      // (a larger buffer left by an earlier call changes nothing about the pieces)
    HIP_TRY(hipMemsetAsync(B.tot.get(), 0, 3 * 8, s));

    std::vector<uint8_t> flags(req_chunk);
    std::vector<unsigned long long> at_start, at_end;
    uint64_t n_runs = 0, n_flagged = 0, text_at = 0;
    if (timing) { HIP_TRY(hipStreamSynchronize(s)); t_last = bk::now_s(); }
    for (size_t k = 0; k + 1 < slice_first.size(); k++) {
        const uint32_t e0 = slice_first[k], e1 = slice_first[k + 1];
        const uint64_t len = ent_ofs[e1] - ent_ofs[e0], n_tiles = (len + kCovTile - 1) / kCovTile;
        int32_t *depth = B.depth.get();
        HIP_TRY(hipMemsetAsync(depth, 0, (size_t)len * 4, s));
        for (uint64_t at = 0; at < n; at += req_chunk) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(req_chunk, n - at);
            HIP_TRY(hipStreamSynchronize(s));                   // (the chunk before has been read)
            if (n > req_chunk || k == 0) {                      // (a call of one chunk still has its requests on the device)
                if (bk::upload_host(B.reqs.get(), reqs + at, (size_t)m * sizeof(bk_cov_req), c->device)) return BK_ERR_INTERNAL;
            }
            HIP_TRY(lap(T_UP));
            hipLaunchKernelGGL(k_cov_mark, dim3((m + kCovBlock - 1) / kCovBlock), dim3(kCovBlock), 0, s, c->ix, B.ent_ofs.get(), reinterpret_cast<const uint4 *>(B.reqs.get()), m, e0,
                               e1, depth, k == 0 ? B.flags.get() : nullptr);
            HIP_TRY(hipGetLastError());
            HIP_TRY(lap(T_MARK));
            if (k == 0) {
                HIP_TRY(hipMemcpyAsync(flags.data(), B.flags.get(), m, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                for (uint32_t t = 0; t < m; t++) n_flagged += flags[t];
            }
        }
        size_t t2 = B.tmp.cap();
        HIP_TRY(bk::prim::inclusive_sum(B.tmp.get(), t2, depth, depth, (size_t)len, s));
        HIP_TRY(lap(T_SCAN));
        for (int q = 0; q < 2; q++) HIP_TRY(hipMemsetAsync(B.tile_n[q].get() + n_tiles, 0, 4, s));
        hipLaunchKernelGGL(k_cov_count, dim3((uint32_t)((n_tiles + kCovWaves - 1) / kCovWaves)), dim3(kCovBlock), 0, s, depth, len, B.tile_n[0].get(), B.tile_n[1].get(),
                           B.tot.get());
        HIP_TRY(hipGetLastError());
        at_start.resize(n_tiles + 1);
        at_end.resize(n_tiles + 1);
        for (int q = 0; q < 2; q++) {
            t2 = B.tmp.cap();
            HIP_TRY(bk::prim::exclusive_sum(B.tmp.get(), t2, B.tile_n[q].get(), B.tile_at[q].get(), (size_t)n_tiles + 1, s));
            HIP_TRY(hipMemcpyAsync((q ? at_end : at_start).data(), B.tile_at[q].get(), ((size_t)n_tiles + 1) * 8, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(lap(T_COUNT));
        const uint64_t slice_runs = at_start[n_tiles];
        if (at_end[n_tiles] != slice_runs) { fprintf(stderr, "biokanga_amd: coverage: %llu run starts but %llu run ends in a slice\n", (unsigned long long)slice_runs, (unsigned long long)at_end[n_tiles]); return BK_ERR_INTERNAL; }
        for (uint64_t lo = 0; lo < slice_runs; lo += run_chunk) {
            const uint64_t hi = std::min<uint64_t>(slice_runs, lo + run_chunk);
            const uint32_t cnt = (uint32_t)(hi - lo);
            // run lo starts in the last tile whose first start is numbered <= lo, run hi - 1 ends in the last tile whose first end is <= hi - 1
            const uint64_t t_lo = (uint64_t)(std::upper_bound(at_start.begin(), at_start.end(), lo) - at_start.begin()) - 1;
            const uint64_t t_hi = (uint64_t)(std::upper_bound(at_end.begin(), at_end.end(), hi - 1) - at_end.begin()) - 1;
            if (t_hi < t_lo || t_hi >= n_tiles) return BK_ERR_INTERNAL;
            hipLaunchKernelGGL(k_cov_emit, dim3((uint32_t)((t_hi - t_lo + kCovWaves) / kCovWaves)), dim3(kCovBlock), 0, s, c->ix, B.ent_ofs.get(), e0, e1, depth, len, B.tile_at[0].get(),
                               B.tile_at[1].get(), t_lo, t_hi, lo, hi, B.runs.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(lap(T_EMIT));
            if (sink.runs) {
                HIP_TRY(hipMemcpyAsync(B.host.get(), B.runs.get(), (size_t)cnt * sizeof(bk_cov_run), hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                if (const int rc = sink.runs(sink.user, reinterpret_cast<const bk_cov_run *>(B.host.get()), cnt, n_runs)) return rc < 0 ? BK_ERR_INTERNAL : BK_ERR_FILEACCESS;
            } else {
                unsigned long long bytes = 0;
                HIP_TRY(hipMemsetAsync(B.len.get() + cnt, 0, 8, s));
                hipLaunchKernelGGL(k_cov_text_measure, dim3((cnt + kCovBlock - 1) / kCovBlock), dim3(kCovBlock), 0, s, c->ix, B.names.get(), B.runs.get(), cnt, B.len.get());
                HIP_TRY(hipGetLastError());
                t2 = B.tmp.cap();
                HIP_TRY(bk::prim::exclusive_sum(B.tmp.get(), t2, B.len.get(), B.at.get(), (size_t)cnt + 1, s));
                HIP_TRY(hipMemcpyAsync(&bytes, B.at.get() + cnt, 8, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                HIP_TRY(B.text.ensure(bytes));
                hipLaunchKernelGGL(k_cov_text_write, dim3((cnt + kCovBlock - 1) / kCovBlock), dim3(kCovBlock), 0, s, c->ix, B.names.get(), B.runs.get(), cnt, B.at.get(),
                                   B.text.get());
                HIP_TRY(hipGetLastError());
                HIP_TRY(lap(T_TEXT));
                for (uint64_t o = 0; o < bytes; o += host_piece) {           // (a line may lie across two pieces)
                    const uint64_t piece = std::min<uint64_t>(host_piece, bytes - o);
                    HIP_TRY(hipMemcpyAsync(B.host.get(), B.text.get() + o, piece, hipMemcpyDeviceToHost, s));
                    HIP_TRY(hipStreamSynchronize(s));
                    if (const int rc = sink.text(sink.user, reinterpret_cast<const char *>(B.host.get()), piece, text_at)) return rc < 0 ? BK_ERR_INTERNAL : BK_ERR_FILEACCESS;
                    text_at += piece;
                }
            }
            n_runs += cnt;
            if (timing) { t_acc[T_OUT] += bk::now_s() - t_last; t_last = bk::now_s(); }
        }
    }
    unsigned long long tot[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(tot, B.tot.get(), sizeof(tot), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (totals) { totals->runs = n_runs; totals->covered = tot[0]; totals->depth_sum = tot[1]; totals->max_depth = tot[2]; totals->flagged = n_flagged; }
    if (timing)
        fprintf(stderr, "bk timing: coverage: %llu requests, %zu slices of up to %llu positions, %llu runs, %llu bytes of text: clear + upload %.2f, k_cov_mark %.2f, scan %.2f, k_cov_count + tile sums %.2f, "
                        "k_cov_emit %.2f, text kernels %.2f, copies + sink %.2f, whole call %.1f ms\n",
                (unsigned long long)n, slice_first.size() - 1, (unsigned long long)max_len, (unsigned long long)n_runs, (unsigned long long)text_at, 1e3 * t_acc[T_UP], 1e3 * t_acc[T_MARK],
                1e3 * t_acc[T_SCAN], 1e3 * t_acc[T_COUNT], 1e3 * t_acc[T_EMIT], 1e3 * t_acc[T_TEXT], 1e3 * t_acc[T_OUT], 1e3 * (bk::now_s() - t_start));
    return BK_OK;
}

}  // namespace

extern "C" int bk_coverage_runs(bk_ctx *c, const bk_cov_req *reqs, uint64_t n, bk_cov_run_sink sink, void *user, bk_cov_totals *totals)
{
    return coverage(c, reqs, n, CovSinks{sink, nullptr, user}, totals);
}

extern "C" int bk_coverage_text(bk_ctx *c, const bk_cov_req *reqs, uint64_t n, bk_sam_sink sink, void *user, bk_cov_totals *totals)
{
    return coverage(c, reqs, n, CovSinks{nullptr, sink, user}, totals);
}
