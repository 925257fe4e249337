// bk_constraints_host.cpp - the loci base constraints of `align -5` behind the C ABI (include/biokanga_amd.h: bk_constraints_*): the set
// of a run validated, sorted and uploaded; the check of finished alignments against it in chunks - requests up, k_constraint_touch, the
// list of touched requests down, their reads' bases gathered and up, k_constraint_check, statuses down.  The kernels are in
// bk_constraints.hip.
#include "bk_engine_int.h"

using namespace bk;

struct bk_constraints {
    bk_ctx *c = nullptr;
    DevBuf<DevConstraint> tab;
    DevBuf<DevConstraintSlice> dir;
    DevConstraints dev{};
    // the staging of bk_constraints_check, made by its first call with requests
    DevBuf<bk_constraint_req> d_reqs;
    DevBuf<uint8_t> d_status, d_bases;
    DevBuf<ConstraintHit> d_list;
    DevBuf<uint32_t> d_cnt;
    DevBuf<uint64_t> d_gofs;
    PinBuf<ConstraintHit> h_list;
    PinBuf<uint32_t> h_cnt;
    PinBuf<uint8_t> h_bases;
    PinBuf<uint64_t> h_gofs;
};

namespace bk {
void launch_constraint_touch(const DevIndex &ix, const DevConstraints &cs, const bk_constraint_req *reqs, uint32_t n, uint64_t n_bases, uint8_t *status,
                             ConstraintHit *list, uint32_t *list_cnt, hipStream_t s);
void launch_constraint_check(const DevIndex &ix, const DevConstraints &cs, const bk_constraint_req *reqs, const ConstraintHit *list, uint32_t n_list,
                             const uint8_t *gbases, const uint64_t *gofs, uint8_t *status, hipStream_t s);
}

extern "C" {

int bk_constraints_create(bk_ctx *c, const bk_constraint *cons, uint32_t n, bk_constraints **out)
{
    if (!c || !out || (n && !cons) || n > BK_MAX_CONSTRAINTS) return BK_ERR_PARAMS;
    *out = nullptr;
    const std::vector<uint32_t> len_of = seq_len_by_id(c);                   // (0: no such sequence)
    std::vector<bk_constraint> v(cons, cons + n);
    for (const bk_constraint &k : v)
        if (k.chrom_id >= len_of.size() || !len_of[k.chrom_id] || k.start > k.end || k.end >= len_of[k.chrom_id] || !k.mask || (k.mask & ~0x1fu)) return BK_ERR_PARAMS;
    std::sort(v.begin(), v.end(), [](const bk_constraint &a, const bk_constraint &b) {
        return a.chrom_id != b.chrom_id ? a.chrom_id < b.chrom_id : (a.start != b.start ? a.start < b.start : (a.end != b.end ? a.end < b.end : a.mask < b.mask));
    });
    std::vector<DevConstraint> tab(n);
    std::vector<DevConstraintSlice> dir;
    for (uint32_t i = 0; i < n; i++) {
        if (dir.empty() || dir.back().chrom_id != v[i].chrom_id) dir.push_back(DevConstraintSlice{v[i].chrom_id, i, 0, 0});
        DevConstraintSlice &sl = dir.back();
        const uint32_t before = sl.count ? tab[i - 1].max_end : 0u;
        tab[i] = DevConstraint{v[i].start, v[i].end, std::max(before, v[i].end), v[i].mask};
        sl.count++;
    }
    if (dir.size() > BK_MAX_CONSTRAINED_SEQS) return BK_ERR_PARAMS;
    bk_constraints *s = new (std::nothrow) bk_constraints;
    if (!s) return BK_ERR_MEM;
    s->c = c;
    auto fail = [&](int rc) { delete s; return rc; };
    if (hipSetDevice(c->device) != hipSuccess) return fail(BK_ERR_INTERNAL);
    // (an empty set keeps one element of each: the kernels are handed pointers they never follow)
    if (s->tab.ensure(std::max<size_t>(n, 1)) != hipSuccess || s->dir.ensure(std::max<size_t>(dir.size(), 1)) != hipSuccess) return fail(BK_ERR_MEM);
    if (n && (hipMemcpy(s->tab.get(), tab.data(), n * sizeof(DevConstraint), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(s->dir.get(), dir.data(), dir.size() * sizeof(DevConstraintSlice), hipMemcpyHostToDevice) != hipSuccess))
        return fail(BK_ERR_INTERNAL);
    s->dev = DevConstraints{s->tab.get(), s->dir.get(), n, (uint32_t)dir.size()};
    *out = s;
    return BK_OK;
}

void bk_constraints_destroy(bk_constraints *s)
{
    if (!s) return;
    (void)hipSetDevice(s->c->device);
    delete s;
}

int bk_constraints_check(bk_constraints *set, const bk_constraint_req *reqs, uint64_t n, const uint8_t *bases, uint64_t n_bases, uint8_t *status_out, uint64_t counts[4])
{
    if (!set || (n && (!reqs || !status_out)) || (n_bases && !bases)) return BK_ERR_PARAMS;
    if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (!n) return BK_OK;
    bk_ctx *c = set->c;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint64_t chunk = std::min<uint64_t>(n, c->constraint_chunk);
    HIP_TRY(set->d_reqs.ensure(chunk));
    HIP_TRY(set->d_status.ensure(chunk));
    HIP_TRY(set->d_list.ensure(chunk));
    HIP_TRY(set->d_cnt.ensure(1));
    HIP_TRY(set->h_list.ensure(chunk));
    HIP_TRY(set->h_cnt.ensure(1));
    // (BK_TIMING=1: where the pass spends its time, on stderr like the other stage clocks; the kernels are waited for either way)
    const bool timing = bk::env::timing();
    double ms[7] = {0, 0, 0, 0, 0, 0, 0};               // requests up, touch, list down, gather, bases up, check, statuses down
    auto now = []() { return 1e3 * bk::now_s(); };
    uint64_t n_touched = 0, n_gathered = 0;
    auto one = [&](uint64_t at, uint32_t m) -> int {
        double t0 = now(), t1;
        auto lap = [&](int k) { t1 = now(); ms[k] += t1 - t0; t0 = t1; };
        HIP_TRY(hipMemcpyAsync(set->d_reqs.get(), reqs + at, (size_t)m * sizeof(bk_constraint_req), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(set->d_cnt.get(), 0, sizeof(uint32_t), s));
        if (timing) { HIP_TRY(hipStreamSynchronize(s)); lap(0); }
        launch_constraint_touch(c->ix, set->dev, set->d_reqs.get(), m, n_bases, set->d_status.get(), set->d_list.get(), set->d_cnt.get(), s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(set->h_cnt.get(), set->d_cnt.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        lap(1);
        const uint32_t n_list = *set->h_cnt.get();
        if (n_list > m) return BK_ERR_INTERNAL;
        if (n_list) {
            HIP_TRY(hipMemcpyAsync(set->h_list.get(), set->d_list.get(), (size_t)n_list * sizeof(ConstraintHit), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            lap(2);
            // the listed reads' bases, back to back in list order (the kernel served these requests: their reads lie inside `bases`)
            HIP_TRY(set->h_gofs.ensure(n_list));
            HIP_TRY(set->d_gofs.ensure(n_list));
            uint64_t total = 0;
            for (uint32_t t = 0; t < n_list; t++) { set->h_gofs.get()[t] = total; total += reqs[at + set->h_list.get()[t].req].read_len; }
            HIP_TRY(set->h_bases.ensure(std::max<uint64_t>(total, 1)));
            HIP_TRY(set->d_bases.ensure(std::max<uint64_t>(total, 1)));
            gather_reads(set->h_bases.get(), set->h_gofs.get(), bases, total, n_list, [&](uint32_t t) {
                const bk_constraint_req &q = reqs[at + set->h_list.get()[t].req];
                return std::make_pair((uint64_t)q.read_ofs, (uint32_t)q.read_len);
            });
            lap(3);
            HIP_TRY(hipMemcpyAsync(set->d_gofs.get(), set->h_gofs.get(), (size_t)n_list * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            if (total) HIP_TRY(hipMemcpyAsync(set->d_bases.get(), set->h_bases.get(), total, hipMemcpyHostToDevice, s));
            if (timing) { HIP_TRY(hipStreamSynchronize(s)); lap(4); }
            launch_constraint_check(c->ix, set->dev, set->d_reqs.get(), set->d_list.get(), n_list, set->d_bases.get(), set->d_gofs.get(), set->d_status.get(), s);
            HIP_TRY(hipGetLastError());
            if (timing) { HIP_TRY(hipStreamSynchronize(s)); lap(5); }
            n_touched += n_list;
            n_gathered += total;
        }
        HIP_TRY(hipMemcpyAsync(status_out + at, set->d_status.get(), m, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        lap(6);
        return BK_OK;
    };
    int rc = BK_OK;
    for (uint64_t at = 0; at < n && !rc; at += chunk) rc = one(at, (uint32_t)std::min(chunk, n - at));
    if (rc) return rc;
    if (counts)
        for (uint64_t i = 0; i < n; i++) counts[status_out[i] == BK_CONSTRAINT_UNTOUCHED ? 0 : (status_out[i] == BK_CONSTRAINT_TOUCHED ? 1 : (status_out[i] == BK_CONSTRAINT_VIOLATED ? 2 : 3))]++;
    if (timing)
        fprintf(stderr, "bk timing: loci constraints: %llu requests in %llu chunks, %llu touched (%llu bases gathered): requests up %.3f ms, k_constraint_touch %.3f, list down %.3f, "
                        "gather %.3f, bases up %.3f, k_constraint_check %.3f, statuses down %.3f\n",
                (unsigned long long)n, (unsigned long long)((n + chunk - 1) / chunk), (unsigned long long)n_touched, (unsigned long long)n_gathered, ms[0], ms[1], ms[2], ms[3], ms[4],
                ms[5], ms[6]);
    return BK_OK;
}

}  // extern "C"
