// What the host decides about a chunk (bk_phase_plan.h) on the host: tests/test_host_phase_plan.py compiles this beside a stand-in for
// <hip/hip_runtime.h>; bk_phase_plan.h, bk_plan_table.h and bk_device.h are the files as they stand.
//   - chunk_bounds against direct calls of plan_geo_direct, for maxlen 1 .. 2000 at the family and tile edges, over the parameter sweep of
//     plan_table_host.cpp: max_phases the largest n_phases, cmax_bound[ph] the largest nc of the lengths that have the phase (capped at
//     kMaxCoresFast), cores_fit false exactly when an nc passes the cap, rows beyond max_phases zero
//   - window_words_for against the ladder in words; rd2w_for half of it wherever it is not zero
//   - sort_prefix against the two rules the phase loop used to spell out (pass B's list, the wave list), restated here, over a grid
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bk_phase_plan.h"

using namespace bk;

static int fail(const char *what) { printf("FAIL: %s\n", what); return 1; }

static const uint32_t kMaxlens[] = {1, 15, 16, 17, 100, 128, 129, 256, 257, 320, 321, 512, 513, 2000};

static int test_bounds()
{
    const int max_subs_v[] = {0, 1, 3, 5, 10, 25, 40, 63}, mm_delta_v[] = {1, 2};
    const int slides_v[] = {6, 8, 9, 1, 50}, min_core_v[] = {4, 14, 19, 1, 1999};
    const int top = kMaxReadLenAbs;
    std::vector<uint2> tab;
    std::vector<int> nph(top + 1), nc((size_t)(top + 1) * (kMaxPhases + 1));
    long checked = 0;
    bool some_unfit = false, some_fit = false;
    for (int ms : max_subs_v)
        for (int md : mm_delta_v)
            for (int sl : slides_v)
                for (int mc : min_core_v) {
                    if ((sl == 1 || sl == 50) && mc != 1 && mc != 14 && mc != 1999) continue;          // (the sweep of plan_table_host.cpp)
                    if (ms >= 25 && !((sl == 8 && mc == 14) || (sl == 6 && mc == 19) || (sl == 50 && mc == 1))) continue;
                    DevAlignCfg c{};
                    c.max_subs = ms; c.mm_delta = md; c.slides_per100 = sl; c.min_core_len = mc;
                    const int rows = plan_table_rows(c, top);
                    if (rows > kMaxPhases + 1) return fail("rows out of range");
                    tab.assign((size_t)rows * (top + 1), make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu));
                    if (!plan_table_fill(c, top, rows, tab.data())) return fail("a value does not fit its field");
                    // the direct calls, once per configuration
                    for (int len = 1; len <= top; len++) {
                        nph[len] = plan_geo_direct(len, 0, c).n_phases;
                        for (int ph = 0; ph < nph[len]; ph++) nc[(size_t)len * (kMaxPhases + 1) + ph] = plan_geo_direct(len, ph, c).nc;
                    }
                    for (uint32_t maxlen : kMaxlens) {
                        int want_phases = 0, want_cmax[kMaxPhases + 1] = {0};
                        bool want_fit = true;
                        for (uint32_t len = 1; len <= maxlen; len++) {
                            want_phases = std::max(want_phases, nph[len]);
                            for (int ph = 0; ph < nph[len]; ph++) {
                                const int v = nc[(size_t)len * (kMaxPhases + 1) + ph];
                                if (v > kMaxCoresFast) want_fit = false;
                                want_cmax[ph] = std::max(want_cmax[ph], std::min(v, (int)kMaxCoresFast));
                            }
                        }
                        const ChunkBounds cb = chunk_bounds(tab.data(), (size_t)top + 1, maxlen);         // (a shorter batch reads the longer table)
                        if (cb.max_phases != want_phases || cb.cores_fit != want_fit) {
                            printf("FAIL: max_subs %d mm_delta %d slides %d min_core %d maxlen %u: max_phases %d (want %d) cores_fit %d (want %d)\n", ms, md, sl, mc, maxlen,
                                   cb.max_phases, want_phases, (int)cb.cores_fit, (int)want_fit);
                            return 1;
                        }
                        for (int ph = 0; ph <= kMaxPhases; ph++) {
                            if (cb.cmax_bound[ph] != want_cmax[ph]) {
                                printf("FAIL: max_subs %d mm_delta %d slides %d min_core %d maxlen %u phase %d: cmax_bound %d, want %d\n", ms, md, sl, mc, maxlen, ph,
                                       cb.cmax_bound[ph], want_cmax[ph]);
                                return 1;
                            }
                            if (ph >= cb.max_phases && cb.cmax_bound[ph] != 0) return fail("a row beyond max_phases is not zero");
                        }
                        (want_fit ? some_fit : some_unfit) = true;
                        checked++;
                    }
                }
    if (!some_fit || !some_unfit) return fail("the sweep did not reach both sides of the core cap");
    printf("bounds: %ld (configuration, maxlen) pairs equal the direct calls\n", checked);
    return 0;
}

static int test_family()
{
    for (uint32_t maxlen : kMaxlens) {
        // the ladder in words: reads of up to 128 bases take the 8-word kernels, up to 256 the 16-word ones, up to 16 * kNwLong and
        // 16 * kNwLongest bases the two wider families, longer reads none of them
        int want;
        if (maxlen <= 128) want = 8;
        else if (maxlen <= 256) want = 16;
        else if (maxlen <= 320) want = 20;
        else if (maxlen <= 512) want = 32;
        else want = 0;
        if (window_words_for(maxlen) != want) { printf("FAIL: window_words_for(%u) = %d, want %d\n", maxlen, window_words_for(maxlen), want); return 1; }
        if (want && rd2w_for(maxlen) * 2 != (uint32_t)want) { printf("FAIL: rd2w_for(%u) = %u\n", maxlen, rd2w_for(maxlen)); return 1; }
        if (want && (uint32_t)want * 16 < maxlen) return fail("a family narrower than its reads");
    }
    if (kNwLong != 20 || kNwLongest != 32) return fail("the ladder's constants moved: restate it");
    return 0;
}

// the rules as the phase loop spelled them out before sort_prefix: pass B's work list ..
static uint32_t rule_slist(bool hist_valid, double hist, uint32_t n, uint64_t lanes, uint64_t cap)
{
    const double f = hist_valid ? hist * 1.05 : 0.30;
    uint32_t n_sort = (uint32_t)std::min<uint64_t>({(uint64_t)(f * n) + 4096, lanes, (uint64_t)0x7FFFFFF0});
    if (cap >= 4096) n_sort = (uint32_t)std::min<uint64_t>(n_sort, cap);
    return n_sort >= 4096 ? n_sort : 0;            // (below 4096: no sort)
}
// .. and the wave list (no clamp at 0x7FFFFFF0 there)
static uint32_t rule_wave(bool hist_valid, double hist, uint32_t n, uint64_t n_wave, uint64_t cap)
{
    const double f = hist_valid ? hist * 1.05 : 0.25;
    uint32_t n_sort = (uint32_t)std::min<uint64_t>((uint64_t)(f * n) + 4096, n_wave);
    if (cap >= 4096) n_sort = (uint32_t)std::min<uint64_t>(n_sort, cap);
    return n_sort >= 4096 ? n_sort : 0;
}

static int test_sort_prefix()
{
    const double fracs[] = {0, 0.01, 0.3, 1.0, 16.0};
    const uint32_t reads[] = {1, 4095, 4096, 70001, 1u << 27};
    const uint64_t uppers[] = {0, 4095, 4096, (1ULL << 31) + 5, 1ULL << 36}, caps[] = {0, 4095, 4096, 1000000};
    long checked = 0, ceiling_matters = 0;
    for (int hv = 0; hv < 2; hv++)
        for (double fr : fracs)
            for (uint32_t n : reads)
                for (uint64_t up : uppers)
                    for (uint64_t cap : caps) {
                        const uint32_t b = sort_prefix(hv != 0, fr, 0.30, n, up, cap, kSortCeiling), wb = rule_slist(hv != 0, fr, n, up, cap);
                        const uint32_t w = sort_prefix(hv != 0, fr, 0.25, n, up, cap, kNoCeiling), ww = rule_wave(hv != 0, fr, n, up, cap);
                        if (b != wb || w != ww) {
                            printf("FAIL: sort_prefix hist %d frac %g reads %u upper %llu cap %llu: pass B %u (rule %u), wave %u (rule %u)\n", hv, fr, n,
                                   (unsigned long long)up, (unsigned long long)cap, b, wb, w, ww);
                            return 1;
                        }
                        // where the ceiling is what tells the two forms apart: only for a list longer than the ceiling itself
                        if (sort_prefix(hv != 0, fr, 0.25, n, up, cap, kSortCeiling) != ww) {
                            if (up <= kSortCeiling) return fail("the ceiling changed a value below it");
                            ceiling_matters++;
                        }
                        checked += 2;
                    }
    printf("sort_prefix: %ld values equal the two rules (%ld grid points where the wave list's missing ceiling shows)\n", checked, ceiling_matters);
    return 0;
}

static int test_main_path()
{
    for (int m = 0; m < 32; m++) {
        const bool wave = m & 1, k2 = m & 2, dbg = m & 4, async = m & 8, light = m & 16;
        if (main_path_common(wave, light ? 100 : 101, k2, dbg, async) != (wave && light && k2 && !dbg && async)) return fail("main_path_common");
    }
    return 0;
}

int main()
{
    if (test_family() || test_main_path() || test_sort_prefix() || test_bounds()) return 1;
    printf("ok\n");
    return 0;
}
