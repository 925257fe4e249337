// bk_phase_plan.h - what the host decides about a chunk of reads before it launches the phase loop (bk_engine.cpp, align_chunk), stated
// once.  Host only and pure - no HIP calls, no context - so every rule here is checked on the CPU (tests/test_host_phase_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include "bk_plan_table.h"

namespace bk {
// 16-base words of the register-window kernel family (k_prep_fused / k_flat / k_wave <NW>) that takes reads of up to maxlen bases:
// <= 128 / <= 256 / <= 16 * kNwLong / <= 16 * kNwLongest bases; 0: beyond the register-window kernels
inline int window_words_for(uint32_t maxlen) { return maxlen <= 128 ? 8 : maxlen <= 256 ? 16 : maxlen <= 16u * (uint32_t)kNwLong ? kNwLong : maxlen <= 16u * (uint32_t)kNwLongest ? kNwLongest : 0; }
// 64-bit words of a read's 2 bit/base row in that family: half as many (beyond those kernels: the widest family's, for the scratch estimates)
inline uint32_t rd2w_for(uint32_t maxlen) { return (uint32_t)(window_words_for(maxlen) ? window_words_for(maxlen) : kNwLongest) / 2; }
// what a read of up to maxlen bases can need: phases, and cores per strand in each (the most of any length that has the phase, capped at
// kMaxCoresFast; cores_fit: no length goes over that cap).  plan: the host copy of the plan table, rows `stride` entries apart.
struct ChunkBounds { int max_phases = 0, cmax_bound[kMaxPhases + 1] = {0}; bool cores_fit = true; };
inline ChunkBounds chunk_bounds(const uint2 *plan, size_t stride, uint32_t maxlen)
{
    ChunkBounds cb;
    for (uint32_t len = 1; len <= maxlen; len++) {
        const int n_phases = plan_unpack(plan[len]).n_phases;
        cb.max_phases = std::max(cb.max_phases, n_phases);
        for (int ph = 0; ph < n_phases && ph <= kMaxPhases; ph++) {
            const int nc = plan_unpack(plan[(size_t)ph * stride + len]).nc;
            if (nc > kMaxCoresFast) cb.cores_fit = false;
            cb.cmax_bound[ph] = std::max(cb.cmax_bound[ph], std::min(nc, (int)kMaxCoresFast));
        }
    }
    return cb;
}

// what "the main path" means to both of its askers, the phase loop that launches from bounds (align_chunk) and the call that only
// enqueues (align_device); each adds the terms only it has (the chunk's core bound and -N there, the 2-bit target and the scratch here)
inline bool main_path_common(bool use_wave, int heavy_thresh, bool have_k2, bool debug, bool async_phases) { return use_wave && heavy_thresh <= 100 && have_k2 && !debug && async_phases; }

// How much of a work list is sorted when the host does not know its length: the previous chunk's need per read (hist_frac + 5 %; no
// history: default_frac) plus 4096, at most `upper`, `ceiling` and - where they hold 4096 or more: they do not grow for a guess - the
// sort buffers; 0 below 4096.  Pass B's list is clamped at kSortCeiling; the wave list never was (kNoCeiling; see profiles/NOTES.md).
constexpr uint64_t kSortCeiling = 0x7FFFFFF0, kNoCeiling = ~0ULL;
inline uint32_t sort_prefix(bool hist_valid, double hist_frac, double default_frac, uint32_t chunk_reads, uint64_t upper, uint64_t sort_cap, uint64_t ceiling)
{
    uint64_t n_sort = std::min<uint64_t>({(uint64_t)((hist_valid ? hist_frac * 1.05 : default_frac) * chunk_reads) + 4096, upper, ceiling});
    if (sort_cap >= 4096) n_sort = std::min(n_sort, sort_cap);
    return n_sort >= 4096 ? (uint32_t)n_sort : 0u;
}
}  // namespace bk
