// bk_plan_table.h - the geometry of a read in a phase as a table, and the item decoding of the two search passes.
//
// What a read's cores look like in a phase - core length, core step, number of cores, mismatches allowed, number of phases - depends on
// (read length, phase, configuration) alone: make_plan + phase_params + core_offsets (bk_device.h), a chain of runtime-divisor
// divisions, an FP64 divide and two data-dependent loops.  The host runs that chain once per (phase, length) and keeps the results in a
// table of one uint2 per entry, one row of `stride` entries per phase (bk_engine.cpp: plan_table_for, cached on the context); the hot
// kernels read an entry instead of deriving it per lane.  The table is filled BY those three functions, so a kernel that keeps the
// direct calls (k_search, k_extend, k_heavy, bk_rescue.hip) and one that reads the table cannot disagree.
//
// The second half is the arithmetic that turns a work item's number into (active read, strand, core) without a runtime-divisor
// division per lane: divisors are small or launch-uniform, so the host passes reciprocals.  Everything here is __host__ __device__
// and is checked on the CPU (tests/test_host_plan_table.py).
#pragma once
#include "bk_device.h"

namespace bk {

struct PlanGeo {
    int cl, cd, nc;             // core length, core step, cores per strand as core_offsets counts them (may exceed kMaxCoresFast)
    int mm, n_phases, max_slides;   // (max_slides: no kernel reads it yet - it is what core_offsets needs, kept for the kernels that still call it)
};

// the derivation itself: what every entry is made from
__host__ __device__ inline PlanGeo plan_geo_direct(int len, int phase, const DevAlignCfg &c)
{
    const ReadPlan p = make_plan(len, c);
    PlanGeo g;
    int dummy[1];
    phase_params(p, c, phase, g.mm, g.cl, g.cd);
    g.nc = core_offsets(len, g.cl, g.cd, p.max_slides, dummy, 0);
    g.n_phases = p.n_phases;
    g.max_slides = p.max_slides;
    return g;
}

// x: cl (11 bits: <= kMaxReadLenAbs) | cd << 11 (11 bits) | nc << 22 (10 bits); y: mm (6 bits: <= 63) | n_phases << 6 (7 bits: <= 65) | max_slides << 13
constexpr int kPlanLenBits = 11, kPlanNcBits = 10, kPlanMmBits = 6, kPlanPhBits = 7;
static_assert(kMaxReadLenAbs < (1 << kPlanLenBits), "core length and step must fit their fields");
__host__ __device__ inline uint2 plan_pack(const PlanGeo &g)
{
    uint2 e;
    e.x = (uint32_t)g.cl | (uint32_t)g.cd << kPlanLenBits | (uint32_t)g.nc << (2 * kPlanLenBits);
    e.y = (uint32_t)g.mm | (uint32_t)g.n_phases << kPlanMmBits | (uint32_t)g.max_slides << (kPlanMmBits + kPlanPhBits);
    return e;
}
__host__ __device__ inline PlanGeo plan_unpack(uint2 e)
{
    PlanGeo g;
    g.cl = (int)(e.x & ((1u << kPlanLenBits) - 1));
    g.cd = (int)(e.x >> kPlanLenBits & ((1u << kPlanLenBits) - 1));
    g.nc = (int)(e.x >> (2 * kPlanLenBits));
    g.mm = (int)(e.y & ((1u << kPlanMmBits) - 1));
    g.n_phases = (int)(e.y >> kPlanMmBits & ((1u << kPlanPhBits) - 1));
    g.max_slides = (int)(e.y >> (kPlanMmBits + kPlanPhBits));
    return g;
}
__host__ __device__ inline bool plan_fits(const PlanGeo &g)         // every field survives the packing
{
    return g.cl >= 0 && g.cl < (1 << kPlanLenBits) && g.cd >= 0 && g.cd < (1 << kPlanLenBits) && g.nc >= 0 && g.nc < (1 << kPlanNcBits) &&
           g.mm >= 0 && g.mm < (1 << kPlanMmBits) && g.n_phases >= 0 && g.n_phases < (1 << kPlanPhBits) && g.max_slides >= 0 &&
           g.max_slides < (1 << (32 - kPlanMmBits - kPlanPhBits));
}

// rows a table for reads of up to maxlen bases has: one per phase any such read runs, and one more - k_flat stages the row of the phase
// behind its own for the reads it hands on, which in the schedule's last phase is past every read's schedule but not past the table
inline int plan_table_rows(const DevAlignCfg &c, int maxlen)
{
    int rows = 0;
    for (int len = 1; len <= maxlen; len++) {
        const int n = make_plan(len, c).n_phases;
        rows = n > rows ? n : rows;
    }
    return rows + 1;
}
// rows x (maxlen + 1) entries, entry [phase * (maxlen + 1) + len], length 0 included (an empty read gets what the direct calls give it;
// c.mm_delta >= 1 keeps its divisions defined).  false: a value does not fit its field (no configuration the library accepts gets there)
inline bool plan_table_fill(const DevAlignCfg &c, int maxlen, int rows, uint2 *out)
{
    const size_t stride = (size_t)maxlen + 1;
    for (int ph = 0; ph < rows; ph++)
        for (int len = 0; len <= maxlen; len++) {
            const PlanGeo g = plan_geo_direct(len, ph, c);
            if (!plan_fits(g)) return false;
            out[ph * stride + len] = plan_pack(g);
        }
    return true;
}

// the entry of a read of `len` bases in a row (in LDS or in global memory) of n entries (DevBatch::plan_n).  n bounds the index: a
// length beyond the batch's longest (a caller that misstated it) reads the row's last entry, never past what was staged
__device__ __forceinline__ PlanGeo plan_lookup(const uint2 *row, uint32_t n, int len)
{
    const uint32_t i = (uint32_t)len < n ? (uint32_t)len : n - 1;
    return plan_unpack(row[i]);
}
// a row of the table into LDS, by a block of `threads` threads (the caller's next barrier stands in front of the look-ups)
__device__ __forceinline__ void plan_stage(uint2 *dst, const DevBatch &b, int phase, uint32_t t, uint32_t threads)
{
    const uint2 *__restrict__ row = b.plan + (size_t)phase * b.plan_stride;
    for (uint32_t i = t; i < b.plan_n; i += threads) dst[i] = row[i];
}

// ---- divisions by launch-uniform numbers ---------------------------------------------------------------------------------------
// x / d for d <= 32 and x < 2048 as (x * m) >> 16, m = 65536 / d + 1: the error term x * (m * d - 65536) <= 2047 * 32 stays below 65536
struct SmallDiv { uint32_t d, m; };
constexpr uint32_t kSmallDivMaxD = 32, kSmallDivMaxX = 2048;
__host__ __device__ inline SmallDiv small_div_make(uint32_t d) { return SmallDiv{d, 65536u / d + 1}; }
__host__ __device__ inline uint32_t small_div(uint32_t x, SmallDiv v) { return (x * v.m) >> 16; }

// n / d for any 32-bit n and d >= 1: the high 64 bits of n * m, m = 2^64 / d rounded up (Lemire, Kaser, Kurz: Faster remainder by
// direct computation, 2019 - exact for every 32-bit n and d); d = 1 has no such m in 64 bits and is taken as it is
struct Div32 { uint64_t m; uint32_t d; };
__host__ __device__ inline Div32 div32_make(uint32_t d) { return Div32{d > 1 ? ~0ULL / d + 1 : 0ULL, d}; }
__host__ __device__ inline uint32_t div32(uint32_t n, Div32 v)
{
    const uint64_t hi = v.m >> 32, lo = v.m & 0xFFFFFFFFu;
    const uint32_t q = (uint32_t)((hi * n + ((lo * n) >> 32)) >> 32);
    return v.d == 1 ? n : q;
}

// ---- pass A: item number -> (position in the active list, strand pass, core) ------------------------------------------------------
// Item i of pass A is (a, si, c) = (i / per_read, i % per_read / cmax, i % per_read % cmax), per_read = strands x cmax <= 32, and
// i = n_act x per_read may pass 2^32.  A block's tiles start at block-uniform items a fixed step apart, so the block divides once
// (item_cursor), advances the pair (a0, rem0) by the step's own quotient and remainder (item_advance: the host divides the step at
// launch) and a lane decodes rem0 + its offset within the tile - below per_read + 256 x ILP, a SmallDiv's range.
struct ItemCursor { uint64_t a0; uint32_t rem0; };                 // the tile starts at item a0 * per_read + rem0, rem0 < per_read
struct ItemGeo { SmallDiv per_read, cmax; uint32_t step_q, step_r; };       // step = step_q * per_read + step_r: a block's stride from tile to tile
constexpr uint32_t kItemMaxLaneOfs = kSmallDivMaxX - kSmallDivMaxD;     // lane offsets within a tile stay below this
inline ItemGeo item_geo_make(uint32_t per_read, uint32_t cmax, uint64_t step)
{
    return ItemGeo{small_div_make(per_read), small_div_make(cmax), (uint32_t)(step / per_read), (uint32_t)(step % per_read)};
}
__host__ __device__ inline ItemCursor item_cursor(uint64_t item, uint32_t per_read)            // (once per block: a plain division)
{
    return ItemCursor{item / per_read, (uint32_t)(item % per_read)};
}
__host__ __device__ inline void item_advance(ItemCursor &t, const ItemGeo &g)
{
    t.a0 += g.step_q;
    t.rem0 += g.step_r;
    if (t.rem0 >= g.per_read.d) { t.rem0 -= g.per_read.d; t.a0++; }
}
__host__ __device__ inline void item_decode(const ItemCursor &t, uint32_t lane_ofs, const ItemGeo &g, uint64_t &a, int &si, int &c)
{
    const uint32_t x = t.rem0 + lane_ofs, q = small_div(x, g.per_read), rem = x - q * g.per_read.d;
    const uint32_t s = small_div(rem, g.cmax);
    a = t.a0 + q;
    si = (int)s;
    c = (int)(rem - s * g.cmax.d);
}

// ---- pass B: interval slot -> (position in the active list, strand, core) -----------------------------------------------------------
// slot = (strand * iv_cores + core) * iv_stride + a (iv_slot, bk_dev_util.h) as pass A's work list holds it: 32 bits
struct SlotGeo { Div32 stride; SmallDiv cores; };
inline SlotGeo slot_geo_make(uint32_t iv_stride, uint32_t iv_cores) { return SlotGeo{div32_make(iv_stride), small_div_make(iv_cores)}; }
__host__ __device__ inline void slot_decode(uint32_t slot, const SlotGeo &g, uint32_t &a, int &strand, int &c)
{
    const uint32_t sc = div32(slot, g.stride);
    a = slot - sc * g.stride.d;
    const uint32_t s = small_div(sc, g.cores);
    strand = (int)s;
    c = (int)(sc - s * g.cores.d);
}

}  // namespace bk
