// The plan table and the item decoding of bk_plan_table.h on the host (tests/test_host_plan_table.py compiles this beside a stand-in for
// <hip/hip_runtime.h>; bk_plan_table.h and bk_device.h are the files as they stand).
//   - the table plan_table_fill makes equals direct calls of make_plan, phase_params and core_offsets for every length 0..2000 and every
//     phase, over max_subs 0, 1, 3, 5, 10 and values whose mismatch count caps at 63, both mm_delta values, slides_per100 and min_core_len
//     at the values derive_cfg hands out and at extremes
//   - item_cursor / item_advance / item_decode equal plain / and % for item numbers below, at and above 2^32 and every per_read 1..32
//   - slot_decode equals plain / and % for iv_stride up to 2^31 and iv_cores 1..16; small_div and div32 over their whole stated ranges
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "bk_plan_table.h"

using namespace bk;

static int fail(const char *what) { printf("FAIL: %s\n", what); return 1; }

static int test_table()
{
    const int max_subs_v[] = {0, 1, 3, 5, 10, 25, 40, 63}, mm_delta_v[] = {1, 2};
    const int slides_v[] = {6, 8, 9, 1, 50}, min_core_v[] = {4, 14, 19, 1, 1999};      // (derive_cfg hands out 6, 8, 9 and 4 .. 19)
    const int maxlen = kMaxReadLenAbs;
    std::vector<uint2> tab;
    long entries = 0;
    bool capped = false;
    for (int ms : max_subs_v)
        for (int md : mm_delta_v)
            for (int sl : slides_v)
                for (int mc : min_core_v) {
                    // (the full cross product at the library's own slide rates; the extreme rates with the extreme core lengths only)
                    if ((sl == 1 || sl == 50) && mc != 1 && mc != 14 && mc != 1999) continue;
                    // (.. and the values whose count caps at 63 - schedules of up to 65 phases - at three corners)
                    if (ms >= 25 && !((sl == 8 && mc == 14) || (sl == 6 && mc == 19) || (sl == 50 && mc == 1))) continue;
                    DevAlignCfg c{};
                    c.max_subs = ms; c.mm_delta = md; c.slides_per100 = sl; c.min_core_len = mc;
                    const int rows = plan_table_rows(c, maxlen);
                    if (rows < 2 || rows > kMaxPhases + 1) return fail("rows out of range");
                    tab.assign((size_t)rows * (maxlen + 1), make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu));
                    if (!plan_table_fill(c, maxlen, rows, tab.data())) return fail("a value does not fit its field");
                    int most = 0;
                    for (int len = 0; len <= maxlen; len++) {          // (0: an empty read gets what the direct calls give it)
                        const ReadPlan p = make_plan(len, c);
                        if (p.max_tot_mm == 63) capped = true;
                        most = p.n_phases > most ? p.n_phases : most;
                        for (int ph = 0; ph < rows; ph++) {
                            int mm, cl, cd, dummy[1];
                            phase_params(p, c, ph, mm, cl, cd);
                            const int nc = core_offsets(len, cl, cd, p.max_slides, dummy, 0);
                            const PlanGeo g = plan_lookup(tab.data() + (size_t)ph * (maxlen + 1), (uint32_t)maxlen + 1, len);
                            if (g.cl != cl || g.cd != cd || g.nc != nc || g.mm != mm || g.n_phases != p.n_phases || g.max_slides != p.max_slides) {
                                printf("FAIL: max_subs %d mm_delta %d slides %d min_core %d len %d phase %d: table {%d %d %d %d %d %d}, direct {%d %d %d %d %d %d}\n", ms, md,
                                       sl, mc, len, ph, g.cl, g.cd, g.nc, g.mm, g.n_phases, g.max_slides, cl, cd, nc, mm, p.n_phases, p.max_slides);
                                return 1;
                            }
                            entries++;
                        }
                    }
                    if (rows != most + 1) return fail("rows is not the longest schedule + 1");
                    // a shorter batch reads the longer table; a length past the staged part reads the last staged entry, never past it
                    const PlanGeo a = plan_lookup(tab.data(), 37, 36), z = plan_lookup(tab.data(), 37, 500), l = plan_lookup(tab.data(), (uint32_t)maxlen + 1, 36);
                    if (a.cl != l.cl || a.nc != l.nc || z.cl != l.cl || z.cd != l.cd || z.nc != l.nc) return fail("plan_lookup's bound");
                }
    if (!capped) return fail("no configuration reached the cap of 63 mismatches");
    printf("table: %ld entries equal the direct calls\n", entries);
    return 0;
}

static int test_small_div()
{
    for (uint32_t d = 1; d <= kSmallDivMaxD; d++) {
        const SmallDiv v = small_div_make(d);
        for (uint32_t x = 0; x < kSmallDivMaxX; x++)
            if (small_div(x, v) != x / d) { printf("FAIL: small_div %u / %u\n", x, d); return 1; }
    }
    std::mt19937_64 rng(5);
    const uint32_t ds[] = {1, 2, 3, 5, 7, 255, 256, 257, 3001, 65535, 65536, 65537, 1000003, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    std::vector<uint32_t> dv(ds, ds + sizeof(ds) / sizeof(ds[0]));
    for (int i = 0; i < 2000; i++) dv.push_back((uint32_t)(rng() >> (rng() % 32)) | 1u), dv.push_back(1u + (uint32_t)(rng() % 0x80000000ULL));
    for (uint32_t d : dv) {
        const Div32 v = div32_make(d);
        for (int i = 0; i < 400; i++) {
            uint32_t n = (uint32_t)rng();
            if (i < 8) n = (uint32_t)(i < 4 ? (uint64_t)d * (uint32_t)(rng() % 40) + (i & 1 ? d - 1 : 0) : 0xFFFFFFFFu - (uint32_t)i);      // around multiples of d, at the top
            if (div32(n, v) != n / d) { printf("FAIL: div32 %u / %u = %u\n", n, d, div32(n, v)); return 1; }
        }
    }
    return 0;
}

// pass A as the kernel runs it: `blocks` blocks, tiles of `per_tile` items, lanes at offsets 0 .. per_tile - 1
static int test_items()
{
    std::mt19937_64 rng(9);
    long checked = 0;
    for (uint32_t per_read = 1; per_read <= 32; per_read++)
        for (uint32_t cmax = 1; cmax <= per_read && cmax <= 16; cmax++) {
            if (per_read % cmax) continue;                 // per_read = strand passes x cmax
            const uint32_t per_tile = 512;
            if (per_tile > kItemMaxLaneOfs) return fail("tile wider than item_decode's range");
            // grids whose item numbers stay below 2^32, cross it, and start above it
            const uint64_t starts[] = {0, (1ULL << 32) - 5 * per_tile - 3, (1ULL << 32) - per_tile, 1ULL << 32, (1ULL << 32) + 12345, (1ULL << 36) + 77};
            for (uint64_t first_tile_item : starts) {
                const uint32_t blocks = 1 + (uint32_t)(rng() % 16384);
                const ItemGeo g = item_geo_make(per_read, cmax, (uint64_t)blocks * per_tile);
                // a block whose first tile starts at first_tile_item rounded down to a tile boundary
                const uint64_t tile0 = first_tile_item / per_tile * per_tile;
                ItemCursor cur = item_cursor(tile0, per_read);
                uint64_t t0 = tile0;
                for (int tile = 0; tile < 40; tile++, t0 += (uint64_t)blocks * per_tile, item_advance(cur, g)) {
                    if (cur.a0 != t0 / per_read || cur.rem0 != t0 % per_read) return fail("item_advance");
                    for (uint32_t ofs = 0; ofs < per_tile; ofs += (tile < 2 ? 1 : 37)) {
                        const uint64_t item = t0 + ofs;
                        uint64_t a;
                        int si, c;
                        item_decode(cur, ofs, g, a, si, c);
                        const uint64_t wa = item / per_read;
                        const uint32_t rem = (uint32_t)(item % per_read);
                        if (a != wa || si != (int)(rem / cmax) || c != (int)(rem % cmax)) {
                            printf("FAIL: item %llu per_read %u cmax %u: (%llu %d %d), want (%llu %u %u)\n", (unsigned long long)item, per_read, cmax, (unsigned long long)a, si, c,
                                   (unsigned long long)wa, rem / cmax, rem % cmax);
                            return 1;
                        }
                        checked++;
                    }
                }
            }
        }
    printf("items: %ld decoded\n", checked);
    return 0;
}

static int test_slots()
{
    std::mt19937_64 rng(13);
    const uint32_t strides[] = {1, 2, 3, 255, 256, 3001, 65536, 1000000, 50000000, 0x7FFFFFFFu, 0x80000000u};
    long checked = 0;
    for (uint32_t stride : strides)
        for (uint32_t cores = 1; cores <= 16; cores++) {
            const SlotGeo g = slot_geo_make(stride, cores);
            const uint64_t planes = 2ULL * cores, n_slots = std::min<uint64_t>(planes * stride, 1ULL << 32);      // (the work list holds 32-bit slots)
            for (int i = 0; i < 3000; i++) {
                uint64_t s = rng() % n_slots;
                if (i < 64) { const uint64_t plane = (uint64_t)(i / 4) % planes; s = plane * stride + (i & 1 ? stride - 1 : 0); if (i & 2) s = n_slots - 1 - (uint64_t)(i / 4); if (s >= n_slots) s = n_slots - 1; }
                uint32_t a;
                int st, c;
                slot_decode((uint32_t)s, g, a, st, c);
                const uint32_t sc = (uint32_t)(s / stride);
                if (a != (uint32_t)(s % stride) || st != (int)(sc / cores) || c != (int)(sc % cores)) {
                    printf("FAIL: slot %llu stride %u cores %u: (%u %d %d)\n", (unsigned long long)s, stride, cores, a, st, c);
                    return 1;
                }
                checked++;
            }
        }
    printf("slots: %ld decoded\n", checked);
    return 0;
}

int main()
{
    if (test_small_div() || test_items() || test_slots() || test_table()) return 1;
    printf("ok\n");
    return 0;
}
