// dev_search_eval.h - one case of the search primitives of bk_dev_util.h / bk_dev_k2.h -> the function under test.  Shared by the test-only
// kernels of devtest.hip (one case per lane) and by the CPU twin tests/cpp/dev_search_host.cpp, which compiles the same headers for the
// host: both run literally the same calls.  A case is a function number (op), three ints and three 64-bit words; what they mean per
// group is said at each function.  Nothing here computes an expected value.
#pragma once
#include <string.h>

#include "../../biokanga_amd/csrc/bk_dev_k2.h"

namespace bkt {

using namespace bk;

struct Case { int32_t op, i0, i1, i2; uint64_t a, b, c; };        // 40 bytes
struct Res { uint64_t x, y, z; };                                 // unused words stay 0

// ---- (a) row access and bit helpers.  w: random words (+ one behind); rd4 / rd2: rows in both forms, b / c = a row's first word there
enum { A_NIB16, A_BITS64_2, A_ROW4_NIB16, A_ROW2_NIB16, A_ROW4_WORD16, A_ROW2_WORD16, A_SPREAD2TO4, A_SQUEEZE2, A_TOP_MASK, A_FLAGS_TO_BITS16, kOpsA };
struct CtxA { const uint64_t *w, *rd4, *rd2; };
__device__ inline Res eval_a(const CtxA &x, const Case &c)
{
    Res r = {0, 0, 0};
    RdRow r4, r2;
    r4.p = x.rd4 + c.b; r4.four = true;
    r2.p = x.rd2 + c.c; r2.four = false;
    switch (c.op) {
    case A_NIB16: r.x = nib16(x.w, c.a); break;
    case A_BITS64_2: r.x = bits64_2(x.w, (int)c.a); break;
    case A_ROW4_NIB16: r.x = r4.nib16((int)c.a); break;
    case A_ROW2_NIB16: r.x = r2.nib16((int)c.a); break;
    case A_ROW4_WORD16: r.x = r4.word16((int)c.a); break;
    case A_ROW2_WORD16: r.x = r2.word16((int)c.a); break;
    case A_SPREAD2TO4: r.x = spread2to4((uint32_t)c.a); break;
    case A_SQUEEZE2: r.x = squeeze2(c.a); break;
    case A_TOP_MASK: r.x = top_mask((int)c.a); break;
    case A_FLAGS_TO_BITS16: r.x = flags_to_bits16(c.a); break;
    default: break;
    }
    return r;
}

// ---- (b) compare and distance.  i0 = the core's offset in the read, i1 = cl / len, i2 = start (cmp_core_from) / limit (hamming*), a = target
// position, b / c = the read's first word in rd4 / rd2.  The result is the int, sign-extended
enum { B_CMP_PTR, B_CMP_ROW4, B_CMP_ROW2, B_FROM_PTR, B_FROM_ROW2, B_HAMMING, B_HAMMING_EOS, kOpsB };
struct CtxB { const uint64_t *rd4, *rd2, *tgt4; };
__device__ inline Res eval_b(const CtxB &x, const Case &c)
{
    Res r = {0, 0, 0};
    const uint64_t *row = x.rd4 + c.b;
    RdRow r4, r2;
    r4.p = row; r4.four = true;
    r2.p = x.rd2 + c.c; r2.four = false;
    int v = 0;
    switch (c.op) {
    case B_CMP_PTR: v = cmp_core(row, c.i0, c.i1, row_nib16(row, c.i0) & top_mask(c.i1), x.tgt4, c.a); break;
    case B_CMP_ROW4: v = cmp_core(r4, c.i0, c.i1, row_nib16(r4, c.i0) & top_mask(c.i1), x.tgt4, c.a); break;
    case B_CMP_ROW2: v = cmp_core(r2, c.i0, c.i1, row_nib16(r2, c.i0) & top_mask(c.i1), x.tgt4, c.a); break;
    case B_FROM_PTR: v = cmp_core_from(row, c.i0, c.i1, c.i2, x.tgt4, c.a); break;
    case B_FROM_ROW2: v = cmp_core_from(r2, c.i0, c.i1, c.i2, x.tgt4, c.a); break;
    case B_HAMMING: v = hamming(row, c.i1, x.tgt4, c.a, c.i2); break;
    case B_HAMMING_EOS: v = hamming_eos(row, c.i1, x.tgt4, c.a, c.i2); break;
    default: break;
    }
    r.x = (uint64_t)(int64_t)v;
    return r;
}

// ---- (c) k-mer table views.  i0 = the view (kViews of them, set up by index_views), i1 = cl, a = code / p0 / element index
enum { C_KTAB_GET, C_KTAB_GET_PAIR, C_CORE_RANGE, C_SA_GET_WIDE, C_SA_GET, kOpsC };
enum { V_TAB32, V_TAB64, V_PACKED, V_TAB2, V_K0, kViews };
struct CtxC { DevIndex ix[kViews]; };
// the four views of one table of order k and the index without a table; n = DevIndex::n of every one of them
inline void index_views(CtxC &x, const uint32_t *tab32, const uint64_t *tab64, const uint64_t *pk_hi, const uint32_t *pk_lo, const uint2 *tab2,
                        const uint32_t *sa_lo, const uint8_t *sa_hi, uint64_t n, int k)
{
    memset(&x, 0, sizeof(x));
    for (int v = 0; v < kViews; v++) { x.ix[v].n = n; x.ix[v].k = v == V_K0 ? 0 : k; x.ix[v].sa_lo = sa_lo; x.ix[v].sa_hi = sa_hi; }
    x.ix[V_TAB32].ktab32 = tab32;
    x.ix[V_TAB64].ktab64 = tab64;
    x.ix[V_PACKED].ktab_hi = pk_hi; x.ix[V_PACKED].ktab32 = pk_lo;
    x.ix[V_TAB2].ktab2 = tab2;
}
__device__ inline Res eval_c(const CtxC &x, const Case &c)
{
    Res r = {0, 0, 0};
    const DevIndex &ix = x.ix[c.i0];
    switch (c.op) {
    case C_KTAB_GET: r.x = ktab_get(ix, c.a); break;
    case C_KTAB_GET_PAIR: ktab_get_pair(ix, c.a, r.x, r.y); break;
    case C_CORE_RANGE: core_range(ix, c.a, c.i1, r.x, r.y); break;
    case C_SA_GET_WIDE: r.x = sa_get<true>(ix, c.a); break;
    case C_SA_GET: r.x = sa_get<false>(ix, c.a); break;
    default: break;
    }
    return r;
}

// ---- (d) search_core.  op = 3 * WIDE + the row's form (0 pointer, 1 RdRow of 4 bit/base, 2 RdRow of 2 bit/base); i0 = the core's offset in
// the read, i1 = cl, a = cap, b / c = the read's first word in rd4 / rd2.  x = first, y = count
enum { D_PTR, D_ROW4, D_ROW2, D_WIDE_PTR, D_WIDE_ROW4, D_WIDE_ROW2, kOpsD };
struct CtxD { DevIndex ix; const uint64_t *rd4, *rd2; };
inline void index_search(CtxD &x, const uint64_t *tgt4, const uint32_t *sa_lo, const uint8_t *sa_hi, const uint32_t *tab32, const uint64_t *tab64,
                         uint64_t n, int k, const uint64_t *rd4, const uint64_t *rd2)
{
    memset(&x, 0, sizeof(x));
    x.ix.tgt4 = tgt4; x.ix.sa_lo = sa_lo; x.ix.sa_hi = sa_hi; x.ix.ktab32 = tab32; x.ix.ktab64 = tab64; x.ix.n = n; x.ix.k = k;
    x.rd4 = rd4; x.rd2 = rd2;
}
__device__ inline Res eval_d(const CtxD &x, const Case &c)
{
    Res r = {0, 0, 0};
    const uint64_t *row = x.rd4 + c.b;
    RdRow r4, r2;
    r4.p = row; r4.four = true;
    r2.p = x.rd2 + c.c; r2.four = false;
    switch (c.op) {
    case D_PTR: search_core<false>(x.ix, row, c.i0, c.i1, c.a, r.x, r.y); break;
    case D_ROW4: search_core<false>(x.ix, r4, c.i0, c.i1, c.a, r.x, r.y); break;
    case D_ROW2: search_core<false>(x.ix, r2, c.i0, c.i1, c.a, r.x, r.y); break;
    case D_WIDE_PTR: search_core<true>(x.ix, row, c.i0, c.i1, c.a, r.x, r.y); break;
    case D_WIDE_ROW4: search_core<true>(x.ix, r4, c.i0, c.i1, c.a, r.x, r.y); break;
    case D_WIDE_ROW2: search_core<true>(x.ix, r2, c.i0, c.i1, c.a, r.x, r.y); break;
    default: break;
    }
    return r;
}

// ---- (e) second-level keys.  k2_make: a = pos, i0 = k; kx_make: a = pos, i0 = from, b = before; k2_cmp / ktab2_absent: a, b, c = their
// three arguments; k2_nkind: a = key; k2_mask: i0 = rem2; k2_count_range: L = k2, [a, b), c = m | q2 << 32 -> x = n_lt, y = n_le;
// k2_bounds: a = first, b = cnt, c = m | q2 << 32 -> x = lb, y = ub
enum { E_K2_MAKE, E_KX_MAKE, E_K2_CMP, E_K2_NKIND, E_K2_MASK, E_KTAB2_ABSENT, E_K2_COUNT_RANGE, E_K2_BOUNDS, kOpsE };
struct CtxE { const uint64_t *tgt4; const uint32_t *k2; uint64_t lv[kK2Levels + 2]; };
inline void k2_ctx(CtxE &x, const uint64_t *tgt4, const uint32_t *k2, uint64_t n)
{
    x.tgt4 = tgt4; x.k2 = k2;
    for (int j = 0; j <= kK2Levels + 1; j++) x.lv[j] = j ? k2s_start(n, j) : 0;
}
__device__ inline Res eval_e(const CtxE &x, const Case &c)
{
    Res r = {0, 0, 0};
    unsigned long long lines = 0;
    uint32_t lt = 0, le = 0;
    switch (c.op) {
    case E_K2_MAKE: r.x = k2_make(x.tgt4, c.a, c.i0); break;
    case E_KX_MAKE: r.x = kx_make(x.tgt4, c.a, c.i0, (uint32_t)c.b); break;
    case E_K2_CMP: r.x = (uint64_t)(int64_t)k2_cmp((uint32_t)c.a, (uint32_t)c.b, (uint32_t)c.c); break;
    case E_K2_NKIND: r.x = k2_nkind((uint32_t)c.a) ? 1 : 0; break;
    case E_K2_MASK: r.x = k2_mask(c.i0); break;
    case E_KTAB2_ABSENT: r.x = ktab2_absent((uint32_t)c.a, (uint32_t)c.b, (uint32_t)c.c) ? 1 : 0; break;
    case E_K2_COUNT_RANGE: k2_count_range(x.k2, c.a, c.b, (uint32_t)c.c, (uint32_t)(c.c >> 32), lt, le, lines); r.x = lt; r.y = le; break;
    case E_K2_BOUNDS: k2_bounds(x.k2, x.lv, c.a, c.b, (uint32_t)c.c, (uint32_t)(c.c >> 32), r.x, r.y, lines); break;
    default: break;
    }
    return r;
}

// ---- (f) entries and the result record.  find_entry / find_entry_lds: a = target position; classify: i0, i1, i2, a, b, c = its six
// arguments; write_result: i0 = rslt, i1 = low_inst, i2 = max_hits, a = hit_left, b = len | low_mm << 16 | nxt << 24 | hit_ent << 32 |
// hit_strand << 48 | diag << 56, written to out[slot] and read back from there -> the record's 20 bytes in x, y, z
enum { F_FIND_ENTRY, F_FIND_ENTRY_LDS, F_CLASSIFY, F_WRITE_RESULT, kOpsF };
struct CtxF { DevIndex ix; bk_hit *out; };
inline void index_entries(CtxF &x, const uint64_t *ent_start, const uint64_t *ent_end, const uint32_t *ent_id, uint32_t n_ent, bk_hit *out)
{
    memset(&x, 0, sizeof(x));
    x.ix.ent_start = ent_start; x.ix.ent_end = ent_end; x.ix.ent_id = ent_id; x.ix.n_ent = n_ent; x.out = out;
}
__device__ inline Res eval_f(const CtxF &x, const LdsEntries &le, const Case &c, uint32_t slot)
{
    Res r = {0, 0, 0};
    switch (c.op) {
    case F_FIND_ENTRY: r.x = (uint64_t)(int64_t)find_entry(x.ix, c.a); break;
    case F_FIND_ENTRY_LDS: r.x = (uint64_t)(int64_t)find_entry_lds(le, x.ix, c.a); break;
    case F_CLASSIFY: r.x = (uint64_t)(int64_t)classify(c.i0, c.i1, c.i2, (int)c.a, (int)c.b, (int)c.c); break;
    case F_WRITE_RESULT: {
        DevAlignCfg cfg;
        memset(&cfg, 0, sizeof(cfg));
        cfg.max_hits = c.i2;
        DevBatch b;
        memset(&b, 0, sizeof(b));
        b.out = x.out;
        write_result(x.ix, cfg, b, slot, (int)(c.b & 0xFFFF), c.i0, c.i1, (int)(int8_t)(c.b >> 16), (int)(int8_t)(c.b >> 24), c.a, (int)((c.b >> 32) & 0xFFFF),
                     (int)((c.b >> 48) & 0xFF), (int)(c.b >> 56));
        const bk_hit h = x.out[slot];
        uint32_t w[6] = {0, 0, 0, 0, 0, 0};
        memcpy(w, &h, sizeof(h));
        r.x = w[0] | (uint64_t)w[1] << 32; r.y = w[2] | (uint64_t)w[3] << 32; r.z = w[4];
        break;
    }
    default: break;
    }
    return r;
}

}  // namespace bkt
