// dev_search_host.cpp - the search primitives of bk_dev_util.h and bk_dev_k2.h compiled for the host as they stand (tests/cpp/hip_shim stands
// in for the HIP runtime header) and run against plain references over one-byte-per-base arrays; for search_core the reference is the CPU
// oracle (oracle/bk_oracle.c, linked in).  tests/test_host_devsearch.py builds and runs it; tests/test_gpu_dev_search.py runs the same
// generators' cases under the kernels of tests/hip/devtest.hip (`dump`).  The calls of the functions under test are in
// tests/hip/dev_search_eval.h, shared with those kernels; no reference below calls a function of the two headers.
//   dev_search_host <repeat.sfx> <basic.sfx>               every group at its full counts, print `ok` or the first failing cases
//   dev_search_host dump <repeat.sfx> <basic.sfx> <file>   a few thousand cases per group, with the references' answers, to a file
// Groups: (a) row access and bit helpers, (b) cmp_core / cmp_core_from / hamming / hamming_eos, (c) the k-mer table views and sa_get,
// (d) search_core, (e) the second-level keys, (f) find_entry*, classify, write_result.
// File: uint32 count, then per array char name[24], uint32 element size, uint64 bytes, the bytes padded to a multiple of 8.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../hip/dev_search_eval.h"
#include "bk_oracle.h"

using namespace bkt;

static std::mt19937_64 g_rng(20251);
static bool g_full = true;
static uint32_t R(uint32_t k) { return (uint32_t)(g_rng() % k); }
static int range(int lo, int hi) { return lo + (int)R((uint32_t)(hi - lo + 1)); }
static long pick(long full, long small) { return g_full ? full : small; }

// ---- plain packing: base j of a 4 bit/base word in nibble 15 - j, of a 2 bit/base word at bits 63 - 2j, 62 - 2j
static std::vector<uint64_t> pack4(const std::vector<uint8_t> &b, size_t words)
{
    std::vector<uint64_t> w(words, 0);
    for (size_t j = 0; j < b.size(); j++) w[j / 16] |= (uint64_t)(b[j] & 15) << (60 - 4 * (j % 16));
    return w;
}
static std::vector<uint64_t> pack2(const std::vector<uint8_t> &b, size_t words)
{
    std::vector<uint64_t> w(words, 0);
    for (size_t j = 0; j < b.size(); j++) w[j / 32] |= (uint64_t)(b[j] & 3) << (62 - 2 * (j % 32));
    return w;
}
// 16 bases from by[at] on as nibbles, the first on top (plain; `fill` beyond the array's end)
static uint64_t nibbles16(const std::vector<uint8_t> &by, size_t at, int count = 16, uint8_t fill = 0)
{
    uint64_t v = 0;
    for (int j = 0; j < count; j++) v |= (uint64_t)((at + j < by.size() ? by[at + j] : fill) & 15) << (60 - 4 * j);
    return v;
}

// ---- the arrays of a run: checked here, or written to the file
struct Blob { std::string name; uint32_t esize; std::vector<uint8_t> data; };
static std::vector<Blob> g_blobs;
template <typename T> static void keep(const std::string &name, const std::vector<T> &v)
{
    if (g_full) return;
    Blob b{name, (uint32_t)sizeof(T), {}};
    b.data.resize(v.size() * sizeof(T));
    if (!v.empty()) memcpy(b.data.data(), v.data(), b.data.size());
    g_blobs.push_back(std::move(b));
}

struct Group {
    const char *name;
    const char *const *ops;
    std::vector<Case> cs;
    std::vector<Res> want;
    void add(int op, int i0, int i1, int i2, uint64_t a, uint64_t b, uint64_t c, Res w)
    {
        cs.push_back(Case{op, i0, i1, i2, a, b, c});
        want.push_back(w);
    }
    // neighbouring lanes of the kernels get different kinds of case
    void shuffle()
    {
        for (size_t i = cs.size(); i > 1; i--) { const size_t j = g_rng() % i; std::swap(cs[i - 1], cs[j]); std::swap(want[i - 1], want[j]); }
    }
};
static long g_fails = 0;
static void fail_case(const Group &g, size_t i, const Res &got)
{
    const Case &c = g.cs[i];
    const Res &w = g.want[i];
    if (g_fails++ < 12)
        printf("FAIL (%s) %s: case %zu: i %d %d %d a %llx b %llx c %llx: got %llx %llx %llx, want %llx %llx %llx\n", g.name, g.ops[c.op], i, c.i0, c.i1, c.i2,
               (unsigned long long)c.a, (unsigned long long)c.b, (unsigned long long)c.c, (unsigned long long)got.x, (unsigned long long)got.y,
               (unsigned long long)got.z, (unsigned long long)w.x, (unsigned long long)w.y, (unsigned long long)w.z);
}
static bool same(const Res &a, const Res &b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
template <typename F> static void run(const Group &g, F eval)
{
    for (size_t i = 0; i < g.cs.size(); i++) {
        const Res got = eval(g.cs[i], i);
        if (!same(got, g.want[i])) fail_case(g, i, got);
    }
    printf("%s: %zu cases\n", g.name, g.cs.size());
}
static void keep_group(const std::string &name, const Group &g) { keep(name + "_cases", g.cs); keep(name + "_want", g.want); }
static int condition(bool ok, const char *what)
{
    if (!ok) { printf("FAIL: the case set misses a condition: %s\n", what); g_fails++; }
    return ok ? 0 : 1;
}

// =================================================================================================================================
// (a) row access and bit helpers
static const char *const kNamesA[] = {"nib16", "bits64_2", "RdRow::nib16 (4 bit)", "RdRow::nib16 (2 bit)", "RdRow::word16 (4 bit)", "RdRow::word16 (2 bit)",
                                      "spread2to4", "squeeze2", "top_mask", "flags_to_bits16"};
static void group_a()
{
    Group g{"a", kNamesA, {}, {}};
    // random words behind nib16 / bits64_2, seen as nibbles and as 2-bit bases by plain shifts
    const int kWords = 40;
    std::vector<uint64_t> w(kWords + 1);
    for (auto &x : w) x = g_rng();
    for (int pos = 0; pos < 16 * kWords; pos++) {                                       // every pos & 15, phase 0 included
        uint64_t v = 0;
        for (int j = 0; j < 16; j++) { const int p = pos + j; v |= ((w[p / 16] >> (60 - 4 * (p % 16))) & 15) << (60 - 4 * j); }
        g.add(A_NIB16, 0, 0, 0, (uint64_t)pos, 0, 0, Res{v, 0, 0});
    }
    for (int pos = 0; pos < 32 * kWords; pos++) {                                       // every pos & 31
        uint64_t v = 0;
        for (int j = 0; j < 32; j++) { const int p = pos + j; v |= ((w[p / 32] >> (62 - 2 * (p % 32))) & 3) << (62 - 2 * j); }
        g.add(A_BITS64_2, 0, 0, 0, (uint64_t)pos, 0, 0, Res{v, 0, 0});
    }
    // N-free reads in rows of 192 bases, both forms of the same bases; row r starts at word 12 r (4 bit) / 6 r (2 bit)
    const int kRows = 24, kRowBases = 192;
    std::vector<uint8_t> by(kRows * kRowBases + 32);
    for (auto &b : by) b = (uint8_t)R(4);
    const std::vector<uint64_t> rd4 = pack4(by, by.size() / 16 + 1), rd2 = pack2(by, by.size() / 32 + 1);
    for (int r = 0; r < kRows; r++) {
        for (int pos = 0; pos <= kRowBases; pos++) {
            const Res want{nibbles16(by, (size_t)r * kRowBases + pos), 0, 0};
            g.add(A_ROW4_NIB16, 0, 0, 0, (uint64_t)pos, 12ULL * r, 6ULL * r, want);
            g.add(A_ROW2_NIB16, 0, 0, 0, (uint64_t)pos, 12ULL * r, 6ULL * r, want);
        }
        for (int k = 0; k < kRowBases / 16; k++) {
            const Res want{nibbles16(by, (size_t)r * kRowBases + 16 * k), 0, 0};
            g.add(A_ROW4_WORD16, 0, 0, 0, (uint64_t)k, 12ULL * r, 6ULL * r, want);
            g.add(A_ROW2_WORD16, 0, 0, 0, (uint64_t)k, 12ULL * r, 6ULL * r, want);
        }
    }
    for (long i = 0; i < pick(20000, 1500); i++) {
        const uint32_t v = (uint32_t)g_rng();
        uint64_t spread = 0, x = g_rng();
        for (int j = 0; j < 16; j++) spread |= (uint64_t)((v >> (30 - 2 * j)) & 3) << (60 - 4 * j);
        g.add(A_SPREAD2TO4, 0, 0, 0, v, 0, 0, Res{spread, 0, 0});
        g.add(A_SQUEEZE2, 0, 0, 0, spread, 0, 0, Res{v, 0, 0});                            // the round trip
        if (i & 1) x |= 0xCCCCCCCCCCCCCCCCULL;                                         // bits 2 and 3 of every nibble set: ignored
        uint32_t sq = 0;
        for (int j = 0; j < 16; j++) sq |= (uint32_t)((x >> (60 - 4 * j)) & 3) << (30 - 2 * j);
        g.add(A_SQUEEZE2, 0, 0, 0, x, 0, 0, Res{sq, 0, 0});
    }
    const int nibs[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 31, 32, 33, 64, 130, 1000};
    for (int n : nibs) {
        uint64_t m = 0;
        for (int j = 0; j < 16 && j < n; j++) m |= 15ULL << (60 - 4 * j);
        g.add(A_TOP_MASK, 0, 0, 0, (uint64_t)n, 0, 0, Res{m, 0, 0});
    }
    for (uint32_t pat = 0; pat < 65536; pat++) {                                        // bit k of pat = the flag of base k
        uint64_t f = 0;
        for (int k = 0; k < 16; k++) f |= (uint64_t)((pat >> k) & 1) << (60 - 4 * k);
        g.add(A_FLAGS_TO_BITS16, 0, 0, 0, f, 0, 0, Res{pat, 0, 0});
    }
    g.shuffle();
    CtxA x{w.data(), rd4.data(), rd2.data()};
    run(g, [&](const Case &c, size_t) { return eval_a(x, c); });
    keep_group("a", g); keep("a_w", w); keep("a_rd4", rd4); keep("a_rd2", rd2);
}

// =================================================================================================================================
// reads in rows of row_bases bases (a multiple of 32), one row per case; both forms packed at the end, a random word behind
struct Rows {
    int row_bases;
    std::vector<uint8_t> by;
    size_t add(const std::vector<uint8_t> &row) { by.insert(by.end(), row.begin(), row.end()); return by.size() / row_bases - 1; }
    uint64_t w4(size_t r) const { return (uint64_t)r * (row_bases / 16); }
    uint64_t w2(size_t r) const { return (uint64_t)r * (row_bases / 32); }
    std::vector<uint64_t> rd4() const { auto v = pack4(by, by.size() / 16 + 1); v.back() = g_rng(); return v; }
    std::vector<uint64_t> rd2() const { auto v = pack2(by, by.size() / 32 + 1); v.back() = g_rng(); return v; }
};

static int pick_len130()
{
    static const int l[] = {1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 130};
    return R(2) ? l[R(18)] : range(1, 130);
}

// (b) compare and distance
static const char *const kNamesB[] = {"cmp_core (pointer row)", "cmp_core (RdRow, 4 bit)", "cmp_core (RdRow, 2 bit)", "cmp_core_from (pointer row)",
                                      "cmp_core_from (RdRow, 2 bit)", "hamming", "hamming_eos"};
static int ref_cmp(const uint8_t *p, const uint8_t *t, int from, int to)              // the per-base loop: nibble values, the first difference decides
{
    for (int i = from; i < to; i++)
        if (p[i] != t[i]) return p[i] < t[i] ? -1 : 1;
    return 0;
}
static void group_b()
{
    Group g{"b", kNamesB, {}, {}};
    Rows rows{224, {}};
    std::vector<uint8_t> tgt;
    long n_cmp = 0, sign[3] = {0, 0, 0}, n_ham = 0, ham_low = 0;
    const long n_cases = pick(300000, 6000);
    for (long it = 0; it < n_cases; it++) {
        const int op = (int)R(kOpsB);
        const bool two = op == B_CMP_ROW2 || op == B_FROM_ROW2, ham = op == B_HAMMING || op == B_HAMMING_EOS, from = op == B_FROM_PTR || op == B_FROM_ROW2;
        const int cl = pick_len130(), ofs = ham ? 0 : range(0, 40), phase = (int)R(16);
        std::vector<uint8_t> row(rows.row_bases);
        for (auto &b : row) b = (uint8_t)(two ? R(4) : R(16));
        for (int j = 0; j < cl; j++) row[ofs + j] = (uint8_t)R(4);
        // the window: rubbish up to the wanted phase, a copy of the core, 20 bases of a, c, g, t behind it
        do tgt.push_back((uint8_t)R(16)); while ((int)(tgt.size() % 16) != phase);
        const size_t t0 = tgt.size();
        for (int j = 0; j < cl + 20; j++) tgt.push_back(j < cl ? row[ofs + j] : (uint8_t)R(4));
        uint8_t *t = tgt.data() + t0, *p = row.data() + ofs;
        if (!ham) {
            static const int starts[] = {0, 16, 32, 9, 11, 13, 9 + 15, 11 + 15, 13 + 15, 13 + 30};      // k, k + 15, k + 30 as bk_search.hip passes them
            const int start = from ? starts[R(10)] : 0;
            if (from && start > 0 && R(2))                                                // differences in front of `start` say nothing
                for (int j = 0; j < start && j < cl; j++) if (R(4) == 0) t[j] = (uint8_t)((t[j] + 1) & 3);
            const int lo = start < cl ? start : cl - 1, kind = (int)R(11);
            int d = -1;                                                                   // the differing base
            switch (kind) {
            case 0: case 10: break;                                                       // equal
            case 1: t[cl] = (uint8_t)((p[cl] & 3) ^ 1); p[cl] = (uint8_t)(p[cl] & 3); break;   // only the first base beyond cl differs: 0
            case 2: d = cl - 1; break;                                                    // only the core's last base
            case 3: d = cl > 15 ? (cl > 16 && R(2) ? 16 : 15) : cl - 1; break;            // base 15 or base 16
            default: d = range(lo, cl - 1); break;
            }
            if (d >= 0) {
                if (kind == 4) t[d] = 4;                                                  // an N in the target: the probe is lower
                else if (kind == 5) t[d] = 7;                                             // a sequence end in the target: the probe is lower
                else if (R(5) < 3) { if (p[d] == 0) p[d] = (uint8_t)range(1, 3); t[d] = (uint8_t)R(p[d]); }         // the probe is higher
                else { if (p[d] == 3) p[d] = (uint8_t)R(3); t[d] = (uint8_t)range(p[d] + 1, 3); }
                if (kind >= 8) for (int j = d + 1; j < cl; j++) if (R(3) == 0) t[j] = (uint8_t)R(4);           // later differences do not matter
            }
            if (!two && R(6) == 0) { const int j = range(0, cl - 1); if (j != d) p[j] = t[j] = 4; }             // N in the read against N in the target: equal
            const int want = ref_cmp(p, t, start, cl);
            if (!from) { n_cmp++; sign[want + 1]++; }
            g.add(op, ofs, cl, start, (uint64_t)t0, 0, 0, Res{(uint64_t)(int64_t)want, 0, 0});
        } else {
            const int limit = (int)R(13);
            int m = (int)R(14);
            if (m > cl) m = cl;
            for (int k = 0; k < m; k++) { const int j = range(0, cl - 1); t[j] = R(8) == 0 ? 4 : (uint8_t)((p[j] + 1 + R(3)) & 3); }
            if (R(8) == 0) { const int j = range(0, cl - 1); p[j] = t[j] = 4; }             // N against N: no mismatch
            const uint32_t e = R(10);
            if (e == 0) t[cl - 1] = 7;                                                    // a sequence end in the last counted base
            else if (e == 1) t[cl] = 7;                                                   // .. just beyond len: not seen
            else if (e == 2) t[range(0, cl - 1)] = 7;
            int cnt = 0;
            bool eos = false;
            for (int j = 0; j < cl; j++) { cnt += p[j] != t[j]; eos |= t[j] == 7; }
            // hamming: `want` is the exact count; what is asserted is that count when it is <= limit, some value > limit otherwise
            const int want = op == B_HAMMING ? cnt : ((eos || cnt > limit) ? 127 : cnt);
            if (op == B_HAMMING) { n_ham++; ham_low += cnt <= limit; }
            g.add(op, 0, cl, limit, (uint64_t)t0, 0, 0, Res{(uint64_t)(int64_t)want, 0, 0});
        }
        const size_t r = rows.add(row);
        g.cs.back().b = rows.w4(r);
        g.cs.back().c = rows.w2(r);
    }
    for (int j = 0; j < 48; j++) tgt.push_back((uint8_t)R(16));
    condition(sign[0] * 5 >= n_cmp && sign[1] * 5 >= n_cmp && sign[2] * 5 >= n_cmp, "each sign of cmp_core at least a fifth of its cases");
    condition(ham_low * 5 >= n_ham && (n_ham - ham_low) * 5 >= n_ham, "each regime of hamming at least a fifth of its cases");
    printf("b: cmp_core %ld cases: %ld below, %ld equal, %ld above; hamming %ld cases, %ld within the limit\n", n_cmp, sign[0], sign[1], sign[2], n_ham, ham_low);
    const std::vector<uint64_t> rd4 = rows.rd4(), rd2 = rows.rd2(), tgt4 = pack4(tgt, tgt.size() / 16 + 2);
    CtxB x{rd4.data(), rd2.data(), tgt4.data()};
    for (size_t i = 0; i < g.cs.size(); i++) {
        const Res got = eval_b(x, g.cs[i]);
        const int64_t gv = (int64_t)got.x, wv = (int64_t)g.want[i].x;
        const bool ok = g.cs[i].op == B_HAMMING && wv > g.cs[i].i2 ? gv > g.cs[i].i2 : gv == wv;
        if (!ok) fail_case(g, i, got);
    }
    printf("b: %zu cases\n", g.cs.size());
    keep_group("b", g); keep("b_rd4", rd4); keep("b_rd2", rd2); keep("b_tgt4", tgt4);
}

// =================================================================================================================================
// (c) the k-mer table views and sa_get
static const char *const kNamesC[] = {"ktab_get", "ktab_get_pair", "core_range", "sa_get<true>", "sa_get<false>"};
static const char *const kViewNames[] = {"ktab32", "ktab64", "ktab_hi + ktab32", "ktab2", "k = 0"};
static void group_c()
{
    Group g{"c", kNamesC, {}, {}};
    const int k = 9;
    const uint64_t ncodes = 1ULL << (2 * k), n = 0x123456789ULL;
    // a non-decreasing table of 4^k + 1 entries (many buckets empty), as plain 64-bit arrays: starts below 2^32, starts from 2^33 on
    std::vector<uint64_t> a32(ncodes + 1), a64(ncodes + 1);
    uint64_t v32 = 0, v64 = (1ULL << 33) + 12345;
    for (uint64_t c = 0; c <= ncodes; c++) {
        if (c) {
            const uint32_t step = R(3) == 0 ? 0 : R(5) == 0 ? R(30000) : R(40);
            v32 += step;
            v64 += R(7) == 0 ? 0 : R(20000) == 0 ? R(1u << 28) : R(50);
            if ((c & 0xFFFF) == 0) v64 += (1ULL << 34) + R(1000);                         // the packed view's groups lie far apart
            if ((c & 0xFFFF) == 0x8000) v64 += 0x90000000ULL;                             // .. and half of a group's offsets have the top bit set
            if (c == ncodes / 2) v32 += 0x80000000u;                                      // .. and half of the 32-bit starts have the top bit set
        }
        a32[c] = v32; a64[c] = v64;
    }
    if (a32[ncodes] >> 32) { printf("FAIL: the 32-bit table overflows\n"); g_fails++; }
    // the views.  Packed (DevIndex::ktab_hi): ktab_hi[g] = tab[g << 16], offsets relative to it, one entry for group 4^k >> 16
    std::vector<uint32_t> t32(ncodes + 1), pk_lo(ncodes + 1), t2(2 * (ncodes + 1));
    std::vector<uint64_t> pk_hi((ncodes >> 16) + 1);
    for (uint64_t gr = 0; gr < pk_hi.size(); gr++) pk_hi[gr] = a64[gr << 16];
    for (uint64_t c = 0; c <= ncodes; c++) {
        t32[c] = (uint32_t)a32[c];
        pk_lo[c] = (uint32_t)(a64[c] - pk_hi[c >> 16]);
        if (a64[c] - pk_hi[c >> 16] > 0xFFFFFFFFULL) { printf("FAIL: a packed offset overflows\n"); g_fails++; break; }
        t2[2 * c] = (uint32_t)a32[c]; t2[2 * c + 1] = (uint32_t)g_rng();                  // {start, anything}
    }
    const std::vector<uint64_t> *plain[kViews] = {&a32, &a64, &a64, &a32, nullptr};
    // codes: every group boundary, both ends, random ones
    std::vector<uint64_t> codes = {0, 1, 2, ncodes - 2, ncodes - 1};
    for (uint64_t b = 0x10000; b < ncodes; b += 0x10000) for (int d = -2; d <= 1; d++) codes.push_back(b + d);
    for (long i = 0; i < pick(4000, 300); i++) codes.push_back(g_rng() % ncodes);
    for (int v = 0; v < V_K0; v++) {
        for (uint64_t c : codes) {
            g.add(C_KTAB_GET, v, 0, 0, c, 0, 0, Res{(*plain[v])[c], 0, 0});
            g.add(C_KTAB_GET_PAIR, v, 0, 0, c, 0, 0, Res{(*plain[v])[c], (*plain[v])[c + 1], 0});
        }
        g.add(C_KTAB_GET, v, 0, 0, ncodes, 0, 0, Res{(*plain[v])[ncodes], 0, 0});
    }
    // core_range: the codes whose first min(cl, k) bases are the core's
    for (int v = 0; v < kViews; v++) {
        for (int cl = 1; cl <= 20; cl++) {
            for (long i = 0; i < pick(120, 12); i++) {
                std::vector<uint8_t> core(16);
                for (auto &b : core) b = (uint8_t)R(16);                                  // beyond the bases looked at: anything, N-like nibbles too
                const int kk = cl < k ? cl : k, kind = (int)(i % 6);
                for (int j = 0; j < kk; j++) core[j] = kind == 1 ? 3 : kind == 2 ? 0 : (uint8_t)R(4);          // 1: all t, reads entry 4^k; 2: all a
                if (kind == 3) core[R((uint32_t)kk)] = 4;                                 // an N inside them: [0, n)
                if (kind == 4) core[kk] = 4;                                              // .. just behind them: no effect
                if (kind == 5) core[kk - 1] = 3;
                bool has_n = false;
                uint64_t c_lo = 0, c_hi = 0;
                for (int j = 0; j < k; j++) {
                    if (j < kk && core[j] >= 4) has_n = true;
                    c_lo = c_lo * 4 + (j < kk ? core[j] & 3 : 0);
                    c_hi = c_hi * 4 + (j < kk ? core[j] & 3 : 3);
                }
                Res want{0, n, 0};
                if (v != V_K0 && !has_n) want = Res{(*plain[v])[c_lo], (*plain[v])[c_hi + 1], 0};
                g.add(C_CORE_RANGE, v, cl, 0, nibbles16(core, 0), 0, 0, want);
            }
        }
    }
    // suffix array elements with high bytes
    const uint64_t n_sa = 5000;
    std::vector<uint32_t> sa_lo(n_sa);
    std::vector<uint8_t> sa_hi(n_sa + 8 - n_sa % 8);
    for (uint64_t i = 0; i < n_sa; i++) { sa_lo[i] = (uint32_t)g_rng(); sa_hi[i] = (uint8_t)range(1, 255); }
    for (long i = 0; i < pick(5000, 500); i++) {
        const uint64_t at = i < 2 ? (i ? n_sa - 1 : 0) : g_rng() % n_sa;
        g.add(C_SA_GET_WIDE, 0, 0, 0, at, 0, 0, Res{(uint64_t)sa_lo[at] + ((uint64_t)sa_hi[at] << 32), 0, 0});
        g.add(C_SA_GET, 0, 0, 0, at, 0, 0, Res{(uint64_t)sa_lo[at], 0, 0});
    }
    g.shuffle();
    CtxC x;
    index_views(x, t32.data(), a64.data(), pk_hi.data(), pk_lo.data(), reinterpret_cast<const uint2 *>(t2.data()), sa_lo.data(), sa_hi.data(), n, k);
    for (size_t i = 0; i < g.cs.size(); i++) {
        const Res got = eval_c(x, g.cs[i]);
        if (!same(got, g.want[i])) { if (g_fails < 12) printf("(view %s) ", kViewNames[g.cs[i].i0]); fail_case(g, i, got); }
    }
    printf("c: %zu cases\n", g.cs.size());
    const std::vector<uint64_t> head = {n, (uint64_t)k};
    keep_group("c", g); keep("c_head", head); keep("c_tab32", t32); keep("c_tab64", a64); keep("c_pk_hi", pk_hi); keep("c_pk_lo", pk_lo); keep("c_tab2", t2);
    keep("c_sa_lo", sa_lo); keep("c_sa_hi", sa_hi);
}

// =================================================================================================================================
// (d) search_core against the oracle
static const char *const kNamesD[] = {"search_core<false> (pointer row)", "search_core<false> (RdRow, 4 bit)", "search_core<false> (RdRow, 2 bit)",
                                      "search_core<true> (pointer row)", "search_core<true> (RdRow, 4 bit)", "search_core<true> (RdRow, 2 bit)"};
struct Sfx {
    ora_sfx *h = nullptr;
    std::vector<uint8_t> seq;                 // one byte per base, sequence ends (7) included
    std::vector<uint32_t> sa;
    std::vector<uint8_t> sa_hi;               // zeros: the elements fit 32 bits (the <true> instantiations run their code path only)
    std::vector<uint64_t> tgt4;
    uint64_t n = 0;
};
static bool load_sfx(const char *path, Sfx &s)
{
    if (ora_sfx_load(path, &s.h) != 0 || s.h->el_size != 4) { printf("FAIL: cannot load %s as an index of 4-byte elements\n", path); return false; }
    s.n = s.h->concat_len;
    s.seq.resize(s.n);
    for (uint64_t i = 0; i < s.n; i++) {
        s.seq[i] = s.h->seq[i] & 15;
        if (s.seq[i] > 4 && s.seq[i] != 7) { printf("FAIL: %s holds base code %d\n", path, s.seq[i]); return false; }
    }
    s.sa.resize(s.n);
    for (uint64_t i = 0; i < s.n; i++) s.sa[i] = (uint32_t)ora_sa_element(s.h, (int64_t)i);
    s.sa_hi.assign(s.n + 8 - s.n % 8, 0);
    s.tgt4 = pack4(s.seq, s.n / 16 + 12);                                                 // sequence-end nibbles behind the last base
    for (uint64_t j = s.n; j < 16 * s.tgt4.size(); j++) s.tgt4[j / 16] |= 7ULL << (60 - 4 * (j % 16));
    return true;
}
// bucket of a suffix: the 2-bit code of its first k bases; one that meets N or a sequence end after j < k bases sorts in the bucket of
// those j bases padded with t (the rule above bk_index.hip's table builder, per base)
static uint64_t plain_bucket(const Sfx &s, uint64_t pos, int k)
{
    uint64_t code = 0;
    bool pad = false;
    for (int j = 0; j < k; j++) {
        const uint8_t b = pos + j < s.n ? s.seq[pos + j] : 7;
        if (b >= 4) pad = true;
        code = code * 4 + (pad ? 3 : b);
    }
    return code;
}
static std::vector<uint64_t> plain_ktab(const Sfx &s, int k)
{
    const uint64_t ncodes = 1ULL << (2 * k);
    std::vector<uint64_t> tab(ncodes + 1, 0);
    uint64_t prev = 0;
    for (uint64_t i = 0; i < s.n; i++) {
        const uint64_t b = plain_bucket(s, s.sa[i], k);
        if (b < prev) { printf("FAIL: the suffix array's buckets of %d bases are not in order at index %llu\n", k, (unsigned long long)i); g_fails++; }
        prev = b;
        tab[b + 1]++;                                                                     // tab[c] = suffixes in buckets below c
    }
    for (uint64_t c = 1; c <= ncodes; c++) tab[c] += tab[c - 1];
    return tab;
}
// the repeat families: runs of >= 1000 suffixes that share their first 25 bases (plain scan of neighbouring suffixes) -> their first indexes
static std::vector<uint64_t> families(const Sfx &s)
{
    std::vector<uint64_t> out;
    uint64_t run0 = 0;
    for (uint64_t i = 0; i + 1 <= s.n; i++) {
        bool shares = i + 1 < s.n;
        for (int j = 0; shares && j < 25; j++) {
            const uint64_t p = (uint64_t)s.sa[i] + j, q = (uint64_t)s.sa[i + 1] + j;
            shares = p < s.n && q < s.n && s.seq[p] == s.seq[q] && s.seq[p] < 4;
        }
        if (!shares) { if (i + 1 - run0 >= 1000) out.push_back(run0); run0 = i + 1; }
    }
    return out;
}
struct SearchStats { long n = 0, absent = 0, one = 0, big = 0; };
static void group_d_config(int cfg, const Sfx &s, int k, bool tab_is_64, bool with_families, SearchStats &st)
{
    Group g{"d", kNamesD, {}, {}};
    Rows rows{160, {}};
    const std::vector<uint64_t> tab = k ? plain_ktab(s, k) : std::vector<uint64_t>();
    std::vector<uint32_t> tab32(tab_is_64 ? 0 : tab.size());
    for (size_t c = 0; c < tab32.size(); c++) tab32[c] = (uint32_t)tab[c];
    const std::vector<uint64_t> fam = with_families ? families(s) : std::vector<uint64_t>();
    if (with_families && fam.empty()) { printf("FAIL: no repeat family of 1000 suffixes sharing 25 bases\n"); g_fails++; return; }
    const uint64_t kNoCap = ~0ULL >> 1;
    const long n_cases = pick(5000, 700);
    for (long it = 0; it < n_cases; it++) {
        const uint32_t kind = R(with_families ? 20 : 11);
        int cl = range(12, 100);
        const int ofs = range(0, 40);
        uint64_t cap = kNoCap;
        std::vector<uint8_t> core;
        uint64_t from = 0;
        if (kind >= 11) {                                                                 // a repeat family at 20, 25, 26 bases (26 ends the run early)
            static const int lens[] = {20, 25, 26};
            cl = lens[R(3)];
            from = s.sa[fam[R((uint32_t)fam.size())] + R(1000)];
        } else if (kind == 0) cl = range(12, 14);                                         // short cores: runs of several suffixes
        if (kind <= 8 || kind >= 11) {                                                    // cut from the target, without a sequence end
            for (int tries = 0; core.empty() && tries < 1000; tries++) {
                if (kind <= 8) from = g_rng() % (s.n - cl);
                bool eos = false;
                for (int j = 0; j < cl; j++) eos |= s.seq[from + j] == 7;
                if (!eos) core.assign(s.seq.begin() + from, s.seq.begin() + from + cl);
                else if (kind >= 11) from = s.sa[fam[R((uint32_t)fam.size())] + R(1000)];
            }
            if (core.empty()) continue;
            if (kind >= 5 && kind <= 7) { const int j = range(0, cl - 1); core[j] = (uint8_t)((core[j] + 1 + R(3)) & 3); }       // one substitution
            if (kind == 8) core[range(0, cl - 1)] = 4;                                    // an N
        } else core.assign(cl, kind == 9 ? 0 : 3);                                        // all a: at or before the first suffix; all t: behind every a,c,g,t suffix
        // the oracle's answer
        const int64_t first = ora_locate_first_exact(s.h, core.data(), cl, 0, (int64_t)s.n - 1, nullptr);
        const int64_t last = first ? ora_locate_last_exact(s.h, core.data(), cl, 0, (int64_t)s.n - 1, nullptr) : 0;
        const uint64_t run_len = first ? (uint64_t)(last - first + 1) : 0;
        if (first && last < first) { printf("FAIL: the oracle's last index lies below its first\n"); g_fails++; }
        if (kind >= 11 || (run_len > 1 && R(3) == 0)) {
            const uint64_t caps[] = {1, 2, 3, 64, run_len, run_len + 1, run_len > 1 ? run_len - 1 : 1, kNoCap};
            cap = caps[R(8)];
        }
        bool has_n = false;
        for (uint8_t b : core) has_n |= b >= 4;
        int op = (int)R(kOpsD);
        if (has_n && op % 3 == D_ROW2) op -= 1;
        std::vector<uint8_t> row(rows.row_bases);
        for (auto &b : row) b = (uint8_t)(op % 3 == D_ROW2 ? R(4) : R(16));
        std::copy(core.begin(), core.end(), row.begin() + ofs);
        const size_t r = rows.add(row);
        // first: the oracle's lower bound (an absent core: z = 1, and what is checked is that `first` parts the suffixes below the core from
        // those above it); count: min(run, cap)
        g.add(op, ofs, cl, cfg, cap, rows.w4(r), rows.w2(r), Res{first ? (uint64_t)(first - 1) : 0, run_len < cap ? run_len : cap, first ? 0u : 1u});
        st.n++; st.absent += run_len == 0; st.one += run_len == 1; st.big += run_len > 64;
    }
    const std::vector<uint64_t> rd4 = rows.rd4(), rd2 = rows.rd2();
    CtxD x;
    index_search(x, s.tgt4.data(), s.sa.data(), s.sa_hi.data(), tab_is_64 || !k ? nullptr : tab32.data(), tab_is_64 && k ? tab.data() : nullptr, s.n, k, rd4.data(), rd2.data());
    for (size_t i = 0; i < g.cs.size(); i++) {
        const Case &c = g.cs[i];
        const Res got = eval_d(x, c), &w = g.want[i];
        bool ok = got.y == w.y;
        if (w.z == 0) ok = ok && got.x == w.x;
        else {
            const uint8_t *p = rows.by.data() + (size_t)i * rows.row_bases + c.i0;
            std::vector<uint8_t> below(c.i1, 7), above(c.i1, 7);                          // (beyond the array's end: sequence ends)
            for (int j = 0; j < c.i1; j++) {
                if (got.x > 0 && got.x <= s.n && (uint64_t)s.sa[got.x - 1] + j < s.n) below[j] = s.seq[(uint64_t)s.sa[got.x - 1] + j];
                if (got.x < s.n && (uint64_t)s.sa[got.x] + j < s.n) above[j] = s.seq[(uint64_t)s.sa[got.x] + j];
            }
            ok = ok && got.x <= s.n && (got.x == 0 || ref_cmp(p, below.data(), 0, c.i1) > 0) && (got.x == s.n || ref_cmp(p, above.data(), 0, c.i1) < 0);
        }
        if (!ok) { if (g_fails < 12) printf("(index %d, k %d%s) ", cfg / 3, k, w.z ? ", absent: first must part the suffixes" : ""); fail_case(g, i, got); }
    }
    printf("d: index %d k %d: %zu cases\n", cfg / 3, k, g.cs.size());
    const std::string nm = "d" + std::to_string(cfg);
    const std::vector<uint64_t> head = {s.n, (uint64_t)k, (uint64_t)(cfg / 3)};
    keep_group(nm, g); keep(nm + "_head", head); keep(nm + "_rd4", rd4); keep(nm + "_rd2", rd2); keep(nm + "_rows", rows.by); keep(nm + "_tab32", tab32);
    keep(nm + "_tab64", tab_is_64 ? tab : std::vector<uint64_t>());
}
static void group_d(const Sfx &rep, const Sfx &basic)
{
    SearchStats st;
    const int ks[3] = {0, 4, 8};
    for (int cfg = 0; cfg < 6; cfg++) group_d_config(cfg, cfg < 3 ? rep : basic, ks[cfg % 3], ks[cfg % 3] == 8, cfg < 3, st);
    printf("d: %ld probes: %ld absent, %ld runs of one, %ld runs longer than 64\n", st.n, st.absent, st.one, st.big);
    condition(st.absent * 10 >= st.n, "a tenth of the probes absent");
    condition(st.one * 10 >= st.n, "a tenth of the probes runs of one");
    condition(st.big * 10 >= st.n, "a tenth of the probes runs longer than 64");
    keep("d_seq0", rep.seq); keep("d_sa0", rep.sa); keep("d_seq1", basic.seq); keep("d_sa1", basic.sa);
}

// =================================================================================================================================
// (e) the second-level keys
static const char *const kNamesE[] = {"k2_make", "kx_make", "k2_cmp", "k2_nkind", "k2_mask", "ktab2_absent", "k2_count_range", "k2_bounds"};
static const uint32_t kAbove = 0xFFFFFFFFu;
static uint8_t base_at(const std::vector<uint8_t> &t, uint64_t p) { return p < t.size() ? t[p] : 7; }
// the 15 bases from p on, 2 bits each from the top, kind 0; with an N or a sequence end among them the bases in front of the first are
// kept, everything from it on is filled with ones, kind 1 (bk_dev_k2.h's opening comment)
static uint32_t plain_key15(const std::vector<uint8_t> &t, uint64_t p)
{
    uint32_t key = 0;
    for (int j = 0; j < 15; j++) {
        const uint8_t b = base_at(t, p + j);
        if (b >= 4) {
            for (int bit = 31 - 2 * j; bit >= 2; bit--) key |= 1u << bit;
            return key | 1u;
        }
        key |= (uint32_t)b << (30 - 2 * j);
    }
    return key;
}
static uint32_t plain_k2(const std::vector<uint8_t> &t, uint64_t pos, int k)
{
    for (int j = 0; j < k; j++) if (base_at(t, pos + j) >= 4) return kAbove;
    return plain_key15(t, pos + k);
}
static uint32_t plain_kx(const std::vector<uint8_t> &t, uint64_t pos, int from, uint32_t before)
{
    if (before == kAbove || (before & 3u) != 0) return kAbove;                             // all ones unless the level before is of kind 0
    return plain_key15(t, pos + from);
}
static uint32_t plain_mask(int rem2)
{
    uint32_t m = 0;
    for (int j = 0; j < rem2 && j < 15; j++) m |= 3u << (30 - 2 * j);
    return m;
}
static void make_cases(Group &g, const std::vector<uint8_t> &t, uint64_t pos, int k)
{
    const uint32_t k2 = plain_k2(t, pos, k), k3 = plain_kx(t, pos, k + 15, k2), k4 = plain_kx(t, pos, k + 30, k3);
    g.add(E_K2_MAKE, k, 0, 0, pos, 0, 0, Res{k2, 0, 0});
    g.add(E_KX_MAKE, k + 15, 0, 0, pos, k2, 0, Res{k3, 0, 0});
    g.add(E_KX_MAKE, k + 30, 0, 0, pos, k3, 0, Res{k4, 0, 0});
}
static void group_e(const Sfx &basic)
{
    Group g{"e", kNamesE, {}, {}};
    // keys of every suffix of `basic`, and of constructed stretches with an N or a sequence end at every place a key looks at
    std::vector<uint8_t> t = basic.seq;
    const int ks[3] = {4, 8, 12};
    struct At { uint64_t pos; int k; };
    std::vector<At> made;
    for (int k : ks)
        for (int p = 0; p < k + 47; p++)                                                  // .. k - 1, k, k + 14, k + 15, k + 29, k + 30, k + 44 among them
            for (int code = 4; code <= 7; code += 3)
                for (int two = 0; two < 2; two++) {
                    const uint64_t at = t.size();
                    for (int j = 0; j < 80; j++) t.push_back((uint8_t)R(4));
                    t[at + p] = (uint8_t)code;
                    if (two) t[at + p + 1 + R(8)] = (uint8_t)(11 - code);                  // a second one behind the first changes nothing
                    made.push_back(At{at, k});
                    if (p > 0) made.push_back(At{at + 1, k});
                }
    for (const At &m : made) make_cases(g, t, m.pos, m.k);
    for (int k : ks) {
        const uint64_t stride = g_full ? 1 : 211;
        for (uint64_t pos = R((uint32_t)stride); pos < basic.n; pos += stride) make_cases(g, t, pos, k);
        for (uint64_t pos = t.size() - 70; pos < t.size(); pos++) make_cases(g, t, pos, k);   // the keys that look beyond the last base
    }
    std::vector<uint64_t> tgt4 = pack4(t, t.size() / 16 + 12);
    for (uint64_t j = t.size(); j < 16 * tgt4.size(); j++) tgt4[j / 16] |= 7ULL << (60 - 4 * (j % 16));
    // k2_mask, k2_cmp, k2_nkind
    for (int rem2 = -3; rem2 <= 20; rem2++) {
        const uint32_t m = plain_mask(rem2);
        g.add(E_K2_MASK, rem2, 0, 0, 0, 0, 0, Res{m, 0, 0});
        for (long i = 0; i < pick(400, 30); i++) {
            uint32_t key = (uint32_t)g_rng();
            if (i % 7 == 0) key = kAbove;
            else if (i % 7 == 1) key |= 3u;                                               // a key must not pass for the all-ones word by its low bits alone
            const uint32_t q2 = (R(2) ? key : (uint32_t)g_rng()) & m;
            const uint32_t km = key & m;
            const int want = key == kAbove ? 1 : km < q2 ? -1 : km > q2 ? 1 : 0;
            g.add(E_K2_CMP, 0, 0, 0, key, m, q2, Res{(uint64_t)(int64_t)want, 0, 0});
            g.add(E_K2_NKIND, 0, 0, 0, key, 0, 0, Res{(key != kAbove && (key & 3u) == 1u) ? 1u : 0u, 0, 0});
        }
    }
    // ktab2_absent: a bitmap of the 32 values of a key's first five bits; absent = no set bit agrees with the probe on the bits the mask keeps
    for (int L = 0; L <= 15; L++) {
        const uint32_t m = plain_mask(L);
        for (long i = 0; i < pick(2000, 60); i++) {
            const uint32_t dens = R(4), q2 = (uint32_t)g_rng() & m;
            uint32_t bitmap = dens == 0 ? 1u << R(32) : dens == 1 ? (uint32_t)g_rng() & (uint32_t)g_rng() & (uint32_t)g_rng() : (uint32_t)g_rng();
            if (i % 16 == 0) bitmap = i % 32 ? 0x80000000u : 1u;
            bool present = false;
            for (uint32_t v = 0; v < 32; v++) present |= ((bitmap >> v) & 1u) && ((v << 27) & m) == (q2 & (31u << 27));
            g.add(E_KTAB2_ABSENT, 0, 0, 0, bitmap, m, q2, Res{present ? 0u : 1u, 0, 0});
        }
    }
    // the key array: buckets side by side, keys sorted inside a bucket and unrelated across buckets, all-ones keys at a bucket's end
    struct Bucket { uint64_t first, cnt; };
    std::vector<Bucket> buckets;
    std::vector<uint32_t> keys;
    const uint64_t cnts[] = {1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 70000, 1048576 + 5};
    std::vector<uint64_t> order(cnts, cnts + 15);
    for (int i = 0; i < 75; i++) order.push_back(i % 3 == 0 ? (uint64_t)range(1, 40) : i % 3 == 1 ? (uint64_t)range(41, 700) : (uint64_t)range(701, 3000));
    for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[g_rng() % i]);
    auto fill_bucket = [&](uint64_t cnt) {
        const uint64_t first = keys.size();
        const uint64_t above = cnt > 3 ? R(4) : 0;
        const uint32_t spread = R(3);                                                     // few distinct keys, some, nearly all distinct
        uint64_t v = R(1u << 20);
        for (uint64_t i = 0; i < cnt - above; i++) {
            const uint64_t room = ((1ULL << 30) - 1 - v) / (cnt - above - i);
            if (spread == 0 ? R(300) == 0 : spread == 1 ? R(8) == 0 : R(8) != 0) v += room ? g_rng() % (2 * room) % ((1ULL << 30) - v) : 0;
            keys.push_back((uint32_t)(v << 2) | (R(9) == 0 ? 1u : 0u));
        }
        std::sort(keys.begin() + first, keys.end());
        for (uint64_t i = 0; i < above; i++) keys.push_back(kAbove);
        return Bucket{first, cnt};
    };
    for (size_t i = 0; i < order.size(); i++) {
        // the bucket's start: every residue mod 16 in turn, random residues mod 256 and mod 4096 (a filler bucket in front makes it so)
        const uint64_t mod = i % 3 == 0 ? 16 : i % 3 == 1 ? 256 : 4096, res = mod == 16 ? (i / 3) % 16 : g_rng() % mod;
        const uint64_t pad = (res + mod - keys.size() % mod) % mod;
        if (pad) fill_bucket(pad);
        buckets.push_back(fill_bucket(order[i]));
    }
    fill_bucket(range(1, 30));
    const uint64_t n = keys.size();
    // the sampled levels (the rule at k_build_k2_levels): sample g of level j is key (g + 1) 16^j - 1, the last clamped to key n - 1, padding all ones;
    // exactly k2s_start(n, kK2Levels + 1) words, so that a whole-line load beyond them is an error under the address sanitizer
    std::vector<uint32_t> k2(k2s_start(n, kK2Levels + 1), kAbove);
    std::copy(keys.begin(), keys.end(), k2.begin());
    for (int j = 1; j <= kK2Levels; j++)
        for (uint64_t s = 0; s < k2s_count(n, j); s++) {
            const uint64_t src = ((s + 1) << (4 * j)) - 1;
            k2[k2s_start(n, j) + s] = keys[src < n ? src : n - 1];
        }
    condition(n > 1200000 && n < 1600000 && k2s_count(n, 5) >= 1, "about 1.3 M keys, level 5 reached");
    bool residues[16] = {false};
    for (const Bucket &b : buckets) residues[b.first % 16] = true;
    condition(std::all_of(residues, residues + 16, [](bool r) { return r; }), "a bucket starting at every residue mod 16");
    for (const Bucket &b : buckets) {
        for (int L = 1; L <= 15; L++) {
            if (!g_full && b.cnt > 300 && R(3)) continue;
            const uint32_t m = plain_mask(L);
            const int n_probes = g_full ? (b.cnt > 60000 ? 4 : 7) : (b.cnt > 60000 ? 1 : 2);
            for (int pr = 0; pr < n_probes; pr++) {
                // a key of the bucket - at random, or next to a sample point - itself or the value one above it; below all; above all
                uint64_t at = b.first + g_rng() % b.cnt;
                if (pr % 2 && b.cnt > 16) { const int j = range(1, 4); const uint64_t s = (((at >> (4 * j)) + 1) << (4 * j)) - 1 + R(3) - 1; if (s >= b.first && s < b.first + b.cnt) at = s; }
                uint32_t q2 = keys[at] & m;
                const uint32_t how = R(8);
                if (how == 0) q2 = 0;
                else if (how == 1) q2 = m;
                else if (how <= 3 && q2 != m) q2 += 1u << (32 - 2 * L);
                uint64_t lt = 0, le = 0;
                for (uint64_t i = b.first; i < b.first + b.cnt; i++) {
                    const uint32_t km = keys[i] == kAbove ? kAbove : keys[i] & m;
                    lt += km < q2; le += km <= q2;
                }
                g.add(E_K2_BOUNDS, L, 0, 0, b.first, b.cnt, (uint64_t)m | (uint64_t)q2 << 32, Res{b.first + lt, b.first + le, 0});
                // k2_count_range on a stretch of the bucket around the probe's place: inside one line, over two or three
                const uint64_t a0 = b.first + (lt > 20 ? lt - R(20) : 0), b0 = std::min(b.first + b.cnt, a0 + 1 + R(44));
                uint64_t lt2 = 0, le2 = 0;
                for (uint64_t i = a0; i < b0; i++) {
                    const uint32_t km = keys[i] == kAbove ? kAbove : keys[i] & m;
                    lt2 += km < q2; le2 += km <= q2;
                }
                g.add(E_K2_COUNT_RANGE, L, 0, 0, a0, b0, (uint64_t)m | (uint64_t)q2 << 32, Res{lt2, le2, 0});
            }
        }
    }
    g.shuffle();
    CtxE x;
    k2_ctx(x, tgt4.data(), k2.data(), n);
    run(g, [&](const Case &c, size_t) { return eval_e(x, c); });
    const std::vector<uint64_t> head = {n};
    keep_group("e", g); keep("e_head", head); keep("e_tgt4", tgt4); keep("e_k2", k2);
}

// =================================================================================================================================
// (f) entries and the result record
static const char *const kNamesF[] = {"find_entry", "find_entry_lds", "classify", "write_result"};
static void group_f()
{
    const uint32_t n_ents[4] = {1, 2, 128, 129};
    for (int tb = 0; tb < 4; tb++) {
        Group g{"f", kNamesF, {}, {}};
        // entries separated by one-base gaps (the sequence end between two sequences)
        const uint32_t n_ent = n_ents[tb];
        std::vector<uint64_t> start(n_ent), end(n_ent);
        std::vector<uint32_t> id(n_ent);
        uint64_t at = tb % 2 ? 5 : 0;
        for (uint32_t i = 0; i < n_ent; i++) { start[i] = at; end[i] = at + (i % 5 == 0 ? 0 : R(3000)); at = end[i] + 2; id[i] = 7 * i + 3; }
        auto both = [&](uint64_t pos, int want) {
            g.add(F_FIND_ENTRY, tb, 0, 0, pos, 0, 0, Res{(uint64_t)(int64_t)want, 0, 0});
            g.add(F_FIND_ENTRY_LDS, tb, 0, 0, pos, 0, 0, Res{(uint64_t)(int64_t)want, 0, 0});
        };
        for (uint32_t i = 0; i < n_ent; i++) {
            both(start[i], (int)i);
            both(end[i], (int)i);
            both((start[i] + end[i]) / 2, (int)i);
            both(end[i] + 1, -1);                                                         // the gap (behind the last entry: beyond the index)
        }
        if (start[0] > 0) { both(start[0] - 1, -1); both(0, -1); }
        both(end[n_ent - 1] + 2, -1);
        both(end[n_ent - 1] + 100000, -1);
        if (tb == 3) {
            // classify: the four rules in order (nothing found; too close to the next best; too many instances; hits)
            for (int low_inst = 0; low_inst <= 4; low_inst++)
                for (int low_mm = 0; low_mm <= 5; low_mm++)
                    for (int nxt = 0; nxt <= 6; nxt++)
                        for (int init = 4; init <= 5; init++)
                            for (int mm_delta = 1; mm_delta <= 2; mm_delta++)
                                for (int max_hits = 1; max_hits <= 3; max_hits++) {
                                    int want = BK_HR_HITS;
                                    if (low_inst == 0 && low_mm == init) want = BK_HR_NONE;
                                    else if (low_inst >= 1 && nxt - low_mm < mm_delta) want = BK_HR_MMDELTA;
                                    else if (low_inst > max_hits) want = BK_HR_HITINSTS;
                                    g.add(F_CLASSIFY, low_inst, low_mm, nxt, (uint64_t)init, (uint64_t)mm_delta, (uint64_t)max_hits, Res{(uint64_t)(int64_t)want, 0, 0});
                                }
            // write_result: every field by the rules restated in its comment (default MLMode)
            const int rslts[] = {BK_HR_NONE, BK_HR_HITS, BK_HR_MMDELTA, BK_HR_HITINSTS, BK_HR_RMMDELTA, 9};
            for (int rslt : rslts)
                for (int max_hits = 1; max_hits <= 5; max_hits += 4) {
                    const int insts[] = {0, 1, 2, max_hits, max_hits + 1, max_hits + 5};
                    for (int low_inst : insts)
                        for (int rep = 0; rep < 3; rep++) {
                            const uint32_t ent = R(n_ent);
                            const uint64_t left = start[ent] + (end[ent] > start[ent] ? g_rng() % (end[ent] - start[ent]) : 0);
                            const int len = range(25, 2000), low_mm = range(0, 60), nxt = range(0, 63), strand = R(2) ? '+' : '-', diag = (int)R(256);
                            const int li = low_inst > max_hits ? max_hits + 1 : low_inst;             // the clamp
                            bk_hit h;
                            memset(&h, 0, sizeof(h));
                            h.rslt = (uint8_t)rslt; h.nar = BK_NAR_NOHIT; h.strand = '?'; h.flags = (uint8_t)diag;
                            if (rslt == BK_HR_HITS && li == 1) {
                                h.nar = BK_NAR_ACCEPTED; h.num_hits = 1; h.strand = (uint8_t)strand; h.chrom_id = id[ent];
                                h.match_loci = (uint32_t)(left - start[ent]); h.match_len = (uint16_t)len; h.mismatches = (uint8_t)low_mm;
                            } else if (rslt == BK_HR_HITS) h.nar = BK_NAR_MULTIALIGN;
                            else if (rslt == BK_HR_MMDELTA) { h.nar = BK_NAR_MMDELTA; h.match_len = (uint16_t)len; }
                            else if (rslt == BK_HR_HITINSTS) { h.nar = BK_NAR_MULTIALIGN; h.match_len = (uint16_t)len; }
                            h.low_hit_instances = (int16_t)li; h.low_mm = (int8_t)low_mm; h.nxt_low_mm = (int8_t)nxt;
                            uint32_t w[6] = {0, 0, 0, 0, 0, 0};
                            memcpy(w, &h, sizeof(h));
                            const uint64_t packed = (uint64_t)len | (uint64_t)low_mm << 16 | (uint64_t)nxt << 24 | (uint64_t)ent << 32 | (uint64_t)strand << 48 | (uint64_t)diag << 56;
                            g.add(F_WRITE_RESULT, rslt, low_inst, max_hits, left, packed, 0, Res{w[0] | (uint64_t)w[1] << 32, w[2] | (uint64_t)w[3] << 32, w[4]});
                        }
                }
        }
        g.shuffle();
        std::vector<bk_hit> out(g.cs.size());
        CtxF x;
        index_entries(x, start.data(), end.data(), id.data(), n_ent, out.data());
        static LdsEntries le;
        threadIdx.x = 0; blockDim.x = 1;
        lds_entries_load(le, x.ix);
        if (le.on != (n_ent <= 128)) { printf("FAIL: lds_entries_load: %u entries, on = %d\n", n_ent, (int)le.on); g_fails++; }
        run(g, [&](const Case &c, size_t i) { return eval_f(x, le, c, (uint32_t)i); });
        const std::string nm = "f" + std::to_string(tb);
        keep_group(nm, g); keep(nm + "_start", start); keep(nm + "_end", end); keep(nm + "_id", id);
    }
}

// =================================================================================================================================
static int write_file(const char *path)
{
    FILE *f = fopen(path, "wb");
    if (!f) { perror(path); return 2; }
    const uint32_t count = (uint32_t)g_blobs.size();
    bool ok = fwrite(&count, 4, 1, f) == 1;
    for (const Blob &b : g_blobs) {
        char name[24] = {0};
        snprintf(name, sizeof(name), "%s", b.name.c_str());
        const uint64_t bytes = b.data.size(), pad = (8 - bytes % 8) % 8, zero = 0;
        ok = ok && fwrite(name, 24, 1, f) == 1 && fwrite(&b.esize, 4, 1, f) == 1 && fwrite(&bytes, 8, 1, f) == 1;
        ok = ok && (bytes == 0 || fwrite(b.data.data(), bytes, 1, f) == 1) && (pad == 0 || fwrite(&zero, pad, 1, f) == 1);
    }
    if (fclose(f) != 0 || !ok) { perror(path); return 2; }
    return 0;
}

int main(int argc, char **argv)
{
    const bool dump = argc == 5 && !strcmp(argv[1], "dump");
    if (!dump && argc != 3) { fprintf(stderr, "usage: dev_search_host [dump] <repeat.sfx> <basic.sfx> [<file>]\n"); return 2; }
    g_full = !dump;
    Sfx rep, basic;
    if (!load_sfx(argv[dump ? 2 : 1], rep) || !load_sfx(argv[dump ? 3 : 2], basic)) return 1;
    group_a();
    group_b();
    group_c();
    group_d(rep, basic);
    group_e(basic);
    group_f();
    ora_sfx_free(rep.h);
    ora_sfx_free(basic.h);
    if (g_fails) { printf("%ld failures\n", g_fails); return 1; }
    if (dump) return write_file(argv[4]);
    printf("ok\n");
    return 0;
}
