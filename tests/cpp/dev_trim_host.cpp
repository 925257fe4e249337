// dev_trim_host.cpp - bk_dev_trim.h (adaptive_trim_dev<8|32>, pe_window_ok, pe_window_key<0|8|32>) compiled for the host as it stands and
// run against the CPU oracle's ora_adaptive_trim (tests/test_host_devtrim.py puts an unchanged copy of the header beside a bk_dev_util.h
// that holds nib16, top_mask and flags_to_bits16 as they stand in the device sources plus host forms of the intrinsics, and links
// oracle/bk_oracle.c).  The case generator below is the only one: `dump` writes its cases to a file for tests/test_gpu_dev_trim.py.
//   dev_trim_host [cases]                          run the generator against the oracle (default 400000 cases), print `ok`
//   dev_trim_host dump <atw> <cases> <scans> <file>  write cases and scan groups for one ATW (8 or 32)
// File (little endian): uint32 n, row_bases, tgt_bases, 0; int32[n] len, min_trim, max_mm, min_flank, family, refused, group, order;
// uint64[n] t; uint8[n * row_bases] reads; uint8[tgt_bases] target (one byte per base; rubbish nibbles 0..15 outside reads and windows).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "bk_dev_trim.h"
#include "bk_oracle.h"

using namespace bk;

enum { F_SUBS, F_SHORT, F_LONG, F_BIT63, F_WORDS, F_MM_FIRST, F_MM_LAST, F_TIE1, F_TIE1_LESS, F_TIE2, F_TIE2_LESS, F_EQ_TIE, F_QUIRK, kFamilies };
enum { R_LEN24 = 1, R_LEN_CAP = 2, R_TRIM14 = 4, R_TRIM_OVER = 8, R_MM16 = 16, R_FLANK11 = 32 };

struct Item {
    int len = 0, min_trim = 0, max_mm = 0, min_flank = 0, family = 0, refused = 0;
    std::vector<uint8_t> read;      // row_bases bytes: the read, rubbish nibbles behind it
    std::vector<uint8_t> targ;      // rubbish, the window(s), at least 32 bases of rubbish; a multiple of 64 bases
    std::vector<uint32_t> ts;       // where the windows start in targ; more than one = a scan group (the same read at each)
};

static int row_words(int atw) { return 4 * atw + 2; }     // a read of 64 atw + 1 bases (refused by adaptive_trim_dev, scanned by pe_window_ok) and the word behind

struct Gen {
    std::mt19937_64 rng;
    int atw;
    Gen(int atw_, uint64_t seed) : rng(seed), atw(atw_) {}
    uint32_t r(uint32_t k) { return (uint32_t)(rng() % k); }
    int range(int lo, int hi) { return lo + (int)r((uint32_t)(hi - lo + 1)); }

    int pick_len()
    {
        static const int l8[] = {25, 26, 63, 64, 65, 127, 128, 129, 511, 512}, l32[] = {25, 513, 1023, 1024, 1025, 2000, 2047, 2048};
        if (r(3) == 0) return atw == 8 ? l8[r(10)] : l32[r(8)];
        return range(25, atw == 8 ? 300 : 2048);
    }
    void runs(std::vector<uint8_t> &m, int from, int to, int mm_max, int match_max, int flank)
    {
        bool mm = r(2) != 0;
        for (int p = from; p < to;) {
            int rl = mm ? range(1, mm_max) : range(1, match_max);
            if (!mm && r(4) == 0) { const int pick[4] = {7, 8, flank > 1 ? flank - 1 : 1, flank > 0 ? flank : 1}; rl = pick[r(4)]; }
            for (int k = 0; k < rl && p < to; k++) m[p++] = mm;
            mm = !mm;
        }
    }
    // k mismatching bases at random places of [from, to)
    void scatter(std::vector<uint8_t> &m, int from, int to, int k)
    {
        while (k > 0) { const int p = range(from, to - 1); if (!m[p]) { m[p] = 1; k--; } }
    }
    void params(Item &it)
    {
        it.min_trim = r(3) == 0 ? it.len : range(15, it.len);
        it.max_mm = (int)r(17);
        it.min_flank = (int)r(12);
        if (it.max_mm == 16) it.refused |= R_MM16;
        if (it.min_flank == 11) it.refused |= R_FLANK11;
        const uint32_t k = r(64);
        if (k == 0) { it.min_trim = 14; it.refused |= R_TRIM14; }
        if (k == 1) { it.min_trim = it.len + 1; it.refused |= R_TRIM_OVER; }
    }
    // the read (random bases) in its row, and one window per mask: the read's base where the mask is 0, another base where it is 1
    void lay_out(Item &it, const std::vector<std::vector<uint8_t>> &masks, bool rare)
    {
        const int row_bases = 16 * row_words(atw);
        it.read.resize(row_bases);
        for (int j = 0; j < row_bases; j++) it.read[j] = (uint8_t)(j < it.len ? r(4) : r(16));
        int n_at = -1, n_both = 0, eos_at = -1;
        if (rare && r(8) == 0) { n_at = range(0, it.len - 1); n_both = (int)r(2); it.read[n_at] = 4; }
        if (rare && r(8) == 0) eos_at = range(0, it.len - 1);
        for (uint32_t k = r(64); k > 0; k--) it.targ.push_back((uint8_t)r(16));
        for (const auto &m : masks) {
            it.ts.push_back((uint32_t)it.targ.size());
            for (int j = 0; j < it.len; j++) {
                uint8_t b = it.read[j] < 4 ? it.read[j] : (uint8_t)r(4);
                if (m[j]) b = (uint8_t)((b + 1 + r(3)) & 3);
                if (j == n_at && n_both) b = 4;                                  // N against N: a match in the reference
                if (j == eos_at) b = 7;
                it.targ.push_back(b);
            }
            for (uint32_t k = r(71); k > 0; k--) it.targ.push_back((uint8_t)r(16));
        }
        for (int k = 0; k < 32; k++) it.targ.push_back((uint8_t)r(16));
        while (it.targ.size() % 64) it.targ.push_back((uint8_t)r(16));
    }
    void base_mask(Item &it, std::vector<uint8_t> &m, int fam)
    {
        m.assign(it.len, 0);
        if (fam == F_SUBS) {
            static const int rate[5] = {0, 1, 5, 15, 40};
            const int pc = rate[r(5)];
            for (int j = 0; j < it.len; j++) m[j] = r(100) < (uint32_t)pc;
        } else if (fam == F_SHORT) runs(m, 0, it.len, 3, 40, it.min_flank);
        else runs(m, 0, it.len, 70, 200, it.min_flank);
    }

    Item next()
    {
        Item it;
        std::vector<uint8_t> m;
        const uint32_t f = r(32), lk = r(48);
        it.family = f < 14 ? F_SUBS : f < 20 ? F_SHORT : f < 25 ? F_LONG : f == 25 ? F_BIT63 : f == 26 ? F_WORDS : f == 27 ? (r(2) ? F_MM_FIRST : F_MM_LAST)
                  : f == 28 ? (r(2) ? F_TIE1 : F_TIE1_LESS) : f == 29 ? (r(2) ? F_TIE2 : F_TIE2_LESS) : f == 30 ? F_EQ_TIE : F_QUIRK;
        if (lk == 0 || (lk == 1 && atw == 8)) {                                  // refused lengths, among the substitution cases
            it.family = F_SUBS;
            it.len = lk == 0 ? 24 : 513;
            it.refused |= lk == 0 ? R_LEN24 : R_LEN_CAP;
            params(it);
            if (it.refused & R_TRIM14) { it.refused &= ~R_TRIM14; it.min_trim = 15; }          // one refusal per case where the length is the point
            base_mask(it, m, F_SUBS);
            lay_out(it, {m}, false);
            return it;
        }
        it.len = pick_len();
        switch (it.family) {
        case F_SUBS: case F_SHORT: case F_LONG:
            params(it);
            base_mask(it, m, it.family);
            break;
        case F_BIT63: {                                                         // a mismatching run whose last base is bit 63 of a map word
            if (it.len < 70) it.len = range(70, atw == 8 ? 512 : 2048);
            params(it);
            m.assign(it.len, 0);
            for (int j = 0; j < it.len; j++) m[j] = r(100) < 2;
            const int w = range(0, (it.len - 2) / 64 - 1), rl = r(4) == 0 ? range(1, 70) : range(1, 5);
            for (int p = 64 * w + 63, k = 0; k < rl && p >= 0; k++, p--) m[p] = 1;
            m[64 * w + 64] = 0;
            break;
        }
        case F_WORDS: {                                                         // a matching run over one or more whole map words
            if (it.len < 140) it.len = range(140, atw == 8 ? 512 : 2048);
            params(it);
            m.assign(it.len, 0);
            runs(m, 0, it.len, 3, 40, it.min_flank);
            const int words = it.len / 64, a = range(1, words - 1), b = range(a + 1, words), lo = 64 * a - range(0, 63), hi = 64 * b + range(0, 63);
            for (int p = lo; p < hi && p < it.len; p++) m[p] = 0;
            if (lo > 0) m[lo - 1] = 1;
            if (hi < it.len) m[hi] = 1;
            break;
        }
        case F_MM_FIRST: case F_MM_LAST:
            params(it);
            m.assign(it.len, 0);
            m[it.family == F_MM_FIRST ? 0 : it.len - 1] = 1;
            break;
        case F_TIE1: case F_TIE1_LESS: case F_TIE2: case F_TIE2_LESS: {
            // a stretch of 100 k bases from its start holding exactly k (max_mm + 1) mismatching bases (the reference rejects on equality),
            // or one fewer.  TIE1: the stretch runs to the read's end, so the first ratio test (against the length from the start) meets
            // the tie; TIE2: mismatching bases follow it, so only the second test (against the stretch itself) does
            const int k = range(1, 2), pre = r(3) == 0 ? 0 : range(1, 60);
            const bool second = it.family == F_TIE2 || it.family == F_TIE2_LESS, less = it.family == F_TIE1_LESS || it.family == F_TIE2_LESS;
            const int suf = second ? range(1, 40) : 0;
            it.len = pre + 100 * k + suf;
            it.max_mm = (int)r(16);
            it.min_flank = (int)r(11);
            it.min_trim = r(3) == 0 ? 100 * k : range(15, 100 * k);
            m.assign(it.len, 0);
            for (int p = 0; p < pre; p++) m[p] = 1;
            for (int p = pre + 100 * k; p < it.len; p++) m[p] = 1;
            scatter(m, pre + 10, pre + 100 * k - 10, k * (it.max_mm + 1) - (less ? 1 : 0));
            break;
        }
        case F_EQ_TIE: {
            // A x1 B x2 C with |A x1 B| == |B x2 C|: two stretches of one length from two starts, their mismatches decide
            const int x1 = range(1, 4), x2 = range(1, 4), a = range(10, 40), b = range(10, 60), c = a + x1 - x2;
            it.len = a + x1 + b + x2 + c;
            if (it.len < 25) it.len = 25;
            it.max_mm = range(1, 15);
            it.min_flank = (int)r(11);
            it.min_trim = range(15, a + x1 + b > 15 ? a + x1 + b : 15);
            if (it.min_trim > it.len) it.min_trim = it.len;
            m.assign(it.len, 0);
            for (int p = a; p < a + x1; p++) m[p] = 1;
            for (int p = a + x1 + b; p < a + x1 + b + x2; p++) m[p] = 1;
            break;
        }
        default: {
            // F_QUIRK: A X B x C with |A| == |B x C| and X too long to stretch over: the exact stretch A is found first, and the later one of
            // the same length with mismatches replaces it (`best_mm == 0 ||` in the reference)
            const int x = range(1, 3), b = range(10, 40), c = range(10, 40), L = b + x + c, X = range(12, 40);
            it.len = 2 * L + X;
            it.max_mm = range(4, 15);
            it.min_flank = (int)r(11);
            it.min_trim = range(15, L);
            m.assign(it.len, 0);
            for (int p = L; p < L + X; p++) m[p] = 1;
            for (int p = L + X + b; p < L + X + b + x; p++) m[p] = 1;
            break;
        }
        }
        lay_out(it, {m}, it.family < F_TIE1);
        return it;
    }

    // the same read against 2-12 windows: copies of one mask (order decides), copies with a mismatch more or fewer (same stretch, other
    // count), copies with another base mismatching near an end (another stretch), unrelated masks
    Item next_scan()
    {
        Item it;
        it.len = pick_len();
        it.family = (int)r(3);
        it.max_mm = (int)r(16);
        it.min_flank = 3;
        it.min_trim = r(3) == 0 ? it.len : range(15, it.len);
        std::vector<uint8_t> base(it.len, 0);
        if (it.family == F_SUBS) { const uint32_t pm = r(40); for (int j = 0; j < it.len; j++) base[j] = r(1000) < pm; }
        else if (it.family == F_SHORT) runs(base, 0, it.len, 2, 60, 3);
        else runs(base, 0, it.len, 20, 200, 3);
        std::vector<std::vector<uint8_t>> masks;
        const int n = range(2, 12);
        for (int j = 0; j < n; j++) {
            std::vector<uint8_t> m = base;
            switch (r(6)) {
            case 0: case 1: break;
            case 2: m[range(it.len / 4, 3 * it.len / 4)] ^= 1; break;
            case 3: m[range(0, it.len - 1)] ^= 1; break;
            case 4: m[r(2) ? range(0, 11) : it.len - 1 - range(0, 11)] = 1; break;
            default: { const uint32_t pm = r(60); for (int p = 0; p < it.len; p++) m[p] = r(1000) < pm; }
            }
            masks.push_back(m);
        }
        lay_out(it, masks, false);
        return it;
    }
};

static std::vector<uint64_t> pack4(const std::vector<uint8_t> &b)              // base j of a word in nibble 15 - j; b.size() a multiple of 16
{
    std::vector<uint64_t> w(b.size() / 16, 0);
    for (size_t j = 0; j < b.size(); j++) w[j / 16] |= (uint64_t)(b[j] & 15) << (60 - 4 * (j % 16));
    return w;
}

struct Ora { int r; uint32_t mm, t5, t3; };
static Ora ora(const Item &it, uint32_t t, int min_trim, int min_flank)
{
    Ora o;
    o.r = ora_adaptive_trim((uint32_t)it.len, it.read.data(), it.targ.data() + t, (uint32_t)min_trim, (uint32_t)it.max_mm, (uint32_t)min_flank, &o.mm, &o.t5, &o.t3);
    if (o.r < 0) { o.r = 0; o.mm = o.t5 = o.t3 = 0; }
    return o;
}

// AlignPairedRead's loop (SfxArrayV2.cpp:8400-8470) over the windows in order: the window it ends with, -1 = none
static int sequential_pick(const Item &it, int min_put)
{
    uint32_t prev_best = (uint32_t)it.max_mm + 1;
    int pick = -1;
    for (size_t j = 0; j < it.ts.size(); j++) {
        uint32_t mm, t5, t3;
        const int r = ora_adaptive_trim((uint32_t)it.len, it.read.data(), it.targ.data() + it.ts[j], (uint32_t)min_put, (uint32_t)it.max_mm, 3, &mm, &t5, &t3);
        if (r > min_put || (r == min_put && mm < prev_best)) { prev_best = mm; min_put = r; pick = (int)j; }
    }
    return pick;
}

struct Stats { long n = 0, zero = 0, trimmed = 0, full = 0, fam[kFamilies] = {0}, refused[6] = {0}, scans = 0, scan_none = 0, scan_later = 0, fails = 0; };

#define FAIL(st, ...) do { if ((st).fails++ < 10) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } while (0)

template <int ATW>
static void check(const Item &it, Stats &st)
{
    const std::vector<uint64_t> rdw = pack4(it.read), tgw = pack4(it.targ);
    const bool scan = it.ts.size() > 1;
    unsigned long long best[2] = {~0ULL, ~0ULL};
    int pick[2] = {-1, -1};
    for (size_t j = 0; j < it.ts.size(); j++) {
        const uint32_t t = it.ts[j];
        int mm, t5, t3;
        if (!scan) {
            Ora o = ora(it, t, it.min_trim, it.min_flank);
            if (it.len > 64 * ATW) o = Ora{0, 0, 0, 0};                           // beyond the instantiation's map: the device refuses, the oracle is not asked
            st.n++; st.fam[it.family]++;
            for (int k = 0; k < 6; k++) st.refused[k] += (it.refused >> k) & 1;
            if (o.r == 0) st.zero++; else if (o.r < it.len) st.trimmed++; else st.full++;
            const int r = adaptive_trim_dev<ATW>(rdw.data(), tgw.data(), t, it.len, it.min_trim, it.max_mm, it.min_flank, mm, t5, t3);
            if (r != o.r || mm != (int)o.mm || t5 != (int)o.t5 || t3 != (int)o.t3)
                FAIL(st, "adaptive_trim_dev<%d> family %d len %d t %u min_trim %d max_mm %d min_flank %d: %d mm %d trims %d %d, oracle %d mm %u trims %u %u", ATW,
                     it.family, it.len, t, it.min_trim, it.max_mm, it.min_flank, r, mm, t5, t3, o.r, o.mm, o.t5, o.t3);
        }
        // pe_window_key<ATW>: AdaptiveTrim down to min_put with flanks of 3
        {
            Ora o = ora(it, t, it.min_trim, 3);
            if (it.len > 64 * ATW) o = Ora{0, 0, 0, 0};
            const bool none = o.r < it.min_trim || o.r == 0 || (o.r == it.min_trim && (int)o.mm > it.max_mm);
            const unsigned long long want = none ? ~0ULL : ((unsigned long long)(4095 - o.r) << 52) | ((unsigned long long)o.mm << 40) | j;
            const unsigned long long key = pe_window_key<ATW>(rdw.data(), it.len, tgw.data(), t, it.max_mm, it.min_trim, j, t5, t3);
            if (key != want || (!none && (t5 != (int)o.t5 || t3 != (int)o.t3)))
                FAIL(st, "pe_window_key<%d> family %d len %d t %u min_put %d max_mm %d: key %llx trims %d %d, want %llx trims %u %u", ATW, it.family, it.len, t,
                     it.min_trim, it.max_mm, key, t5, t3, want, o.t5, o.t3);
            if (key < best[0]) { best[0] = key; pick[0] = (int)j; }
        }
        // pe_window_ok / pe_window_key<0>: the read whole
        {
            const Ora o = ora(it, t, it.len, 3);
            const bool ok = o.r == it.len && it.len > 0, acc = ok && (int)o.mm <= it.max_mm;
            const unsigned long long want = !acc ? ~0ULL : ((unsigned long long)(4095 - it.len) << 52) | ((unsigned long long)o.mm << 40) | j;
            const bool got_ok = pe_window_ok(rdw.data(), it.len, tgw.data(), t, it.max_mm, mm);
            const unsigned long long key = pe_window_key<0>(rdw.data(), it.len, tgw.data(), t, it.max_mm, it.len, j, t5, t3);
            if (got_ok != ok || (acc && mm != (int)o.mm) || key != want || t5 != 0 || t3 != 0)
                FAIL(st, "pe_window_ok family %d len %d t %u max_mm %d: ok %d mm %d key %llx, oracle %d mm %u, want key %llx", it.family, it.len, t, it.max_mm,
                     (int)got_ok, mm, key, o.r, o.mm, want);
            if (key < best[1]) { best[1] = key; pick[1] = (int)j; }
        }
    }
    if (scan) {
        // the scan claim: the smallest key is the window AlignPairedRead's loop ends with
        const int want[2] = {it.len > 64 * ATW ? -1 : sequential_pick(it, it.min_trim), sequential_pick(it, it.len)};
        st.scans++;
        if (want[0] < 0) st.scan_none++;
        if (want[0] > 0) st.scan_later++;
        for (int v = 0; v < 2; v++)
            if (pick[v] != want[v])
                FAIL(st, "scan, pe_window_key<%d>: len %d min_put %d max_mm %d, %d windows: smallest key at %d, the loop ends with %d", v ? 0 : ATW, it.len,
                     v ? it.len : it.min_trim, it.max_mm, (int)it.ts.size(), pick[v], want[v]);
    }
}

// the conditions on the case set, from the oracle's answers alone
static int conditions(const Stats &st, int atw)
{
    int bad = 0;
    if (st.zero * 10 < st.n || st.trimmed * 10 < st.n || st.full * 10 < st.n) bad = 1;
    for (int f = 0; f < kFamilies; f++) if (st.fam[f] == 0) bad = 1;
    for (int k = 0; k < 6; k++) if (st.refused[k] == 0 && !((1 << k) == R_LEN_CAP && atw != 8)) bad = 1;
    if (st.scans > 0 && (st.scan_none * 20 < st.scans || st.scan_later * 10 < st.scans || st.scan_none * 10 > st.scans * 9)) bad = 1;
    printf("ATW %d: %ld cases: %ld zero, %ld trimmed, %ld full; %ld scans, %ld without a placement, %ld ending behind the first window%s\n", atw, st.n, st.zero,
           st.trimmed, st.full, st.scans, st.scan_none, st.scan_later, bad ? " - FAIL: the case set misses a condition" : "");
    return bad;
}

template <int ATW>
static int run(long cases, long scans)
{
    Gen g(ATW, 20250 + ATW);
    Stats st;
    for (long i = 0; i < cases; i++) check<ATW>(g.next(), st);
    for (long i = 0; i < scans; i++) check<ATW>(g.next_scan(), st);
    const int bad = conditions(st, ATW);
    if (st.fails) printf("ATW %d: %ld differing results\n", ATW, st.fails);
    return bad || st.fails != 0;
}

template <typename T> static void put(FILE *f, const std::vector<T> &v) { if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { perror("fwrite"); exit(2); } }

static int dump(int atw, long cases, long scans, const char *path)
{
    Gen g(atw, 20250 + atw);
    std::vector<int32_t> len, min_trim, max_mm, min_flank, family, refused, group, order;
    std::vector<uint64_t> t;
    std::vector<uint8_t> reads, tgt;
    for (long i = 0; i < cases + scans; i++) {
        const Item it = i < cases ? g.next() : g.next_scan();
        for (size_t j = 0; j < it.ts.size(); j++) {
            len.push_back(it.len); min_trim.push_back(it.min_trim); max_mm.push_back(it.max_mm); min_flank.push_back(it.min_flank);
            family.push_back(it.family); refused.push_back(it.refused); group.push_back(i < cases ? -1 : (int32_t)(i - cases)); order.push_back((int32_t)j);
            t.push_back(tgt.size() + it.ts[j]);
            reads.insert(reads.end(), it.read.begin(), it.read.end());
        }
        tgt.insert(tgt.end(), it.targ.begin(), it.targ.end());
    }
    FILE *f = fopen(path, "wb");
    if (!f) { perror(path); return 2; }
    const std::vector<uint32_t> head = {(uint32_t)len.size(), (uint32_t)(16 * row_words(atw)), (uint32_t)tgt.size(), 0};
    put(f, head); put(f, len); put(f, min_trim); put(f, max_mm); put(f, min_flank); put(f, family); put(f, refused); put(f, group); put(f, order);
    put(f, t); put(f, reads); put(f, tgt);
    return fclose(f) == 0 ? 0 : 2;
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "dump")) {
        const int atw = atoi(argv[2]);
        if (atw != 8 && atw != 32) return 2;
        return dump(atw, atol(argv[3]), atol(argv[4]), argv[5]);
    }
    const long cases = argc > 1 ? atol(argv[1]) : 400000;
    // three quarters of the cases on the short map: the long one's reads are seven times as long
    if (run<8>(cases - cases / 4, cases / 16) | run<32>(cases / 4, cases / 64)) return 1;
    printf("ok\n");
    return 0;
}
