// indextest.hip - the index set-up kernels of biokanga_amd/csrc/bk_index.hip under test-only entry points: the file is included as it
// stands, nothing of the library is linked in.  Built as biokanga_amd/lib/libbk_indextest.so (csrc/Makefile); tests/helpers.py
// indextest_lib() loads it.  Every entry point takes raw device pointers with the sizes of the buffers behind them, fills a DevIndex with
// the fields its launcher reads and nothing else, calls the LAUNCHER on the null stream with the arguments bk_image.cpp gives it,
// synchronises and returns the hipError_t.  Arguments that would let a kernel leave its buffers - an empty index, a k outside 2 .. 16, a
// flag granule below a 64-base block, a table or range larger than the sizes stated - are answered with hipErrorInvalidValue and no launch.
#include <vector>

#include "../../biokanga_amd/csrc/bk_index.hip"

using namespace bk;

namespace {

constexpr int kBad = (int)hipErrorInvalidValue;

int finish()
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}

bool k_ok(int k) { return k >= 2 && k <= 16; }

// words of a 4 bit/base target that nib16 may load for a suffix of an index of n bases, `ahead` bases in: the word and the one behind it
bool tgt4_holds(uint64_t tgt4_words, uint64_t n, uint64_t ahead) { return ((n - 1 + ahead) >> 4) + 2 <= tgt4_words; }
// .. and of the 2 bit/base copy (32 bases a word)
bool tgt2_holds(uint64_t tgt2_words, uint64_t n, uint64_t ahead) { return ((n - 1 + ahead) >> 5) + 2 <= tgt2_words; }

}  // namespace

extern "C" {

// kSwBlkShift, kSwMinRun, kSwHead, kSwLevels, kTab2BitmapMax, kK2Levels, kK2Bases, SwGeo<3>::pre, SwGeo<5>::pre, kMaxReadLenAbs
void bkit_consts(uint32_t *out10)
{
    out10[0] = (uint32_t)kSwBlkShift; out10[1] = kSwMinRun; out10[2] = kSwHead; out10[3] = (uint32_t)kSwLevels; out10[4] = (uint32_t)kTab2BitmapMax;
    out10[5] = (uint32_t)kK2Levels; out10[6] = (uint32_t)kK2Bases; out10[7] = (uint32_t)SwGeo<3>::pre; out10[8] = (uint32_t)SwGeo<5>::pre;
    out10[9] = (uint32_t)kMaxReadLenAbs;
}

// seq: n bytes, from the allocation's start (the kernel loads 16 bytes at a time from multiples of 16); tgt4: nwords words
int bkit_pack_target(const uint8_t *seq, uint64_t n, uint64_t *tgt4, uint64_t nwords)
{
    if (n == 0 || nwords == 0 || nwords * 16 < n || ((uintptr_t)seq & 15)) return kBad;
    launch_pack_target(seq, n, tgt4, nwords, 0);
    return finish();
}

// tgt2: tgt2_words words; nflag: nflag_bytes bytes, a multiple of 4, zeroed by the caller
int bkit_pack_target2(const uint64_t *tgt4, uint64_t nwords4, uint64_t *tgt2, uint64_t tgt2_words, unsigned int *nflag, uint64_t nflag_bytes, int flag_shift)
{
    if (nwords4 == 0 || (nwords4 & 3) || flag_shift < 6 || flag_shift > 40 || tgt2_words < nwords4 / 2) return kBad;
    const uint64_t g_last = (nwords4 / 4 - 1) >> (flag_shift - 6);
    if ((nflag_bytes & 3) || ((g_last >> 5) + 1) * 4 > nflag_bytes) return kBad;
    launch_pack_target2(tgt4, nwords4, tgt2, nflag, flag_shift, 0);
    return finish();
}

int bkit_split_sa5(const uint8_t *sa5, uint64_t n, uint32_t *lo, uint8_t *hi)
{
    if (n == 0) return kBad;
    launch_split_sa5(sa5, n, lo, hi, 0);
    return finish();
}

// tab: tab_entries entries of 4 bytes, of 8 bytes (tab64) or of two 4-byte words (pairs); starts: null or starts_words words.  i1 = 0: the whole array
int bkit_build_ktab(const uint64_t *tgt4, uint64_t tgt4_words, const uint32_t *sa_lo, const uint8_t *sa_hi, uint64_t n, void *tab, uint64_t tab_entries, int k,
                    int tab64, int pairs, uint64_t i0, uint64_t i1, unsigned long long *starts, uint64_t starts_words)
{
    if (n == 0 || !k_ok(k) || tab_entries < (1ULL << (2 * k)) + 1 || !tgt4_holds(tgt4_words, n, 0)) return kBad;
    if (i0 > n + 1 || i1 > n + 1 || (i1 != 0 && i1 < i0) || (tab64 && pairs)) return kBad;
    if (starts != nullptr && starts_words < (n >> 6) + 1) return kBad;
    DevIndex ix{};
    ix.tgt4 = tgt4; ix.sa_lo = sa_lo; ix.sa_hi = sa_hi; ix.n = n; ix.k = k;
    launch_build_ktab(ix, tab, k, tab64 != 0, 0, i0, i1, starts, pairs != 0);
    return finish();
}

// k2, k3, k4: key_words words each (k3, k4 may be null); bad: two counters, which the kernel adds to.  i1 = 0: the whole array
int bkit_build_k2(const uint64_t *tgt4, uint64_t tgt4_words, const uint32_t *sa_lo, const uint8_t *sa_hi, uint64_t n, int k, uint32_t *k2, uint32_t *k3,
                  uint32_t *k4, uint64_t key_words, unsigned long long *bad, uint64_t i0, uint64_t i1, int write_k2)
{
    if (n == 0 || !k_ok(k) || key_words < n || k2 == nullptr || bad == nullptr || !tgt4_holds(tgt4_words, n, (uint64_t)k + 2 * kK2Bases)) return kBad;
    if (i0 > n || i1 > n || (i1 != 0 && i1 < i0)) return kBad;
    DevIndex ix{};
    ix.tgt4 = tgt4; ix.sa_lo = sa_lo; ix.sa_hi = sa_hi; ix.n = n; ix.k = k;
    launch_build_k2(ix, k2, k3, k4, bad, 0, i0, i1, write_k2 != 0);
    return finish();
}

int bkit_build_k2_levels(uint32_t *k2, uint64_t n, uint64_t key_words)
{
    if (n == 0 || key_words < k2s_start(n, kK2Levels + 1)) return kBad;
    launch_build_k2_levels(k2, n, 0);
    return finish();
}

// tab: n_entries bucket starts, none above n; k2: n keys; out: n_entries pairs; sa_elem: null or n elements
int bkit_make_ktab2(const uint32_t *tab, const uint32_t *k2, uint64_t n_entries, uint64_t n, void *out, const uint32_t *sa_elem)
{
    if (n == 0 || n_entries == 0 || k2 == nullptr) return kBad;
    launch_make_ktab2(tab, k2, n_entries, n, out, 0, sa_elem);
    return finish();
}

// tab2: n_entries pairs whose first words are in place; k2 may be null
int bkit_fill_ktab2_y(void *tab2, const uint32_t *k2, uint64_t n_entries, const uint32_t *sa_elem)
{
    if (n_entries == 0) return kBad;
    launch_fill_ktab2_y(tab2, k2, n_entries, 0, sa_elem);
    return finish();
}

// off: n_entries words; hi: hi_words words; overflow: one word, zeroed by the caller
int bkit_pack_ktab64(const uint64_t *tab, uint64_t n_entries, uint32_t *off, uint64_t *hi, uint64_t hi_words, uint32_t *overflow)
{
    if (n_entries == 0 || hi_words < ((n_entries - 1) >> 16) + 1) return kBad;
    launch_pack_ktab64(tab, n_entries, off, hi, overflow, 0);
    return finish();
}

// sa: n elements, a permutation of 0 .. n - 1; isa: n entries
int bkit_build_isa(const uint32_t *sa, uint64_t n, uint32_t *isa, uint64_t i0, uint64_t i1)
{
    if (n == 0 || i0 > n || i1 > n || (i1 != 0 && i1 < i0)) return kBad;
    launch_build_isa(sa, n, isa, 0, i0, i1);
    return finish();
}

int bkit_count_nonzero(const uint32_t *flags, uint64_t n, unsigned long long *count)
{
    if (n == 0) return kBad;
    launch_count_nonzero(flags, n, count, 0);
    return finish();
}

// swin: swin_entries entries of `words` 16-byte words, whole blocks of 32
int bkit_build_swin(const uint64_t *tgt2, uint64_t tgt2_words, const uint32_t *sa_lo, const uint8_t *sa_hi, uint64_t n, void *swin, uint64_t swin_entries,
                    int words)
{
    if (n == 0 || (words != 3 && words != 5) || (swin_entries & 31) || swin_entries < n || !tgt2_holds(tgt2_words, n, 64ULL * words)) return kBad;
    DevIndex ix{};
    ix.tgt2 = tgt2; ix.sa_lo = sa_lo; ix.sa_hi = sa_hi; ix.n = n;
    launch_build_swin(ix, swin, words, 0);
    return finish();
}

// map: map_blocks entries, one per block of 32 suffix array indexes (the whole map); swin: swin_blocks blocks of 32 entries.  The map is
// read back first: a slot beyond swin_blocks is refused
int bkit_swin_fill(const uint64_t *tgt2, uint64_t tgt2_words, const uint32_t *sa_lo, const uint8_t *sa_hi, uint64_t n, const uint32_t *map, uint64_t map_blocks,
                   void *swin, uint64_t swin_blocks, int words, uint64_t a, uint64_t e)
{
    if (n == 0 || (words != 3 && words != 5) || a > e || e > n || !tgt2_holds(tgt2_words, n, 64ULL * words)) return kBad;
    if (map_blocks == 0 || map_blocks < ((e + 31) >> kSwBlkShift)) return kBad;
    std::vector<uint32_t> h(map_blocks);
    const hipError_t ce = hipMemcpy(h.data(), map, map_blocks * 4, hipMemcpyDeviceToHost);
    if (ce != hipSuccess) return (int)ce;
    for (uint32_t s : h)
        if (s != kSwNone && s >= swin_blocks) return kBad;
    DevIndex ix{};
    ix.tgt2 = tgt2; ix.sa_lo = sa_lo; ix.sa_hi = sa_hi; ix.n = n;
    launch_swin_fill(ix, map, swin, words, a, e, 0);
    return finish();
}

// flags, incl, map: n_blocks entries; used: one word
int bkit_swin_map(const uint32_t *flags, const uint32_t *incl, uint64_t n_blocks, uint32_t cap_blocks, uint32_t *used, uint32_t *map)
{
    if (n_blocks == 0) return kBad;
    launch_swin_map(flags, incl, n_blocks, cap_blocks, used, map, 0);
    return finish();
}

// w: n_levels core lengths in HOST memory, ascending; brk: n_levels bitmaps of brk_words words each, one behind the other; starts: the
// bitmap k_build_ktab left (starts_words words), or null - then tab32, the 4^k + 1 bucket starts, is read instead
int bkit_swin_breaks(const uint64_t *tgt4, const uint64_t *tgt2, uint64_t tgt2_words, const uint8_t *nflag, uint64_t nflag_bytes, int flag_shift,
                     const uint32_t *sa_lo, const uint8_t *sa_hi, const uint32_t *k2, const uint32_t *tab32, uint64_t n, int k, const int *w, int n_levels,
                     unsigned long long *brk, uint64_t brk_words, uint64_t a, uint64_t e, uint64_t n_words, const unsigned long long *starts, uint64_t starts_words)
{
    if (n == 0 || !k_ok(k) || flag_shift < 6 || flag_shift > 40 || n_levels < 1 || n_levels > kSwLevels || k2 == nullptr) return kBad;
    for (int l = 0; l < n_levels; l++)
        if (w[l] < 1 || w[l] > kMaxReadLenAbs || (l > 0 && w[l] <= w[l - 1])) return kBad;
    if ((a & 63) || a >= e || e > n || n_words > brk_words || n_words * 64 <= e - a) return kBad;
    if (!tgt2_holds(tgt2_words, n, 64) || (((n - 1) >> flag_shift) >> 3) + 1 > nflag_bytes) return kBad;
    if (starts != nullptr ? starts_words < (n >> 6) + 1 : tab32 == nullptr) return kBad;
    DevIndex ix{};
    ix.tgt4 = tgt4; ix.tgt2 = tgt2; ix.nflag = nflag; ix.flag_shift = flag_shift; ix.nflag_bytes = (uint32_t)nflag_bytes;
    ix.sa_lo = sa_lo; ix.sa_hi = sa_hi; ix.k2 = k2; ix.ktab32 = tab32; ix.n = n; ix.k = k;
    unsigned long long *ptr[kSwLevels];
    for (int l = 0; l < n_levels; l++) ptr[l] = brk + (uint64_t)l * brk_words;
    launch_swin_breaks(ix, w, n_levels, ptr, a, e, n_words, starts, 0);
    return finish();
}

// brk: brk_words words, bit i = a run starts at index i of the range, bit n - the range's end - set (read back first: the kernel's scans
// end at it); flags: n_blocks = the range's blocks of 32
int bkit_swin_cover(const unsigned long long *brk, uint64_t brk_words, uint64_t n, uint32_t max_run, uint32_t min_run, uint32_t *flags, uint64_t n_blocks,
                    int first_level)
{
    if (n == 0 || brk_words < (n >> 6) + 1 || n_blocks != ((n + 31) >> kSwBlkShift) || min_run < 2 || max_run < min_run) return kBad;
    unsigned long long last = 0;
    const hipError_t ce = hipMemcpy(&last, brk + (n >> 6), 8, hipMemcpyDeviceToHost);
    if (ce != hipSuccess) return (int)ce;
    if (!((last >> (n & 63)) & 1)) return kBad;
    launch_swin_cover(brk, n, max_run, min_run, flags, n_blocks, first_level, 0);
    return finish();
}

}  // extern "C"
