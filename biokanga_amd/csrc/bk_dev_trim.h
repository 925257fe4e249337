// bk_dev_trim.h - CSfxArrayV3::AdaptiveTrim on the device, shared by the chimeric form of k_heavy (bk_heavy.hip) and the paired-end
// orphan recovery (bk_rescue.hip), and the orphan recovery's window check (pe_window_ok, pe_window_key) - here so that the test kernels of
// tests/hip/devtest.hip can include them as they stand.
#pragma once
#include "bk_dev_util.h"

namespace bk {

// CSfxArrayV3::AdaptiveTrim (SfxArrayV2.cpp:5482-5682) for one candidate: the longest stretch of the read that starts and ends in a
// run of >= min_flank matching bases, is at least min_trim long and stays under (max_mm + 1) % mismatches - counting, as the
// reference does, every base of a mismatching run against the length from the stretch's start (first test) and against the
// stretch itself (second test), in double precision.  The reference keeps a table of match / mismatch runs; here the runs are
// read off a bitmap of the mismatching positions (bit i of word i / 64): ATW = 8 words for reads of up to 512 bases (registers), 32 for
// the longest reads the boundary takes (2000 bases; the map then lives in scratch memory - its own instantiation of the kernel).
template <int ATW>
__device__ __forceinline__ int at_run_end(const uint64_t (&bm)[ATW], int p, int n)    // first q > p with bit(q) != bit(p), or n
{
    constexpr int kATWords = ATW;
    const int bit = (int)((bm[p >> 6] >> (p & 63)) & 1);
    int w = p >> 6;
    uint64_t x = (bit ? ~bm[w] : bm[w]) >> (p & 63);
    if (x) { const int q = p + (__ffsll((unsigned long long)x) - 1); return q < n ? q : n; }
    for (w++; w < kATWords && (w << 6) < n; w++) {
        x = bit ? ~bm[w] : bm[w];
        if (x) { const int q = (w << 6) + (__ffsll((unsigned long long)x) - 1); return q < n ? q : n; }
    }
    return n;
}

// returns the trimmed length (0 = nothing acceptable); trim5 / trim3 = bases cut from the start / end of the read as given
template <int ATW>
__device__ int adaptive_trim_dev(const uint64_t *__restrict__ rdw, const uint64_t *__restrict__ tgt, uint64_t t, int len, int min_trim, int max_mm,
                                 int min_flank, int &trim_mm, int &trim5, int &trim3)
{
    constexpr int kATWords = ATW;
    trim_mm = 0; trim5 = 0; trim3 = 0;
    if (len < 25 || len > 64 * kATWords || min_trim < 15 || min_trim > len || max_mm > 15 || min_flank > 10) return 0;
    if (min_flank == 0) min_flank = 1;
    uint64_t bm[kATWords];
#pragma unroll
    for (int w = 0; w < kATWords; w++) bm[w] = 0;
    for (int i = 0; i < len; i += 16) {
        const int nv = len - i < 16 ? len - i : 16;
        const uint64_t x = (nib16(rdw, i) ^ nib16(tgt, t + i)) & top_mask(nv);
        const uint64_t f = (x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x1111111111111111ULL;
        bm[i >> 6] |= (uint64_t)flags_to_bits16(f) << (i & 63);            // bit k of the 16 = base i + k mismatches
    }
    // pass 1: is there an exact run of >= 8; first / last run that may start a stretch, last run that may end one
    bool have8 = false;
    int first_start = -1, last_start = -1, last_end = -1, first_end = -1;
    for (int p = 0; p < len;) {
        const int q = at_run_end<ATW>(bm, p, len), rl = q - p;
        const bool mm = ((bm[p >> 6] >> (p & 63)) & 1) != 0;
        if (!mm) {
            if (rl >= 8) have8 = true;
            if (rl >= min_flank) {
                if (p <= len - min_trim) { last_start = p; if (first_start < 0) first_start = p; }
                if (p + rl >= min_trim) { last_end = p; if (first_end < 0) first_end = p; }
            }
        }
        p = q;
    }
    if (!have8 || first_start < 0 || first_end < 0) return 0;
    const double lim = (max_mm + 1.0) / 100.0;
    int best_len = 0, best_mm = 0, best_start = 0, best_end = 0;
    for (int sp = first_start; sp <= last_start;) {
        const int sq = at_run_end<ATW>(bm, sp, len);
        const bool smm = ((bm[sp >> 6] >> (sp & 63)) & 1) != 0;
        const bool can_start = !smm && (sq - sp) >= min_flank && sp <= len - min_trim;
        if (can_start) {
            int cur_len = 0, cur_mm = 0;
            for (int p = sp; p < len && p <= last_end;) {
                const int q = at_run_end<ATW>(bm, p, len), rl = q - p;
                const bool mm = ((bm[p >> 6] >> (p & 63)) & 1) != 0;
                const bool can_end = !mm && rl >= min_flank && p + rl >= min_trim;
                cur_len += rl;
                p = q;
                if (mm) {
                    if (max_mm == 0) break;
                    cur_mm += rl;
                    if (lim <= (double)cur_mm / (double)(len - sp)) break;
                } else if (best_len == 0) {
                    best_start = sp; best_end = len - (sp + cur_len); best_len = cur_len; best_mm = 0;
                    continue;
                }
                if (cur_len < min_trim || !can_end) continue;
                if (lim <= (double)cur_mm / (double)cur_len) continue;
                if (best_len < cur_len || (best_len == cur_len && (best_mm == 0 || cur_mm < best_mm))) {
                    best_start = sp; best_end = len - (sp + cur_len); best_len = cur_len; best_mm = cur_mm;
                }
            }
        }
        sp = sq;
    }
    if (best_len < min_trim) return 0;
    trim_mm = best_mm; trim5 = best_start; trim3 = best_end;
    return best_len;
}

// AdaptiveTrim(full length) acceptance of the read (packed words rdw) against the target at t
__device__ __forceinline__ bool pe_window_ok(const uint64_t *__restrict__ rdw, int len, const uint64_t *__restrict__ tgt, uint64_t t,
                                             int max_mm, int &mm_out)
{
    int mm = 0, run = 0;
    bool have8 = false, first3 = false;
    for (int i = 0; i < len; i += 16) {
        int nv = len - i < 16 ? len - i : 16;
        uint64_t x = (nib16(rdw, i) ^ nib16(tgt, t + i)) & top_mask(nv);
        uint64_t f = (x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x1111111111111111ULL;
        uint32_t bits = flags_to_bits16(f);                         // bit k = base i+k mismatches
        uint32_t valid = nv >= 16 ? 0xFFFFu : ((1u << nv) - 1);
        uint32_t g = ~bits & valid;                                 // bit k = base matches
        mm += __popc(bits);
        if (i == 0) first3 = (g & 7u) == 7u;
        // runs of >= 8 matches: inside the word, or continuing the run carried from previous words
        uint32_t y = g & (g >> 1);
        y &= y >> 2;
        y &= y >> 4;
        int lead = __ffs((int)(~g & 0x1FFFFu)) - 1;                 // matches at the start of this word (0..16)
        if (lead > nv) lead = nv;
        if (y != 0 || run + lead >= 8) have8 = true;
        if (g == valid) run += nv;
        else run = nv - (32 - __clz((int)(~g & valid)));            // matches after the last mismatch of this word
    }
    mm_out = mm;
    if (len < 25 || len > 2048 || max_mm > 15) return false;         // AdaptiveTrim parameter validation -> eBSFerrParams
    if (!have8 || !first3 || run < 3) return false;
    if (mm > 0 && max_mm == 0) return false;
    if ((max_mm + 1.0) / 100.0 <= (double)mm / (double)len) return false;
    return true;
}

// One candidate window of AlignPairedRead.  ATW == 0: the partner must fit whole (MinChimericLen == 0, MinPutLen = ReadLen); otherwise
// AdaptiveTrim may cut its ends down to min_put bases (SfxArrayV2.cpp:8327-8330,8400-8470).  The reference raises MinPutLen to the length of
// every placement it takes and hands that to the next AdaptiveTrim call; a call with the initial MinPutLen returns the same stretch whenever
// that stretch is at least as long as the raised limit and nothing acceptable otherwise (the limit only removes shorter candidates from
// AdaptiveTrim's scan), so the outcome of the scan is the first window with the longest stretch and, among those, the fewest mismatches.
// key: smaller = better; ~0 = not a candidate.  Bits 52.. = 4095 - trimmed length, bits 40..51 = mismatches, low 40 bits = scan order.
template <int ATW>
__device__ __forceinline__ unsigned long long pe_window_key(const uint64_t *__restrict__ rdw, int len, const uint64_t *__restrict__ tgt, uint64_t t,
                                                            int max_mm, int min_put, unsigned long long order, int &t5, int &t3)
{
    t5 = 0; t3 = 0;
    if constexpr (ATW == 0) {
        int mm;
        if (!(pe_window_ok(rdw, len, tgt, t, max_mm, mm) && mm <= max_mm)) return ~0ULL;
        return ((unsigned long long)(4095 - len) << 52) | ((unsigned long long)mm << 40) | order;
    } else {
        int mm;
        const int r = adaptive_trim_dev<ATW>(rdw, tgt, t, len, min_put, max_mm, 3, mm, t5, t3);
        if (r < min_put || r == 0 || (r == min_put && mm > max_mm)) return ~0ULL;
        return ((unsigned long long)(4095 - r) << 52) | ((unsigned long long)mm << 40) | order;
    }
}

}  // namespace bk
