// bk_wave_form.h - which form of the wave kernel a batch gets: the rule of launch_wave (bk_wave.hip) as plain functions of the batch's
// shortest and longest read and of the index's tables.  Nothing of HIP here: the rule is checked on the CPU (tests/test_host_wave_form.py).
#pragma once
#include <cstdint>

namespace bk {

// the word launch_min_len (bk_prep.hip) and the stream's k_extent keep - the maximum of the lengths' complements over a zeroed word - as
// the shortest read; 0: no read was seen
inline uint32_t min_len_of(uint32_t word) { return word ? ~word : 0u; }

// the batch's uniform dword count: (len + 15) >> 4 of every read when the shortest and the longest agree in it, else 0.
// min_len 0 means "not known" (a call that only enqueues; an empty batch) and gives 0.
inline int uniform_dwords(uint32_t min_len, uint32_t max_len)
{
    if (min_len == 0 || min_len > max_len) return 0;
    const uint32_t d0 = (min_len + 15) >> 4, d1 = (max_len + 15) >> 4;
    return d0 == d1 ? (int)d0 : 0;
}

// the length-specialised form k_wave<8, .., ND> exists for the 8-word window-array form without hash set (4-byte suffix array with its
// inverse, window array of three-word entries in place, 2-bit read rows) and ND = 1 .. 8; every other form is launched with ND = 0.
// nw: words of the kernel family (8, 16, ..); wide: 5-byte suffix array; hash: no inverse suffix array; sw: the window array serves this family
inline int wave_form_nd(int dwords, int nw, bool wide, bool hash, bool sw)
{
    if (nw > 8 || wide || hash || !sw) return 0;
    return dwords >= 1 && dwords <= 8 ? dwords : 0;
}
inline int wave_len_nd(uint32_t min_len, uint32_t max_len, int nw, bool wide, bool hash, bool sw)
{
    return wave_form_nd(uniform_dwords(min_len, max_len), nw, wide, hash, sw);
}

}  // namespace bk
