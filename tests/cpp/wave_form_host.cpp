// The wave kernel's dispatch rule (biokanga_amd/csrc/bk_wave_form.h, the file as it stands) on the host: tests/test_host_wave_form.py
// compiles and runs this.
//   - wave_len_nd(min, max, form) against the rule written out: ND = (len + 15) >> 4 when the shortest and the longest read agree in it,
//     it is 1 .. 8 and the form is the 8-word window-array one without hash set; else 0 - for every pair of lengths 0 .. 300 and every form
//   - the boundaries 96 / 97 and 112 / 113, a minimum of 0 (not known), a maximum above 128
//   - min_len_of: the word launch_min_len keeps, a zeroed word included
#include <cstdint>
#include <cstdio>

#include "bk_wave_form.h"

using namespace bk;

static int fail(const char *what, long a = 0, long b = 0) { printf("FAIL: %s (%ld, %ld)\n", what, a, b); return 1; }

int main()
{
    const bool F = false, T = true;
    // every pair of lengths, every form
    for (uint32_t mn = 0; mn <= 300; mn++)
        for (uint32_t mx = 0; mx <= 300; mx++)
            for (int form = 0; form < 16; form++) {
                const int nw = (form & 1) ? 16 : 8;
                const bool wide = form & 2, hash = form & 4, sw = form & 8;
                int exp = 0;
                if (nw == 8 && !wide && !hash && sw && mn >= 1 && mn <= mx && (mn + 15) / 16 == (mx + 15) / 16 && (mx + 15) / 16 <= 8) exp = (int)((mx + 15) / 16);
                if (wave_len_nd(mn, mx, nw, wide, hash, sw) != exp) return fail("wave_len_nd", mn, mx);
                if (exp && (exp < 1 || exp > 8)) return fail("range", mn, mx);
            }
    // the boundaries, by name
    if (wave_len_nd(96, 96, 8, F, F, T) != 6) return fail("96");
    if (wave_len_nd(97, 97, 8, F, F, T) != 7) return fail("97");
    if (wave_len_nd(96, 97, 8, F, F, T) != 0) return fail("96 / 97");
    if (wave_len_nd(97, 112, 8, F, F, T) != 7) return fail("97 .. 112");
    if (wave_len_nd(100, 100, 8, F, F, T) != 7) return fail("100");
    if (wave_len_nd(112, 113, 8, F, F, T) != 0) return fail("112 / 113");
    if (wave_len_nd(113, 128, 8, F, F, T) != 8) return fail("113 .. 128");
    if (wave_len_nd(1, 16, 8, F, F, T) != 1) return fail("1 .. 16");
    if (wave_len_nd(0, 100, 8, F, F, T) != 0) return fail("minimum not known");
    if (wave_len_nd(0, 0, 8, F, F, T) != 0) return fail("empty");
    if (wave_len_nd(129, 129, 8, F, F, T) != 0) return fail("129 in the 8-word family");
    if (wave_len_nd(129, 144, 16, F, F, T) != 0) return fail("the 16-word family");
    if (wave_len_nd(100, 100, 8, T, T, T) != 0 || wave_len_nd(100, 100, 8, F, T, F) != 0 || wave_len_nd(100, 100, 8, F, F, F) != 0) return fail("other forms");
    if (wave_len_nd(101, 100, 8, F, F, T) != 0) return fail("minimum above the maximum");
    if (wave_form_nd(9, 8, F, F, T) != 0 || wave_form_nd(-1, 8, F, F, T) != 0 || wave_form_nd(8, 8, F, F, T) != 8) return fail("wave_form_nd");
    // the word of launch_min_len
    if (min_len_of(0u) != 0u || min_len_of(~100u) != 100u || min_len_of(~0u) != 0u || min_len_of(~1u) != 1u) return fail("min_len_of");
    printf("ok\n");
    return 0;
}
