"""The device AdaptiveTrim and the paired-end window check on the host (CPU only): bk_dev_trim.h as it stands - adaptive_trim_dev<8|32>,
pe_window_ok, pe_window_key<0|8|32> - under tests/cpp/dev_trim_host.cpp against the CPU oracle's ora_adaptive_trim, with nib16, top_mask
and flags_to_bits16 taken from bk_dev_util.h as they stand (no copy kept here) and the intrinsics supplied as host functions.  The program
holds the case generator that tests/test_gpu_dev_trim.py uses as well (trim_twin_exe builds it, `dump` writes the cases)."""
import os
import subprocess

import helpers
from test_host_devlogic import CSRC, _between

TRIM_SHIM = r'''// stands in for bk_dev_util.h when bk_dev_trim.h is compiled for the host
#pragma once
#include <cstdint>
#define __device__
#define __forceinline__ inline
#define __restrict__
static inline uint64_t __brevll(uint64_t v) { uint64_t r = 0; for (int i = 0; i < 64; i++) if (v >> i & 1) r |= 1ULL << (63 - i); return r; }
static inline int __ffsll(unsigned long long v) { return __builtin_ffsll((long long)v); }
static inline int __ffs(int v) { return __builtin_ffs(v); }
static inline int __clz(int v) { return v == 0 ? 32 : __builtin_clz((unsigned)v); }
static inline int __popc(unsigned v) { return __builtin_popcount(v); }
namespace bk {
%s
}  // namespace bk
'''


def util_helpers_text():
    """nib16, top_mask and flags_to_bits16 as they stand in bk_dev_util.h"""
    text = open(os.path.join(CSRC, "bk_dev_util.h")).read()
    return "\n".join([_between(text, "__device__ __forceinline__ uint64_t nib16(", "// 16 bases at 2 bit/base"),
                      _between(text, "__device__ __forceinline__ uint32_t flags_to_bits16(", "__device__ __forceinline__ uint64_t ktab_get(")])


def trim_twin_exe(tmp_path, header_text=None):
    """bk_dev_trim.h (the text given, or the file as it stands; unchanged) beside the shims, under tests/cpp/dev_trim_host.cpp, linked with
    oracle/bk_oracle.c compiled as C -> the program"""
    d = tmp_path / "twin"
    d.mkdir()
    if header_text is None:
        header_text = open(os.path.join(CSRC, "bk_dev_trim.h")).read()
    assert "adaptive_trim_dev(" in header_text and "pe_window_ok(" in header_text and "pe_window_key(" in header_text
    (d / "bk_dev_trim.h").write_text(header_text)
    (d / "bk_dev_util.h").write_text(TRIM_SHIM % util_helpers_text())
    exe, obj = str(d / "dev_trim_host"), str(d / "bk_oracle.o")
    cxx = helpers.cxx()
    cflags = [f for f in cxx[1:] if not f.startswith("-std=")]
    subprocess.check_call(["gcc"] + cflags + ["-pthread", "-c", "-o", obj, os.path.join(helpers.ORACLE_DIR, "bk_oracle.c")])
    subprocess.check_call(cxx + ["-pthread", "-I" + str(d), "-I" + helpers.ORACLE_DIR, "-o", exe, os.path.join(helpers.ROOT, "tests", "cpp", "dev_trim_host.cpp"), obj])
    return exe


def test_adaptive_trim_and_pe_window_on_the_host_against_the_oracle(tmp_path):
    """400 000 generated cases and the scan claim of pe_window_key (the smallest key is the window AlignPairedRead's loop ends with); the
    program also checks the conditions on its case set: each of zero / trimmed / full at least a tenth, every refusal, every family"""
    out = subprocess.run([trim_twin_exe(tmp_path)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
