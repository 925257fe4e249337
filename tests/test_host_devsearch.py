"""The search primitives of bk_dev_util.h and bk_dev_k2.h on the host (CPU only): the two headers and bk_device.h compiled as they stand - no
text cut out, no copy - with tests/cpp/hip_shim standing in for the HIP runtime header, under tests/cpp/dev_search_host.cpp, against plain
references over one-byte-per-base arrays.  All results are integers and must be equal.

(a) nib16, bits64_2, RdRow::nib16 / word16 in both row forms, spread2to4, squeeze2, top_mask, flags_to_bits16; (b) cmp_core (pointer row and
RdRow of either form), cmp_core_from, hamming, hamming_eos against per-base loops; (c) ktab_get, ktab_get_pair, core_range over the four
views of one synthetic table of order 9 (bucket starts above 2^32 in the 64-bit and the packed view) and the index without a table,
sa_get<true> with non-zero high bytes; (d) search_core<false|true> against the CPU oracle's LocateFirstExact / LocateLastExact on the
`repeat` and `basic` golden indexes, k = 0, 4, 8 with tables counted in plain code - the <true> instantiations get a zero sa_hi, which
exercises their code path only: element values above 2^32 are covered by (c); (e) k2_make, kx_make, k2_cmp, k2_nkind, k2_mask,
ktab2_absent, and k2_count_range / k2_bounds on an array of about 1.3 M keys in buckets laid side by side, levels filled by the rule of
k_build_k2_levels - level 5 is reached, levels 6 and 7 need 16 M and 268 M keys and are left out; (f) find_entry, find_entry_lds (1, 2,
128, 129 entries), classify, write_result.

The program holds the case generators that tests/test_gpu_dev_search.py uses as well (`dump`), and checks the conditions on its case
sets itself.  It is a stand-alone program: BK_TEST_CXXFLAGS="-O1 -fsanitize=address,undefined" builds it with the sanitizers."""
import os
import subprocess

import helpers


def search_twin_exe(tmp_path):
    """tests/cpp/dev_search_host.cpp with the device headers as they stand, linked with oracle/bk_oracle.c compiled as C -> the program"""
    d = tmp_path / "search_twin"
    d.mkdir()
    exe, obj = str(d / "dev_search_host"), str(d / "bk_oracle.o")
    cxx = helpers.cxx()
    cflags = [f for f in cxx[1:] if not f.startswith("-std=")]
    subprocess.check_call(["gcc"] + cflags + ["-pthread", "-c", "-o", obj, os.path.join(helpers.ORACLE_DIR, "bk_oracle.c")])
    subprocess.check_call(cxx + ["-pthread", "-I" + os.path.join(helpers.ROOT, "tests", "cpp", "hip_shim"), "-I" + os.path.join(helpers.ROOT, "biokanga_amd", "csrc"),
                                 "-I" + helpers.ORACLE_DIR, "-o", exe, os.path.join(helpers.ROOT, "tests", "cpp", "dev_search_host.cpp"), obj])
    return exe


def twin_indexes(golden_tmp):
    return [os.path.join(golden_tmp[name], "genome.sfx") for name in ("repeat", "basic")]


def test_search_primitives_on_the_host_against_plain_references(tmp_path, golden_tmp):
    """every group at its full counts (2.4 M cases); the program prints `ok`, or the first failing cases - each with the function's name and
    its inputs - and the conditions its case sets miss (each sign of cmp_core and each regime of hamming a fifth of their cases; a tenth of
    the search probes absent, a tenth runs of one, a tenth runs longer than 64; a bucket start at every residue mod 16)"""
    out = subprocess.run([search_twin_exe(tmp_path)] + twin_indexes(golden_tmp), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-6000:] + out.stderr[-3000:]
