"""The grouping table of the request passes (biokanga_amd/csrc/bk_dev_group.h) on the host (CPU only): the header as it stands, compiled
beside a stand-in for bk_dev_util.h - one thread, the atomics as plain accesses that count their steps - under tests/cpp/dev_group_host.cpp,
which checks claim, join, find-again, the full table and the clear kernel against std::map for both slot layouts.  The 64-bit mix is
checked here against its statement in Python.  It is a stand-alone program: BK_TEST_CXXFLAGS="-O1 -fsanitize=address,undefined" builds it
with the sanitizers."""
import os
import subprocess

import helpers

CSRC = os.path.join(helpers.ROOT, "biokanga_amd", "csrc")

GROUP_SHIM = r'''// stands in for bk_dev_util.h when bk_dev_group.h is compiled for the host: one thread, the atomics as plain accesses that count their steps
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define __HIP_MEMORY_SCOPE_AGENT 4
static unsigned long long g_steps = 0, g_loads = 0;
constexpr unsigned long long kMaxSteps = 1000000;          // between two resets by the harness: no probe sequence of a sound helper is that long
static inline void twin_step() { if (++g_steps > kMaxSteps) { printf("FAIL: a probe loop does not end\n"); exit(2); } }
template <typename T> static inline T twin_load(const T *p) { twin_step(); g_loads++; return *p; }
#define __hip_atomic_load(p, order, scope) twin_load(p)
template <typename T, typename V> static inline T atomicCAS(T *p, T expect, V v) { twin_step(); const T old = *p; if (old == expect) *p = (T)v; return old; }
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct twin_dim { unsigned x; };
static const twin_dim blockIdx{0}, threadIdx{0}, blockDim{1}, gridDim{1};       // a grid of one thread
'''

MASK = (1 << 64) - 1


def group_hash(a, b):
    """the mix in words: a times the golden-ratio constant; b is folded in boost's hash_combine manner with a second odd constant; then the
    finalizer of MurmurHash3 (two xor-shift-multiply rounds and a last xor-shift by 33)"""
    h = (a * 0x9E3779B97F4A7C15) & MASK
    h ^= (b + 0xD6E8FEB86659FD93 + (h << 6) + (h >> 2)) & MASK
    for mul in (0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53):
        h ^= h >> 33
        h = (h * mul) & MASK
    return h ^ (h >> 33)


def test_grouping_table_on_the_host_against_std_map(tmp_path):
    """group_claim / group_find / k_group_clear / group_hash of bk_dev_group.h as they stand, single-threaded: random keys with heavy
    repetition and distinct keys in tables of 2n and of exactly n slots, every key hashed to one slot, find-again of every request, a key
    never inserted, a table one slot too small (no slot after exactly `slots` looks), owner at offset 0 and at offset 8, the clear value"""
    d = tmp_path / "twin"
    d.mkdir()
    (d / "bk_dev_group.h").write_text(open(os.path.join(CSRC, "bk_dev_group.h")).read())
    (d / "bk_dev_util.h").write_text(GROUP_SHIM)
    exe = str(d / "dev_group_host")
    subprocess.check_call(helpers.cxx() + ["-I" + str(d), "-o", exe, os.path.join(helpers.ROOT, "tests", "cpp", "dev_group_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    hashes = [tuple(int(x) for x in ln.split()[1:]) for ln in out.stdout.splitlines() if ln.startswith("hash ")]
    assert len(hashes) == 6
    for a, b, got in hashes:
        assert got == group_hash(a, b), (a, b, got)
