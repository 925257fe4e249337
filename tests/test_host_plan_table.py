"""The plan table and the item decoding of the search passes on the host (CPU only): biokanga_amd/csrc/bk_plan_table.h and bk_device.h as
they stand under tests/cpp/plan_table_host.cpp, with a stand-in for <hip/hip_runtime.h> (the qualifiers as nothing, uint2 / uint4 as plain
structs).  The table the host builds against direct calls of make_plan, phase_params and core_offsets for every length 0..2000 and every
phase over the parameter sweep; item_decode and slot_decode against plain / and %."""
import os
import subprocess

import helpers
from test_host_devlogic import CSRC

HIP_SHIM = r'''// stands in for <hip/hip_runtime.h> when the device headers are compiled for the host
#pragma once
#include <cstddef>
#include <cstdint>
#define __host__
#define __device__
#define __forceinline__ inline
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
'''


def plan_twin_exe(tmp_path):
    d = tmp_path / "twin"
    (d / "hip").mkdir(parents=True)
    (d / "hip" / "hip_runtime.h").write_text(HIP_SHIM)
    exe = str(d / "plan_table_host")
    subprocess.check_call(helpers.cxx() + ["-I" + str(d), "-I" + CSRC, "-o", exe, os.path.join(helpers.ROOT, "tests", "cpp", "plan_table_host.cpp")])
    return exe


def test_plan_table_and_item_decoding_on_the_host(tmp_path):
    out = subprocess.run([plan_twin_exe(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
