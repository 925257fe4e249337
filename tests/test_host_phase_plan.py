"""What the host decides about a chunk before it launches the phase loop (CPU only): biokanga_amd/csrc/bk_phase_plan.h as it stands under
tests/cpp/phase_plan_host.cpp, with the stand-in for <hip/hip_runtime.h> the plan table's test uses.  The chunk's bounds against direct
calls of plan_geo_direct, the window family against the ladder in words, sort_prefix against the two rules it replaced."""
import os
import subprocess

import helpers
from test_host_devlogic import CSRC
from test_host_plan_table import HIP_SHIM


def test_phase_plan_on_the_host(tmp_path):
    d = tmp_path / "twin"
    (d / "hip").mkdir(parents=True)
    (d / "hip" / "hip_runtime.h").write_text(HIP_SHIM)
    exe = str(d / "phase_plan_host")
    subprocess.check_call(helpers.cxx() + ["-I" + str(d), "-I" + CSRC, "-o", exe, os.path.join(helpers.ROOT, "tests", "cpp", "phase_plan_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
