"""Which form of the wave kernel a batch gets (CPU only): biokanga_amd/csrc/bk_wave_form.h as it stands under tests/cpp/wave_form_host.cpp.
The rule as a plain function of (shortest read, longest read, form): the length-specialised dword count for the 8-word window-array form
without hash set when every read has the same number of 16-base dwords, 0 otherwise - every pair of lengths up to 300 against the rule
written out, the boundaries 96 / 97 and 112 / 113, a minimum that is not known, a maximum beyond 128."""
import os
import subprocess

import helpers
from test_host_devlogic import CSRC


def test_wave_form_dispatch_on_the_host(tmp_path):
    exe = str(tmp_path / "wave_form_host")
    subprocess.check_call(helpers.cxx() + ["-I" + CSRC, "-o", exe, os.path.join(helpers.ROOT, "tests", "cpp", "wave_form_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
