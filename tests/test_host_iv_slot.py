"""Where the interval record of (read, strand, core) lies, by position in the active list and by read number, and the way back (CPU only):
biokanga_amd/csrc/bk_iv_slot.h as it stands under tests/cpp/iv_slot_host.cpp.  Slot function and decode are inverse over batches of 1,
63, 64, 65, 257 and 1500 reads, one and two strand passes and 1 .. 16 cores per strand; no two records share a slot."""
import os
import subprocess

import helpers
from test_host_devlogic import CSRC


def test_slot_and_decode_are_inverse(tmp_path):
    exe = str(tmp_path / "iv_slot_host")
    subprocess.check_call(helpers.cxx() + ["-I" + CSRC, "-o", exe, os.path.join(helpers.ROOT, "tests", "cpp", "iv_slot_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
