"""`biokanga align --coverage`: the refusals that end the run before anything touches a device - CPU only, the binary run the way
tests/test_cli_options_cpu.py runs it."""
import os
import subprocess

import pytest

import helpers

BIN = os.path.join(helpers.ROOT, "biokanga_amd", "bin", "biokanga")
pytestmark = pytest.mark.skipif(not os.path.exists(BIN), reason="the command line has not been built (python -c 'import __graft_entry__ as g; g.build()')")


def run(args):
    r = subprocess.run([BIN, "align", "-i", "none.fa", "-I", "none.sfx", "-o", "none.sam"] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    return r.returncode, r.stdout


@pytest.mark.parametrize("args,text", [
    (["--coverage", ""], "Error: coverage file '--coverage' needs a file name"),
    (["--coverage="], "Error: coverage file '--coverage' needs a file name"),
    (["--coverage", "none.sam"], "Error: coverage file '--coverage none.sam' is the output file '-o' itself"),
    (["-M0", "--coverage=none.sam"], "Error: coverage file '--coverage none.sam' is the output file '-o' itself"),
])
def test_coverage_refusals_before_any_device_work(args, text):
    rc, out = run(args)
    assert rc == 1, out
    assert text in out, out
    assert "Exit code: 1" in out
    assert "Loading suffix array file" not in out
