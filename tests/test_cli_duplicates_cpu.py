"""`biokanga align --mark-duplicates`: the refusals that end the run before anything touches a device - CPU only, the binary run the way
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
    (["-M0", "--mark-duplicates"], "Error: duplicate marking '--mark-duplicates' is only available with SAM / BAM output formats '-M5' and '-M6'"),
    (["--mark-duplicates", "-M4"], "Error: duplicate marking '--mark-duplicates' is only available with SAM / BAM output formats '-M5' and '-M6'"),
    (["--mark-duplicates", "-r5", "-R10"], "Error: duplicate marking '--mark-duplicates' is not available when reporting all multiloci alignments '-r5'"),
    (["--mark-duplicates=x"], "option --mark-duplicates takes no value"),
])
def test_duplicate_marking_refusals_before_any_device_work(args, text):
    rc, out = run(args)
    assert rc == 1, out
    assert text in out, out
    assert "unknown option" not in out
    assert "Loading suffix array file" not in out


@pytest.mark.parametrize("args", [["--mark-duplicates"], ["--mark-duplicates", "-M6", "-s3"], ["-U3", "-u", "none2.fa", "--mark-duplicates", "--sam-tags", "NM"]])
def test_the_option_takes_no_value_and_is_accepted(args):
    """the run gets as far as the index that is not there; the option has not eaten the argument behind it"""
    rc, out = run(args)
    assert "unknown option" not in out and "unexpected argument" not in out and "needs a value" not in out, out
    assert "Loading suffix array file" in out, out
