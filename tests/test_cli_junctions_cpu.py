"""`biokanga align --junctions <file>` / `--splice-strand`: the refusals that end the run before anything touches a device - CPU only, the
binary run the way tests/test_cli_options_cpu.py runs it."""
import os
import subprocess

import pytest

import helpers

BIN = os.path.join(helpers.ROOT, "biokanga_amd", "bin", "biokanga")
pytestmark = pytest.mark.skipif(not os.path.exists(BIN), reason="the command line has not been built (python -c 'import __graft_entry__ as g; g.build()')")


def run(args, out="none.sam"):
    r = subprocess.run([BIN, "align", "-i", "none.fa", "-I", "none.sfx", "-o", out] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    return r.returncode, r.stdout


@pytest.mark.parametrize("args,out,text", [
    (["-A5000", "--junctions", ""], "none.sam", "Error: junction table '--junctions' needs a file name"),
    (["-A5000", "--junctions="], "none.sam", "Error: junction table '--junctions' needs a file name"),
    (["-A5000", "--junctions", "none.sam"], "none.sam", "Error: junction table '--junctions none.sam' is the output file '-o' itself"),
    (["-A5000", "--junctions", "none.sam.jct"], "none.sam", "Error: junction table '--junctions none.sam.jct' is the junction BED file of '-o' itself"),
    (["-A5000", "--junctions", "none.sam.jct"], "none.sam.gz", "Error: junction table '--junctions none.sam.jct' is the junction BED file of '-o' itself"),
    (["-A5000", "-M0", "--junctions", "none.csv.jct"], "none.csv", "Error: junction table '--junctions none.csv.jct' is the junction BED file of '-o' itself"),
    (["--junctions", "sj.tab"], "none.sam", "Error: junction table '--junctions' needs RNAseq splice junction processing '-A<len>'"),
    (["--junctions", "sj.tab", "-a5"], "none.sam", "Error: junction table '--junctions' needs RNAseq splice junction processing '-A<len>'"),
    (["--splice-strand"], "none.sam", "Error: transcript strand tags '--splice-strand' need RNAseq splice junction processing '-A<len>'"),
    (["-A5000", "-M0", "--splice-strand"], "none.sam", "Error: transcript strand tags '--splice-strand' are only available with SAM / BAM output formats '-M5' and '-M6'"),
    (["--splice-strand", "-M4", "-A5000"], "none.sam", "Error: transcript strand tags '--splice-strand' are only available with SAM / BAM output formats '-M5' and '-M6'"),
    (["-A5000", "--splice-strand=x"], "none.sam", "option --splice-strand takes no value"),
    (["-A5000", "--junctions"], "none.sam", "option --junctions needs a value"),
])
def test_refusals_before_any_device_work(args, out, text):
    rc, log = run(args, out)
    assert rc == 1, log
    assert text in log, log
    assert "unknown option" not in log
    assert "Loading suffix array file" not in log


@pytest.mark.parametrize("args", [["-A5000", "--junctions", "sj.tab"], ["-A5000", "--splice-strand"], ["--splice-strand", "-A5000", "-M6", "-s3"],
                                  ["-A5000", "-M0", "--junctions", "sj.tab"], ["-A500", "--junctions=sj.tab", "--splice-strand", "--sam-tags", "NM"],
                                  ["-A5000", "-r2", "-N", "--junctions", "sj.tab", "--splice-strand"]])
def test_the_options_are_accepted(args):
    """the run gets as far as the index that is not there; --splice-strand has not eaten the argument behind it"""
    rc, out = run(args)
    assert "unknown option" not in out and "unexpected argument" not in out and "needs a value" not in out and "takes no value" not in out, out
    assert "Loading suffix array file" in out, out
