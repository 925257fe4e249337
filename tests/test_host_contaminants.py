"""`biokanga align -H`, the parts that need no GPU: the contaminants file's parser (host/contaminants.cpp) against the files the reference
accepted for tests/golden/contam and against what it refuses, and the Python statement of the rule (contam_rule.py) - which the GPU tests
hold the device matcher to - against every read of every golden case: the reference's SAM records hold exactly the reads the rule keeps,
cut where the rule cuts them, and its four count lines are the rule's counts."""
import gzip
import os
import subprocess

import pytest

import contam_rule as cr
import helpers


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("c") / "contam_harness")
    host = os.path.join(helpers.ROOT, "biokanga_amd", "csrc", "host")
    src = [os.path.join(helpers.ROOT, "tests", "cpp", "contam_harness.cpp"), os.path.join(host, "contaminants.cpp"), os.path.join(host, "fasta.cpp"),
           os.path.join(host, "fast_inflate.cpp")]
    subprocess.check_call(helpers.cxx() + ["-pthread", "-o", exe] + src + ["-lz"])
    return exe


def parsed(harness, path):
    r = subprocess.run([harness, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if not l.startswith("[")]
    if lines and lines[0].startswith("rc "):
        return int(lines[0].split()[1]), r.stdout
    return [(int(l.split()[1]), l.split()[4]) for l in lines], r.stdout


@pytest.mark.parametrize("name", ["ad13.fa", "names.fa", "rc57.fa", "nn.fa", "pe.fa", "many.fa"])
def test_parser_makes_the_entries_of_the_files_the_reference_accepted(harness, name):
    path = os.path.join(cr.CONTAM, name)
    got, _ = parsed(harness, path)
    assert got == cr.entries(path) and len(got) > 0


def test_parser_name_codes(harness, tmp_path):
    """the backwards scan of the name: codes behind '@', default codes without one, digits that are part of the name"""
    p = str(tmp_path / "c.fa")
    open(p, "w").write(">a@13 words\nACGTTGCA\n>b12\nACGGTTCA\n>c@19\nAAGGTTCA\n>88\nAAGGTACA\n>d@\nAGGGTACA\n>e@57\nAGGNTACAC\n>  f@8 x\nacgtaacc\ntt\n")
    got, _ = parsed(harness, p)
    dflt = lambda s: [(1, s), (2, s), (1, cr.revcomp(s)), (2, cr.revcomp(s))]
    assert got == [(1, "ACGTTGCA"), (3, "ACGTTGCA")] + dflt("ACGGTTCA") + dflt("AAGGTTCA") + dflt("AAGGTACA") + dflt("AGGGTACA") + \
        [(1, "GTGTANCCT"), (3, "GTGTANCCT"), (4, "AAGGTTACGT")]
    assert got == cr.entries(p)


@pytest.mark.parametrize("text,what", [
    (">v&12\nACGTACGTACGTACGTACGTACGTACGT\n", "vector contaminant"),                 # '&': whole-read containment, not built
    (">a@1\nACG\n", "outside of accepted length range"),
    (">a@1\n" + "ACGT" * 50 + "A\n", "outside of accepted length range"),
    (">@13\nACGTACGT\n", "Parameter errors"),                                          # nothing but codes: no name left
    (">a@1\nACGTACGT\n>b@1\nACGTACGT\n", "duplicated sequence"),
    (">a@1\nACGTACGT\n>A@1\nACGTACGA\n", "duplicated with different sequences"),
    (">pal\nACGT\n", "duplicated sequence"),                                           # default codes: its reverse complement is itself
    ("".join(f">s{k}@1234\n{''.join('ACGT'[(k >> (2 * j)) & 3] for j in range(12))}\n" for k in range(401)), "Too many flank contaminants"),
])
def test_parser_refuses_what_the_reference_refuses(harness, tmp_path, text, what):
    p = str(tmp_path / "bad.fa")
    open(p, "w").write(text)
    got, log = parsed(harness, p)
    assert isinstance(got, int) and got < 0 and what in log, log
    with pytest.raises(ValueError):
        cr.entries(p)


def sam_records(path):
    out = []
    for line in gzip.open(path, "rt"):
        if line.startswith("@"):
            continue
        f = line.rstrip("\n").split("\t")
        flag, seq, qual = int(f[1]), f[9], f[10]
        if flag & 16:
            seq, qual = cr.revcomp(seq), qual[::-1]
        out.append((f[0], 1 if flag & 0x80 else 0, seq, qual))
    return out


@pytest.mark.parametrize("tag", sorted(cr.cases()))
def test_rule_predicts_every_read_of_the_reference_run(tag):
    """every read of the case: kept or dropped as the reference did, the kept ones cut as the reference cut them; the count lines too"""
    case = cr.cases()[tag]
    kept, counts = cr.expected_store(case)
    recs = sam_records(os.path.join(cr.CONTAM, tag + ".m6.sam.gz"))
    assert len(recs) == len(kept)
    exp = sorted((n, e, cr.norm(s), None if q is None else len(q)) for n, s, q, e in kept)
    got = sorted((n, e, cr.norm(s), None if q == "*" else len(q)) for n, e, s, q in recs)
    assert got == exp
    lines = open(os.path.join(cr.CONTAM, tag + ".contam.txt")).read().splitlines()
    want = [f"Load: total of {counts[0]} sequences PE1 sequences were 5' contaminate trimmed",
            f"Load: total of {counts[1]} sequences PE1 sequences were 3' contaminate trimmed"]
    if "mates" in case:
        want += [f"Load: total of {counts[2]} sequences PE1 sequences were 5' contaminant trimmed",
                 f"Load: total of {counts[3]} sequences PE1 sequences were 3' contaminant trimmed"]
    assert lines == want
