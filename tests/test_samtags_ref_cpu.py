"""--sam-tags without a GPU: the literal-walk reference of tests/samtags_ref.py against hand-worked lines and over the aligned records
of golden files, and the option checks of `biokanga align --sam-tags` that end before anything touches a device."""
import os
import subprocess

import pytest

import helpers
import samtags_ref as sr

#              0         1         2         3
#              0123456789012345678901234567890123456789
G = sr.Genome(seqs={1: ("chrA", "ACGTACGTACGGTTCAGNNAACCGGTTACGATCGATCGAAC"), 2: ("chrB", "TTTTTCCCCC")})


def line(pos, cigar, seq, flag=0, rname="chrA"):
    return f"r\t{flag}\t{rname}\t{pos}\t255\t{cigar}\t*\t0\t0\t{seq}\t*"


@pytest.mark.parametrize("pos,cigar,seq,exp", [
    (1, "10M", "ACGTACGTAC", (0, "10")),                       # all matching
    (1, "10M", "CCGTACGTAC", (1, "0A9")),                      # first base
    (1, "10M", "ACGTACGTAG", (1, "9C0")),                      # last base
    (1, "10M", "ACGGTCGTAC", (2, "3T0A5")),                    # adjacent mismatches: a 0 between them
    (1, "5M2D5M", "ACGTATACGG", (2, "5^CG5")),                 # deletion: ^ and the target's letters; NM counts them
    (1, "5M2D5M", "ACGTTTACGG", (3, "4A0^CG5")),               # a mismatch right in front of a deletion
    (1, "5M2I5M", "ACGTAGGCGTAC", (2, "10")),                  # insertion: NM 2, the run goes on across it
    (1, "5M20N5M", "ACGTATTACG", (0, "10")),                   # N: nothing written, the run goes on
    (3, "2S6M2S", "TTGTACGTTT", (0, "6")),                     # clips consume SEQ only
    (1, "2S4M2S2D4M", "TTACGTTTGTAC", (2, "4^AC4")),           # the shape the writers make: the second M run follows the 3' clip
    (17, "4M", "GNNA", (2, "1N0N1")),                          # a read N over a target N is a mismatch (the target's letter is N)
    (17, "4M", "GAAA", (2, "1N0N1")),
    (15, "3M", "NAG", (1, "0C2")),                             # a read N over a base
    (32, "10M", "TCGATCGAAC", (0, "10")),                      # ends at the last base of its sequence
    (1, "10M", "TTTTTCCCCC", (0, "10")),
])
def test_hand_worked_lines(pos, cigar, seq, exp):
    rname = "chrB" if seq == "TTTTTCCCCC" else "chrA"
    assert sr.ref_tags(line(pos, cigar, seq, rname=rname), G) == exp


def test_adjacent_mismatch_example_of_the_issue():
    """3A0C5: the letters are the TARGET's"""
    g = sr.Genome(seqs={1: ("c", "GGGACGGGGG")})
    assert sr.ref_tags(line(1, "10M", "GGGTTGGGGG", rname="c"), g) == (2, "3A0C5")
    g = sr.Genome(seqs={1: ("c", "GGGGGACGGGGG")})
    assert sr.ref_tags(line(1, "5M2D5M", "GGGGGGGGGG", rname="c"), g) == (2, "5^AC5")
    assert sr.ref_tags(line(1, "5M100N5M", "GGGGGGGGGG", rname="c"), sr.Genome(seqs={1: ("c", "G" * 200)})) == (0, "10")


@pytest.mark.parametrize("pos,cigar,seq", [
    (1, "0M", ""), (1, "10M0S", "ACGTACGTAC"), (1, "5M-2D5M", "ACGTATACGG"),       # a number <= 0
    (1, "9M", "ACGTACGTAC"), (1, "11M", "ACGTACGTAC"), (1, "5M2I5M", "ACGTACGTAC"),  # does not consume exactly SEQ
    (35, "10M", "ACGTACGTAC"), (30, "5M10D5M", "ACGTACGTAC"), (30, "5M10N5M", "ACGTACGTAC"),   # leaves its sequence
    (0, "10M", "ACGTACGTAC"), (1, "10X", "ACGTACGTAC"), (1, "M", "A"),
])
def test_malformed_walks_get_no_tags(pos, cigar, seq):
    assert sr.ref_tags(line(pos, cigar, seq), G) is None


def test_unaligned_and_unknown_sequence():
    assert sr.ref_tags(line(0, "10M", "ACGTACGTAC", flag=4, rname="*"), G) is None
    assert sr.ref_tags(line(1, "10M", "ACGTACGTAC", rname="chrZ"), G) is None


def test_requests_and_tag_splitting():
    r, codes = sr.request(line(5, "2S4M2S3D4M", "TTACGTTTCGTA", flag=16), G, 77)
    assert (int(r["read_ofs"]), int(r["chrom_id"]), int(r["pos"]), int(r["read_len"]), chr(r["strand"])) == (77, 1, 4, 12, "-")
    assert (int(r["c5"]), int(r["m"]), int(r["c3"]), chr(r["gop"]), int(r["gap"]), int(r["m2"])) == (2, 4, 2, "D", 3, 4)
    assert "".join(sr.LETTERS[c] for c in codes) == sr.revcomp("TTACGTTTCGTA")
    assert sr.request(line(1, "4M2I2D4M", "ACGTACGTAC"), G, 0) is None
    bare = line(1, "10M", "ACGTACGTAC")
    assert sr.split_tags(bare + "\tNM:i:3\tMD:Z:1A2^CC4") == (bare, 3, "1A2^CC4")
    assert sr.split_tags(bare) == (bare, None, None)
    un = "r\t4\t*\t0\t255\t10M\t*\t0\t0\tACGTACGTAC\t*\t\tYU:Z:NL"
    assert sr.split_tags(un.encode()) == (un.encode(), None, None)


# (fixture, golden SAM, the run's -s): the runs the feature's tests demand tags of on EVERY aligned line
GOLDENS = [("basic", "s3.m6", 3), ("indel", "a10.m6", 3), ("indel", "a10x4.m6", 3), ("splice", "A5000.m6", 3), ("splice", "A5000a5.m6", 3),
           ("chimeric", "c50.m6", 3), ("multi", "r5R5x4.m6", 3)]


@pytest.mark.parametrize("fixture,tag,subs", GOLDENS, ids=[f"{g[0]}-{g[1]}" for g in GOLDENS])
def test_every_aligned_golden_record_walks(fixture, tag, subs):
    """no aligned record of these files is malformed, every one has the writers' shape, and a one-segment record has at most the
    substitutions its run allowed: -s is a rate per 100 bp of read, so at most ceil(s * aligned bases / 100) ... never fewer than a
    read of up to 100 bases is allowed, s"""
    g = sr.Genome(os.path.join(helpers.GOLDEN, fixture, "genome.sfx.gz"))
    _, recs = helpers.parse_sam(os.path.join(helpers.GOLDEN, fixture, tag + ".sam.gz"))
    n = 0
    for r in recs:
        if r["flag"] & 4:
            continue
        t = sr.ref_tags(r, g)
        assert t is not None, r["raw"]
        assert sr.request(r, g, 0) is not None, r["raw"]
        if not any(op in r["cigar"] for op in "NID"):
            assert t[0] <= max(subs, (subs * len(r["seq"]) + 99) // 100), (t, r["raw"])
        n += 1
    assert n > 100


BIN = os.path.join(helpers.ROOT, "biokanga_amd", "bin", "biokanga")


@pytest.mark.parametrize("args,text", [
    (["--sam-tags", "XX"], "'--sam-tags XX' must be a list of NM and MD"),
    (["--sam-tags", "NM,XX"], "'--sam-tags NM,XX' must be a list of NM and MD"),
    (["--sam-tags", ""], "'--sam-tags ' must be a list of NM and MD"),
    (["--sam-tags", "NM", "-M0"], "'--sam-tags NM' are only available with SAM / BAM output formats"),
    (["--sam-tags=NM,MD", "-M4"], "'--sam-tags NM,MD' are only available with SAM / BAM output formats"),
])
def test_cli_refuses_before_any_device_work(args, text):
    r = subprocess.run([BIN, "align", "-i", "none.fa", "-I", "none.sfx", "-o", "none.sam"] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 1, r.stdout
    assert text in r.stdout, r.stdout
    assert "Exit code: 1" in r.stdout
