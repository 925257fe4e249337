"""The line as written (biokanga_amd/csrc/bk_line.h through bk::RecordSet::line, host/post_filters.h) on the host (CPU only): POS and
the numbers of [c5 S] m M [c3 S] [gap N|I|D m2 M] of made-up records under tests/cpp/line_host.cpp, against the rule as stated here in
words - not a translation of the header:

  * the trims are kept in read orientation; on the target the left one is the 5' clip of a '+' record and the 3' clip of a '-' record.
    POS - 1 is the hit's start plus the 5' clip, m what the trims leave of the hit
  * a read has a second segment when its entry carries the splice flag (4) or the microInDel flag (1); the chimeric flag (8) alone marks
    trims, not a segment.  d is the distance from the end of the hit (untrimmed) to the start of the second segment
  * splice flag: N, which takes d target bases as it is, negative or zero too; else with bit 2: I, which takes no target base and is written
    with what the two segments leave of the read; else D, which takes and is written with |d|
  * with a record -> read table the second segment is the READ's"""
import os
import subprocess

import numpy as np
import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "line_host.cpp")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("h") / "line_host")
    subprocess.check_call(helpers.cxx() + ["-o", exe, SRC])
    return exe


def expected(rec, read, with_trims, with_seg2):
    """rec: (chrom, loci, length, strand, tl, tr, rd); read: (read_len, seg_loci, seg_len, seg_flags) -> the eight numbers of a line"""
    _, loci, length, strand, tl, tr, _ = rec
    read_len, s_loci, s_len, s_flags = read
    if not with_trims:
        tl = tr = 0
    c5, c3 = (tl, tr) if strand == "+" else (tr, tl)
    line = [loci + c5, length - tl - tr, c5, c3]
    if not with_seg2 or not (s_flags & 5):
        return line + [0, 0, 0, 0]
    d = s_loci - (loci + length)
    if s_flags & 4:
        return line + [ord("N"), s_len, d, d]
    if s_flags & 2:
        return line + [ord("I"), s_len, 0, read_len - length - s_len]
    return line + [ord("D"), s_len, abs(d), abs(d)]


def run(exe, tmp_path, recs, reads, with_src, with_trims, with_seg2):
    inp, outp = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(inp, "w") as f:
        f.write(f"{len(recs)} {len(reads)} {int(with_src)} {int(with_trims)} {int(with_seg2)}\n")
        f.writelines(" ".join(str(x) for x in r) + "\n" for r in recs)
        f.writelines(" ".join(str(x) for x in r) + "\n" for r in reads)
    subprocess.check_call([exe, inp, outp])
    got = [[int(x) for x in ln.split()] for ln in open(outp)]
    assert len(got) == len(recs)
    for i, (g, rec) in enumerate(zip(got, recs)):
        want = expected(rec, reads[rec[6] if with_src else i], with_trims, with_seg2)
        assert g == want, (i, rec, reads[rec[6] if with_src else i], g, want)


# second segments by what they make: none, chimeric trims only, N (d > 0, d = 0, d < 0, with the other bits set), I, D (d > 0, d < 0)
SEG_KINDS = [("none", 0, 0), ("chimeric", 8, 40), ("N", 4, 500), ("N d=0", 4, 0), ("N d<0", 4, -30), ("N|2", 6, 77), ("N|1", 5, 9), ("I", 3, 0), ("I far", 3, 12),
             ("D", 1, 6), ("D d<0", 1, -6), ("D|8", 9, 3)]


def test_enumerated_corners(harness, tmp_path):
    """both strands x trims 0 / non-zero at either end x every kind of second segment, one record per read"""
    recs, reads = [], []
    for strand in "+-":
        for tl, tr in ((0, 0), (5, 0), (0, 7), (5, 7)):
            for _, flags, d in SEG_KINDS:
                loci, length = 100000 + 13 * len(recs), 60
                recs.append((1 + len(recs) % 3, loci, length, strand, tl, tr, len(recs)))
                reads.append((101, loci + length + d, 35, flags))
    assert len(recs) == 2 * 4 * len(SEG_KINDS)
    run(harness, tmp_path, recs, reads, False, True, True)


@pytest.mark.parametrize("with_src,with_trims,with_seg2", [(False, True, True), (True, True, True), (False, False, True), (False, True, False), (True, False, False)])
def test_random_records(harness, tmp_path, with_src, with_trims, with_seg2):
    """400 random records; with a record -> read table several records share a read (-r5), without the tables the line is the hit's own"""
    rng = np.random.default_rng(77 + 4 * with_src + 2 * with_trims + with_seg2)
    n = 400
    nreads = 90 if with_src else n
    reads = []
    for _ in range(nreads):
        flags = int(rng.choice([0, 0, 1, 3, 4, 8, 9, 6]))
        reads.append((int(rng.integers(30, 600)), int(rng.integers(0, 1 << 31)), int(rng.integers(1, 300)), flags))
    recs = []
    for i in range(n):
        length = int(rng.integers(1, 65536 if i % 50 == 0 else 400))
        tl = int(rng.integers(0, length)) if rng.random() < 0.5 else 0
        tr = int(rng.integers(0, length - tl)) if rng.random() < 0.5 else 0
        rd = int(rng.integers(0, nreads)) if with_src else i
        loci = int(rng.integers(0, (1 << 32) - 140000))
        if rng.random() < 0.5:          # a second segment near the hit, on either side of its end
            rl, _, sl, fl = reads[rd]
            if not with_src:
                reads[rd] = (rl, max(0, loci + length + int(rng.integers(-50, 3000))), sl, fl)
        recs.append((int(rng.integers(1, 20)), loci, length, "+-"[int(rng.integers(0, 2))], tl, tr, rd))
    run(harness, tmp_path, recs, reads, with_src, with_trims, with_seg2)
