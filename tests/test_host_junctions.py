"""Host logic on CPU: host/junctions.h - the requests `align --junctions` / `--splice-strand` make of a record set, what the strand answers
do to the records and the table's lines - driven through tests/cpp/junction_harness.cpp, also built with the address and
undefined-behaviour sanitizers.  The reference is tests/junction_ref.py over the SAM lines the writers would print for the same records:
POS and CIGAR are made as format_rec of host/report.cpp makes them (sam_lines of tests/test_host_duplicates.py)."""
import subprocess

import numpy as np
import pytest

import helpers
import junction_ref as jr
from test_host_duplicates import ACCEPTED, IDS, IN_DTYPE, record, sam_lines

SRC = helpers.ROOT + "/tests/cpp/junction_harness.cpp"
REQ_DTYPE = np.dtype([("req", jr.JUNCTION_REQ_DTYPE), ("rec", "<u4")])
assert REQ_DTYPE.itemsize == 20


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("h") / "junction_harness")
    if request.param == "plain":
        subprocess.check_call(helpers.cxx() + ["-o", exe, SRC])
    else:
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-o", exe, SRC])
    return exe


def run(exe, tmp_path, recs):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([0, len(recs)], dtype="<u4").tobytes() + recs.tobytes())
    subprocess.check_call([exe, inp, outp])
    raw = open(outp, "rb").read()
    nt = int(np.frombuffer(raw[:4], dtype="<u4")[0])
    rq = np.frombuffer(raw[4:4 + 20 * nt], dtype=REQ_DTYPE)
    at = 4 + 20 * nt
    xs = np.frombuffer(raw[at:at + len(recs)], dtype=np.uint8)
    n_tagged = int(np.frombuffer(raw[at + len(recs):at + len(recs) + 8], dtype="<i8")[0])
    return rq, xs, n_tagged, raw[at + len(recs) + 8:].decode()


def check(harness, tmp_path, recs):
    recs = np.array(recs, dtype=IN_DTYPE)
    rq, xs, n_tagged, text = run(harness, tmp_path, recs)
    lines, _ = sam_lines(recs, 0)
    exp, line_of = jr.requests_of_sam(lines, IDS)
    assert rq["req"].tolist() == exp.tolist()
    assert rq["rec"].tolist() == line_of
    want = np.zeros(len(recs), dtype=np.uint8)
    for t, k in enumerate(line_of):
        want[k] = (ord("+"), ord("-"), 0)[t % 3]
    assert xs.tolist() == want.tolist() and n_tagged == int((want != 0).sum())
    # the table's lines: name, start + 1, end, strand code, motif, 0, reads, 0, overhang
    exp_text = "".join(f"d{'ABC'[int(q['chrom_id']) - 1]}\t{int(q['start']) + 1}\t{int(q['end'])}\t{(0, 1, 2, 1, 2, 1, 2)[t % 7]}\t{t % 7}\t0\t{t + 1}\t0\t{int(q['overhang'])}\n"
                       for t, q in enumerate(exp))
    assert text == exp_text
    return rq


def test_spliced_records_on_both_strands(harness, tmp_path):
    recs = [record(3, 1000, 60, "+", seg2=("N", 2560, 80)), record(3, 1000, 60, "-", seg2=("N", 2560, 80)), record(3, 1000, 60, "-"),
            record(1, 10, 90, "+", seg2=("N", 130, 10)), record(2, 0, 30, "-", seg2=("N", 31, 120))]
    rq = check(harness, tmp_path, recs)
    # by hand: the intron starts behind the first M run and is `gap` long, whatever the read's strand
    assert [(int(q["chrom_id"]), int(q["start"]), int(q["end"]), int(q["overhang"])) for q in rq["req"]] == \
        [(3, 1060, 2560, 60), (3, 1060, 2560, 60), (1, 100, 130, 10), (2, 30, 31, 30)]
    assert rq["rec"].tolist() == [0, 1, 3, 4]


def test_end_trims_on_both_strands(harness, tmp_path):
    """-x / -A trims: POS moves by the 5' clip (in target order) and m shrinks by both, so the line's POS - 1 + m is what it was minus
    the 3' clip - and the writers put that clip in front of the N"""
    recs = [record(1, 100, 100, "+", tl=3, tr=5, seg2=("N", 700, 50)), record(1, 100, 100, "-", tl=3, tr=5, seg2=("N", 700, 50)),
            record(1, 100, 100, "+", seg2=("N", 700, 50)), record(1, 100, 100, "+", tl=9, seg2=("N", 700, 95))]
    rq = check(harness, tmp_path, recs)
    # '+': POS 104, 92M, 5S: start 103 + 92 = 195, gap 500.  '-': POS 106 (the right trim leads), 92M, 3S: start 105 + 92 = 197
    assert [(int(q["start"]), int(q["end"]), int(q["overhang"])) for q in rq["req"]] == [(195, 695, 50), (197, 697, 50), (200, 700, 50), (200, 700, 91)]


def test_records_that_make_no_request(harness, tmp_path):
    recs = [record(1, 100, 100, "+", seg2=("I", 200, 40)), record(1, 100, 100, "+", seg2=("D", 205, 40)), record(1, 100, 100, "+", nar=3, seg2=("N", 700, 50)),
            record(1, 100, 100, "?", nar=3), record(2, 500, 120, "+", tl=20, tr=10, chimeric=True), record(1, 100, 100, "+", seg2=("N", 200, 50)),
            record(1, 100, 100, "+", seg2=("N", 150, 50)), record(2, 7, 64, "-", seg2=("N", 9000, 64))]
    rq = check(harness, tmp_path, recs)
    # an N of 0 bases, or a second segment in front of the first's end, is no intron: the record makes no request
    assert rq["rec"].tolist() == [7]


def test_random_records(harness, tmp_path):
    rng = np.random.default_rng(20261020)
    recs = []
    for i in range(600):
        strand = "+-"[int(rng.integers(0, 2))]
        nar = ACCEPTED if rng.random() < 0.8 else int(rng.choice([0, 3, 4, 15]))
        shape = int(rng.integers(0, 6))
        loci, mlen = int(rng.integers(0, 40)) * 5, int(rng.choice([60, 70, 90]))
        kw = {}
        if shape == 1:
            kw = dict(tl=int(rng.integers(0, 9)), tr=int(rng.integers(0, 9)))
        elif shape == 2:
            kw = dict(tl=int(rng.integers(0, 30)), tr=int(rng.integers(0, 30)), chimeric=True)
        elif shape >= 3:
            kind = "NNID"[int(rng.integers(0, 4))]
            kw = dict(seg2=(kind, loci + mlen + {"N": int(rng.integers(1, 40)) * 25, "I": 0, "D": 3}[kind], int(rng.integers(10, 60))))
            if kind == "N" and rng.random() < 0.5:
                kw.update(tl=int(rng.integers(0, 9)), tr=int(rng.integers(0, 9)))
        recs.append(record(int(rng.integers(1, 4)), loci, mlen, strand, nar=nar, **kw))
    rq = check(harness, tmp_path, recs)
    trimmed = sum(1 for k in rq["rec"] if recs[k]["tl"] or recs[k]["tr"])
    minus = sum(1 for k in rq["rec"] if recs[k]["hit"]["strand"] == ord("-"))
    assert len(rq) > 100 and trimmed > 30 and 30 < minus < len(rq) - 30
