"""Host logic on CPU: host/duplicates.h - the templates `align --mark-duplicates` makes of a record set, their requests and what the
answers do to the records - driven through tests/cpp/dup_harness.cpp, also built with the address and undefined-behaviour sanitizers.
The reference is tests/dup_ref.py over the SAM lines the writers would print for the same records: POS, CIGAR and FLAG are made here as
format_rec of host/report.cpp makes them."""
import subprocess

import numpy as np
import pytest

import dup_ref as dr
import helpers

SRC = helpers.ROOT + "/tests/cpp/dup_harness.cpp"
SEG2_DTYPE = np.dtype([("match_loci", "<u4"), ("match_len", "<u2"), ("read_ofs", "<u2"), ("mismatches", "u1"), ("flags", "u1"), ("score", "<u2")])
IN_DTYPE = np.dtype([("hit", helpers.HIT_DTYPE), ("tl", "<u2"), ("tr", "<u2"), ("seg2", SEG2_DTYPE), ("_p", "<u4")])
TMPL_DTYPE = np.dtype([("req", dr.DUP_REQ_DTYPE), ("first", "<u4")])
assert IN_DTYPE.itemsize == 40 and TMPL_DTYPE.itemsize == 20
ACCEPTED = 1
NAMES = {1: "dA", 2: "dB", 3: "dC"}
IDS = {v: k for k, v in NAMES.items()}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("h") / "dup_harness")
    if request.param == "plain":
        subprocess.check_call(helpers.cxx() + ["-o", exe, SRC])
    else:
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-o", exe, SRC])
    return exe


def run(exe, tmp_path, paired, recs):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([paired, len(recs)], dtype="<u4").tobytes() + recs.tobytes())
    subprocess.check_call([exe, inp, outp])
    raw = open(outp, "rb").read()
    nt = int(np.frombuffer(raw[:4], dtype="<u4")[0])
    tm = np.frombuffer(raw[4:4 + 20 * nt], dtype=TMPL_DTYPE)
    dup = np.frombuffer(raw[4 + 20 * nt:4 + 20 * nt + len(recs)], dtype=np.uint8)
    return tm, dup, int(np.frombuffer(raw[4 + 20 * nt + len(recs):], dtype="<i8")[0])


def record(chrom, loci, mlen, strand, nar=ACCEPTED, tl=0, tr=0, seg2=None, chimeric=False, pe_aligned=False, low_bits=0):
    r = np.zeros(1, dtype=IN_DTYPE)
    h = r["hit"]
    h["chrom_id"], h["match_loci"], h["match_len"], h["strand"], h["nar"] = chrom, loci, mlen, ord(strand), nar
    h["flags"] = (0x80 if pe_aligned else 0) | low_bits
    r["hit"] = h
    r["tl"], r["tr"] = tl, tr
    if seg2 is not None:                    # (kind, match_loci, match_len): kind 'N' | 'I' | 'D'
        r["seg2"]["flags"] = {"N": 4, "I": 3, "D": 1}[seg2[0]]
        r["seg2"]["match_loci"], r["seg2"]["match_len"] = seg2[1], seg2[2]
    elif chimeric:
        r["seg2"]["flags"], r["seg2"]["match_len"], r["seg2"]["read_ofs"] = 8, tl, tr
    return r[0]


def sam_lines(recs, paired, read_len=150):
    """the lines format_rec would write for these records (QNAME r<i>): clips in target order, the second segment behind the 3' clip"""
    lines, load = [], {}
    for i, r in enumerate(recs):
        h, g = r["hit"], r["seg2"]
        acc, plus = h["nar"] == ACCEPTED, h["strand"] == ord("+")
        flag = 0
        if not paired:
            flag = (0 if plus else 16) if acc else 4
        else:
            m = recs[i ^ 1]["hit"]
            flag = 0x1 | 0x2 | (0x80 if i & 1 else 0x40) | ((0 if plus else 0x10) if acc else 0x4)
            if (h["flags"] & 0x80) and (m["flags"] & 0x80) and m["nar"] == ACCEPTED:
                flag |= 0 if m["strand"] == ord("+") else 0x20
            else:
                flag |= 0x8
        load[f"r{i}"] = i
        if not acc:
            lines.append(dict(qname=f"r{i}", flag=flag, rname="*", pos=0, cigar=f"{read_len}M"))
            continue
        tl, tr = int(r["tl"]), int(r["tr"])
        c5, c3 = (tl, tr) if plus else (tr, tl)
        cigar = (f"{c5}S" if c5 else "") + f"{int(h['match_len']) - tl - tr}M" + (f"{c3}S" if c3 else "")
        if g["flags"] & 5:
            d = int(g["match_loci"]) - (int(h["match_loci"]) + int(h["match_len"]))
            if g["flags"] & 4:
                cigar += f"{d}N"
            elif g["flags"] & 2:
                cigar += f"{read_len - (int(h['match_len']) + int(g['match_len']))}I"
            else:
                cigar += f"{abs(d)}D"
            cigar += f"{int(g['match_len'])}M"
        lines.append(dict(qname=f"r{i}", flag=flag, rname=NAMES[int(h["chrom_id"])], pos=int(h["match_loci"]) + (tl if plus else tr) + 1, cigar=cigar))
    return lines, load


def check(harness, tmp_path, recs, paired):
    recs = np.array(recs, dtype=IN_DTYPE)
    tm, dup, n_marked = run(harness, tmp_path, paired, recs)
    lines, load = sam_lines(recs, paired)
    exp, members = dr.requests_of_sam(lines, load, IDS)
    assert tm["req"].tolist() == exp.tolist()
    assert tm["first"].tolist() == [m[0] for m in members]
    want = np.zeros(len(recs), dtype=np.uint8)
    for t, ks in enumerate(members):
        if t % 3 == 1:
            want[ks] = 1
    assert dup.tolist() == want.tolist() and n_marked == int(want.sum())
    return tm


def test_plain_records(harness, tmp_path):
    recs = [record(1, 100, 100, "+"), record(1, 100, 100, "-"), record(2, 0, 50, "+"), record(3, 7, 64, "-", nar=3), record(1, 100, 100, "?", nar=3),
            record(2, 0, 50, "+", low_bits=0x41)]
    tm = check(harness, tmp_path, recs, 0)
    # by hand: '+' at its start, '-' at its last base; the unaccepted records make no template, whatever bk_hit.flags holds below bit 7
    assert [(int(q["chrom_id"]), int(q["pos5"]), chr(q["strand"]), int(q["score"]), int(q["strand_mate"])) for q in tm["req"]] == \
        [(1, 100, "+", 100, 0), (1, 199, "-", 100, 0), (2, 0, "+", 50, 0), (2, 0, "+", 50, 0)]
    assert tm["first"].tolist() == [0, 1, 2, 5]


def test_end_trims_on_both_strands_give_back_the_untrimmed_ends(harness, tmp_path):
    recs = [record(1, 100, 100, "+", tl=3, tr=5), record(1, 100, 100, "-", tl=3, tr=5), record(1, 2, 100, "+", tl=9), record(1, 100, 100, "+"), record(1, 100, 100, "-")]
    tm = check(harness, tmp_path, recs, 0)
    # '+': POS moves to 103, 3S in front: 100 again.  '-': POS moves to 105 (the right trim), 92M, 3S behind: 105 + 92 - 1 + 3 = 199 again
    assert tm["req"]["pos5"].tolist() == [100, 199, 2, 100, 199] and tm["req"]["score"].tolist() == [92, 92, 91, 100, 100]


def test_chimeric_trims(harness, tmp_path):
    recs = [record(2, 500, 120, "+", tl=20, tr=10, chimeric=True), record(2, 500, 120, "-", tl=20, tr=10, chimeric=True), record(2, 5, 120, "+", tl=30, chimeric=True)]
    tm = check(harness, tmp_path, recs, 0)
    assert tm["req"]["pos5"].tolist() == [500, 619, 5] and tm["req"]["score"].tolist() == [90, 90, 90]


@pytest.mark.parametrize("kind,gap", [("N", 1500), ("I", 0), ("D", 7)])
def test_second_segments(harness, tmp_path, kind, gap):
    recs = [record(3, 1000, 60, "+", seg2=(kind, 1060 + gap, 80)), record(3, 1000, 60, "-", seg2=(kind, 1060 + gap, 80)), record(3, 1000, 60, "-")]
    tm = check(harness, tmp_path, recs, 0)
    assert tm["req"]["pos5"].tolist() == [1000, 1000 + 60 + gap + 80 - 1, 1059] and tm["req"]["score"].tolist() == [140, 140, 60]


def test_pairs_orphans_and_ends_treated_as_single(harness, tmp_path):
    recs = [record(1, 100, 100, "+", pe_aligned=True), record(1, 300, 100, "-", pe_aligned=True, tr=4),          # a pair
            record(1, 300, 100, "-", pe_aligned=True), record(1, 100, 100, "+", pe_aligned=True, tl=2),          # the same ends, PE1 and PE2 swapped
            record(1, 100, 100, "+"), record(1, 300, 100, "-", nar=15),                                          # an orphan end
            record(1, 100, 100, "+"), record(2, 300, 100, "-"),                                                  # both accepted, not paired: two fragments
            record(1, 100, 100, "+", pe_aligned=True), record(1, 300, 100, "-", nar=3, pe_aligned=True),         # a stale pair bit beside an unaccepted mate
            record(3, 10, 50, "-", nar=3), record(3, 10, 50, "+", nar=4)]
    tm = check(harness, tmp_path, recs, 1)
    q = tm["req"]
    assert tm["first"].tolist() == [0, 2, 4, 6, 7, 8]
    assert [chr(x) if x else "" for x in q["strand_mate"]] == ["-", "+", "", "", "", ""]
    assert (int(q[0]["pos5"]), int(q[0]["pos5_mate"]), int(q[0]["score"])) == (100, 399, 196)
    assert (int(q[1]["pos5"]), int(q[1]["pos5_mate"]), int(q[1]["score"])) == (399, 100, 198)
    assert dr.key_of(q[0]) == dr.key_of(q[1])
    # the same records as single ends: every accepted one a fragment
    tm = check(harness, tmp_path, recs, 0)
    assert len(tm) == 8 and not tm["req"]["strand_mate"].any()


def test_random_records(harness, tmp_path):
    rng = np.random.default_rng(20261020)
    recs = []
    for i in range(600):
        strand = "+-"[int(rng.integers(0, 2))]
        nar = ACCEPTED if rng.random() < 0.8 else int(rng.choice([0, 3, 4, 15]))
        shape = int(rng.integers(0, 6))
        kw = {}
        if shape == 1:
            kw = dict(tl=int(rng.integers(0, 9)), tr=int(rng.integers(0, 9)))
        elif shape == 2:
            kw = dict(tl=int(rng.integers(0, 30)), tr=int(rng.integers(0, 30)), chimeric=True)
        elif shape == 3:
            kind = "NID"[int(rng.integers(0, 3))]
            kw = dict(seg2=(kind, 0, int(rng.integers(10, 60))))
        loci, mlen = int(rng.integers(0, 40)) * 5, int(rng.choice([60, 70, 90]))
        if "seg2" in kw:
            kw["seg2"] = (kw["seg2"][0], loci + mlen + {"N": 900, "I": 0, "D": 3}[kw["seg2"][0]], kw["seg2"][2])
        recs.append(record(int(rng.integers(1, 4)), loci, mlen, strand, nar=nar, pe_aligned=bool(rng.integers(0, 2)), **kw))
    recs = np.array(recs, dtype=IN_DTYPE)
    recs["hit"]["flags"][1::2] = recs["hit"]["flags"][0::2]               # the pair bit on both mates or on neither ..
    recs["hit"]["chrom_id"][1::2] = recs["hit"]["chrom_id"][0::2]         # .. and mates on one sequence
    assert len(check(harness, tmp_path, recs, 0)) > 400
    tm = check(harness, tmp_path, recs, 1)
    assert 50 < (tm["req"]["strand_mate"] != 0).sum() < 200
