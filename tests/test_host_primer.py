"""Host logic on CPU: primer_correct.h - which records of a run the 5' primer correction asks the device about, the request it makes of
one, and what a canned answer does to the record and to the read's bytes (the high bits of every byte kept) - driven through
tests/cpp/primer_harness.cpp; and the `-6` option checks that end before anything touches a device."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import primer_ref as pr

BIN = os.path.join(helpers.ROOT, "biokanga_amd", "bin", "biokanga")
SRC = os.path.join(helpers.ROOT, "tests", "cpp", "primer_harness.cpp")
IN_DTYPE = np.dtype([("hit", helpers.HIT_DTYPE), ("read_len", "<u4"), ("two_seg", "<u4"), ("read", "u1", (16,)), ("_p", "<u4"), ("res", pr.PRIMER_RES_DTYPE)])
OUT_DTYPE = np.dtype([("selected", "<u4"), ("_p", "<u4"), ("req", pr.PRIMER_REQ_DTYPE), ("hit", helpers.HIT_DTYPE), ("read", "u1", (16,)), ("rc", "<i4")])
assert IN_DTYPE.itemsize == 64 and OUT_DTYPE.itemsize == 72
ACCEPTED, NOHIT = 1, 3


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("h") / "primer_harness")
    subprocess.check_call(helpers.cxx() + ["-o", exe, SRC])
    return exe


def run_harness(exe, tmp_path, rate, recs):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([rate], dtype="<i4").tobytes() + np.array([len(recs)], dtype="<u4").tobytes() + recs.tobytes())
    txt = subprocess.check_output([exe, inp, outp], text=True)
    raw = open(outp, "rb").read()
    out = np.frombuffer(raw[:len(recs) * OUT_DTYPE.itemsize], dtype=OUT_DTYPE)
    counts = np.frombuffer(raw[len(recs) * OUT_DTYPE.itemsize:], dtype="<u8")
    return out, [int(x) for x in counts], txt


def records(rate):
    """records of every kind the selection tells apart, with reads whose bytes carry high bits, and for the selected ones an answer made
    by the restatement against a random target window"""
    rng = np.random.default_rng(6)
    n = 600
    recs = np.zeros(n, dtype=IN_DTYPE)
    recs["read_len"] = rng.choice([50, 60, 75, 100], n)
    h = recs["hit"]
    h["chrom_id"], h["match_loci"], h["strand"] = rng.integers(1, 4, n), rng.integers(0, 10000, n), rng.choice([ord("+"), ord("-")], n)
    h["match_len"] = recs["read_len"]
    h["nar"] = np.where(rng.random(n) < 0.8, ACCEPTED, rng.choice([0, 2, 3, 4, 5], n))
    h["num_hits"] = (h["nar"] == ACCEPTED).astype(np.uint8)
    h["low_mm"] = rng.integers(0, 9, n)
    h["mismatches"] = h["low_mm"]
    recs["hit"] = h
    short = rng.random(n) < 0.1                      # match_len != read length
    recs["hit"]["match_len"][short] -= 3
    recs["two_seg"] = rng.random(n) < 0.1
    codes = rng.integers(0, 5, (n, 16)).astype(np.uint8)
    high = (rng.integers(0, 32, (n, 16)) << 3).astype(np.uint8)
    recs["read"] = codes | high
    exp_sel = np.zeros(n, dtype=bool)
    for i in range(n):
        hit, ln = recs["hit"][i], int(recs["read_len"][i])
        mms = pr.max_mms(rate, ln)
        exp_sel[i] = hit["nar"] == ACCEPTED and not recs["two_seg"][i] and int(hit["low_mm"]) > mms and int(hit["match_len"]) == ln
        tgt = [int(x) for x in rng.integers(0, 5, 12)]
        if i % 3 == 0:                               # near the read: a few mismatches only
            tgt = [int(x) for x in codes[i, :12]]
            for k in rng.choice(12, int(rng.integers(0, 5)), replace=False):
                tgt[k] = (tgt[k] + 1) % 5
        st, cur, after, fixed = pr.correct([int(x) for x in codes[i, :12]], tgt, int(hit["low_mm"]), mms)
        recs["res"][i] = (pr.pack_codes(after), sum(1 << k for k in fixed), st, cur, len(fixed), 0)
    return recs, codes, high, exp_sel


@pytest.mark.parametrize("rate", [0, 2, 5])
def test_selection_requests_patching_and_counts(harness, tmp_path, rate):
    recs, codes, high, exp_sel = records(rate)
    out, counts, txt = run_harness(harness, tmp_path, rate, recs)
    assert txt.split() == ["initial", "5", "15", "2", "7"]
    assert np.array_equal(out["selected"].astype(bool), exp_sel)
    assert 50 < exp_sel.sum() < len(recs) - 50
    want = [0, 0, 0]
    seen = set()
    for i in range(len(recs)):
        h0, h1, res = recs["hit"][i], out["hit"][i], recs["res"][i]
        if not exp_sel[i]:
            assert h1.tobytes() == h0.tobytes() and np.array_equal(out["read"][i], recs["read"][i]) and not out["req"][i].tobytes().strip(b"\0")
            continue
        q = out["req"][i]
        assert pr.unpack_codes(q["codes"]) == [int(x) for x in codes[i, :12]]
        assert (q["chrom_id"], q["match_loci"], q["match_len"], q["strand"], q["low_mm"]) == (h0["chrom_id"], h0["match_loci"], h0["match_len"], h0["strand"], h0["low_mm"])
        assert q["max_mms"] == pr.max_mms(rate, int(recs["read_len"][i])) and out["rc"][i] == 0
        seen.add(int(res["status"]))
        assert np.array_equal(out["read"][i] & 0xf8, high[i])                    # the high bits of every byte stay
        assert np.array_equal(out["read"][i][12:], recs["read"][i][12:])
        if res["status"] == pr.CORRECTED:
            assert [int(x) & 7 for x in out["read"][i][:12]] == pr.unpack_codes(res["codes"])
            assert (h1["low_mm"], h1["mismatches"], h1["nar"], h1["num_hits"]) == (res["mismatches"], res["mismatches"], ACCEPTED, 1)
            want[0] += 1
            want[1] += int(res["n_corrected"])
        else:
            assert res["status"] == pr.REJECTED
            assert np.array_equal(out["read"][i], recs["read"][i])
            assert (h1["nar"], h1["num_hits"], h1["low_mm"], h1["mismatches"]) == (NOHIT, 0, h0["low_mm"], h0["mismatches"])
            want[2] += 1
        for f in ("chrom_id", "match_loci", "match_len", "strand", "flags", "rslt", "low_hit_instances", "nxt_low_mm"):
            assert h1[f] == h0[f]
    assert counts == want and seen == {pr.CORRECTED, pr.REJECTED}


def test_a_flagged_answer_is_an_error(harness, tmp_path):
    recs, _, _, exp_sel = records(2)
    i = int(np.flatnonzero(exp_sel)[0])
    one = recs[i:i + 1].copy()
    one["res"]["status"] = pr.BAD
    out, counts, _ = run_harness(harness, tmp_path, 2, one)
    assert out["rc"][0] == -1 and counts == [0, 0, 0] and out["hit"][0].tobytes() == one["hit"][0].tobytes()


def test_harness_is_clean_under_sanitizers(tmp_path):
    """the same harness as a stand-alone program built with the address and undefined-behaviour sanitizers: reads of exactly twelve bytes
    included, a patch beyond them would be seen"""
    exe = str(tmp_path / "primer_harness_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-o", exe, SRC])
    recs, _, _, _ = records(2)
    out, counts, _ = run_harness(exe, tmp_path, 2, recs)
    assert counts[0] > 0 and counts[2] > 0


needs_bin = pytest.mark.skipif(not os.path.exists(BIN), reason="the command line has not been built (python -c 'import __graft_entry__ as g; g.build()')")


def run_cli(args, cwd=None):
    r = subprocess.run([BIN, "align", "-i", "none.fa", "-I", "none.sfx", "-o", "none.sam"] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    return r.returncode, r.stdout


@needs_bin
@pytest.mark.parametrize("args,n", [(["-6", "6"], 6), (["-6-1"], -1), (["--pcrprimersubs", "9"], 9)])
def test_range_error(args, n):
    rc, out = run_cli(args)
    assert rc == 1, out
    assert f"Error: PCR primer correction subs '-6{n}' specified outside of range 0..5" in out, out
    assert "Exit code: 1" in out


@needs_bin
def test_refused_with_chimeric_trimming():
    rc, out = run_cli(["-6", "2", "-c", "60"])
    assert rc == 1 and "Error: PCR primer correction subs not allowed when also specifying chimeric trimming" in out, out


@needs_bin
def test_refused_with_all_multiloci_records():
    rc, out = run_cli(["-6", "2", "-r5", "-R10"])
    assert rc == 1 and "'-62' is not available when reporting all multiloci alignments '-r5'" in out, out


@needs_bin
@pytest.mark.parametrize("args,n", [(["-6", "3", "-s2"], 3), (["--pcrprimersubs", "5", "-s", "12"], 5), (["-62", "-s0"], 2), (["-6", "1", "-r3", "-R5"], 1)])
def test_option_is_accepted(args, n, tmp_path):
    """the run gets as far as the index that is not there: the option itself is taken, and says so the way the reference does"""
    rc, out = run_cli(args, cwd=str(tmp_path))
    assert "unknown option" not in out and "outside of range" not in out, out
    assert f"correcting PCR 5' artefacts : {n}\n" in out, out
    assert "Loading suffix array file" in out, out


@needs_bin
def test_without_the_option_nothing_is_said(tmp_path):
    rc, out = run_cli(["-s2"], cwd=str(tmp_path))
    assert "PCR 5'" not in out and "Loading suffix array file" in out, out
    rc, out = run_cli(["-s2", "-6", "0"], cwd=str(tmp_path))
    assert "PCR 5'" not in out and "Loading suffix array file" in out, out
