"""Host logic on CPU: loci_constraints.h - the constraints CSV as the reference reads it, with its refusals word for word, the request
made of one record from its adjusted loci, and what canned answers do to the records and their mates - driven through
tests/cpp/constraints_harness.cpp, also built with the address and undefined-behaviour sanitizers; and the `-5` option up to the point
where the run needs its index."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import constraints_ref as cr

BIN = os.path.join(helpers.ROOT, "biokanga_amd", "bin", "biokanga")
SRC = os.path.join(helpers.ROOT, "tests", "cpp", "constraints_harness.cpp")
SEG2_DTYPE = np.dtype([("match_loci", "<u4"), ("match_len", "<u2"), ("read_ofs", "<u2"), ("mismatches", "u1"), ("flags", "u1"), ("score", "<u2")])
IN_DTYPE = np.dtype([("hit", helpers.HIT_DTYPE), ("a_start", "<u4"), ("a_len", "<u4"), ("trim_left", "<u4"), ("has_seg2", "<u4"), ("seg2", SEG2_DTYPE),
                     ("read_ofs", "<u8"), ("read_len", "<u4"), ("status", "<u4")])
OUT_DTYPE = np.dtype([("selected", "<u4"), ("rc", "<i4"), ("req", cr.CONSTRAINT_REQ_DTYPE), ("hit", helpers.HIT_DTYPE), ("_p", "<u4")])
assert IN_DTYPE.itemsize == 64 and OUT_DTYPE.itemsize == 64 and SEG2_DTYPE.itemsize == 12
ACCEPTED = 1
NAMES, LENS = ["lcA", "lc,B", "lcC"], [28000, 18000, 10000]
MANY = [f"m{k:02d}" for k in range(cr.MAX_CHROMS + 2)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the harness as the other host harnesses are built, and once more as a stand-alone program under the sanitizers"""
    exe = str(tmp_path_factory.mktemp("h") / "constraints_harness")
    if request.param == "plain":
        subprocess.check_call(helpers.cxx() + ["-o", exe, SRC])
    else:
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-o", exe, SRC])
    return exe


def write_entries(path, names, lens, ids=None):
    with open(path, "w") as f:
        for i, (n, ln) in enumerate(zip(names, lens)):
            f.write(f"{ids[i] if ids else i + 1} {ln} {n}\n")
    return path


def load(exe, cwd, csv, entries):
    r = subprocess.run([exe, "load", csv, entries, "out.bin"], cwd=cwd, stdout=subprocess.PIPE, text=True)
    if r.returncode:
        assert r.returncode == 1, r
        return None, r.stdout.rstrip("\n")
    return np.fromfile(os.path.join(cwd, "out.bin"), dtype=cr.CONSTRAINT_DTYPE), r.stdout.split()


def test_main_file_loads_as_the_restatement_loads_it(harness, tmp_path):
    helpers.gunzip_to(os.path.join(cr.DIR, "main.csv.gz"), str(tmp_path / "main.csv"))
    ents = write_entries(str(tmp_path / "ents.txt"), NAMES, LENS)
    got, said = load(harness, str(tmp_path), "main.csv", ents)
    want = cr.load_constraints(str(tmp_path / "main.csv"), NAMES, LENS)
    assert said == ["ok", str(len(want)), "3"]
    assert sorted((int(c["chrom_id"]), int(c["start"]), int(c["end"]), int(c["mask"])) for c in got) == want
    assert not got["_r"].any()
    # EntryIDs as the index has them, not positions
    ents = write_entries(str(tmp_path / "ents2.txt"), NAMES, LENS, ids=[7, 3, 12])
    got2, _ = load(harness, str(tmp_path), "main.csv", ents)
    assert np.array_equal(got2["chrom_id"], np.array([0, 7, 3, 12], dtype=np.uint32)[got["chrom_id"]])


@pytest.mark.parametrize("tag", sorted(cr.spec()["errors"]))
def test_refusals_word_for_word(harness, tmp_path, tag):
    e = cr.spec()["errors"][tag]
    if tag != "e_missing":
        helpers.gunzip_to(os.path.join(cr.DIR, e["file"] + ".gz"), str(tmp_path / e["file"]))
    names, lens = (NAMES, LENS) if e["index"] == "genome" else (MANY, [120] * len(MANY))
    got, said = load(harness, str(tmp_path), e["file"], write_entries(str(tmp_path / "ents.txt"), names, lens))
    assert got is None and said == e["messages"][-2]


def test_reader_corners_and_limits(harness, tmp_path):
    ents = write_entries(str(tmp_path / "ents.txt"), NAMES, LENS)
    many = write_entries(str(tmp_path / "many.txt"), MANY, [120] * len(MANY))

    def put(text, name="t.csv"):
        with open(str(tmp_path / name), "w", newline="") as f:
            f.write(text)
        return name

    # CR LF lines, a comment, blank lines, "" inside quotes, no line feed at the end, text behind a closing quote
    got, said = load(harness, str(tmp_path), put('\r\n# c,o,m\r\n  "lcA" junk , 5 ,7x,"a""c"\r\n\r\nLCC,0,0,r'), ents)
    assert said is not None and got is None and said == "Illegal base specifiers for 'lcA' at line 2 in 't.csv'"
    got, said = load(harness, str(tmp_path), put('\r\n# c,o,m\r\n  "lcA" junk , 5 ,7x,"a c"\r\n\r\nLCC,0,0,r'), ents)
    assert said == ["ok", "2", "2"] and [tuple(int(x) for x in (c["chrom_id"], c["start"], c["end"], c["mask"])) for c in got] == [(1, 5, 7, 3), (3, 0, 0, 16)]
    # a first line of text only is a header; one with a number in it is data
    assert load(harness, str(tmp_path), put("lcA,five,seven,A\nlcA,1,1,A\n"), ents)[1] == ["ok", "1", "1"]
    assert load(harness, str(tmp_path), put("lcA,0,seven,A\nlcA,1,1,A\n"), ents)[1] == ["ok", "2", "1"]
    # the limits themselves are taken
    assert load(harness, str(tmp_path), put("".join(f"lcA,{k},{k},A\n" for k in range(cr.MAX_LOCI))), ents)[1] == ["ok", "6400", "1"]
    assert load(harness, str(tmp_path), put("".join(f"m{k:02d},5,5,A\n" for k in range(cr.MAX_CHROMS))), many)[1] == ["ok", "64", "64"]
    # files the reference cannot size: empty, shorter than five bytes, comments only
    for text in ("", "a,b\n", "# nothing here\n"):
        assert load(harness, str(tmp_path), put(text), ents) == (None, "Unable to open 't.csv' for processing")
    for text in ("lcA,1,1,A\n", "x,1,1,A\n# c\n"):
        try:
            want = ["ok", str(len(cr.load_constraints(str(tmp_path / put(text)), NAMES, LENS))), "1"]
        except cr.LoadError as err:
            want = str(err).replace(str(tmp_path) + "/", "")
        assert load(harness, str(tmp_path), "t.csv", ents)[1] == want


def records(paired):
    rng = np.random.default_rng(55)
    n = 800
    recs = np.zeros(n, dtype=IN_DTYPE)
    h = recs["hit"]
    h["chrom_id"], h["match_loci"], h["strand"] = rng.integers(0, 6, n), rng.integers(0, 10000, n), rng.choice([ord("+"), ord("-")], n)
    h["match_len"] = rng.choice([50, 60, 100], n)
    h["nar"] = np.where(rng.random(n) < 0.8, ACCEPTED, rng.choice([0, 2, 3, 4, 5], n))
    h["num_hits"] = (h["nar"] == ACCEPTED).astype(np.uint8)
    h["low_hit_instances"] = h["num_hits"]
    recs["hit"] = h
    recs["trim_left"], tr = rng.integers(0, 9, n), rng.integers(0, 9, n)
    recs["a_start"] = h["match_loci"] + np.where(h["strand"] == ord("+"), recs["trim_left"], tr)
    recs["a_len"] = h["match_len"] - recs["trim_left"] - tr
    recs["has_seg2"] = rng.random(n) < 0.2
    recs["seg2"]["match_loci"], recs["seg2"]["match_len"], recs["seg2"]["read_ofs"] = rng.integers(0, 10000, n), rng.integers(5, 40, n), rng.integers(20, 60, n)
    recs["read_ofs"] = rng.integers(0, 1 << 40, n)
    recs["read_len"] = h["match_len"] + rng.integers(0, 40, n)
    recs["status"] = rng.choice([cr.UNTOUCHED, cr.TOUCHED, cr.VIOLATED], n, p=[0.4, 0.3, 0.3])
    constrained = np.array([0, 1, 0, 1, 1], dtype=np.uint8)       # chrom_id 5 lies beyond the table
    return recs, constrained


def run_apply(exe, tmp_path, paired, recs, constrained):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([paired, len(recs), len(constrained)], dtype="<u4").tobytes() + constrained.tobytes() + recs.tobytes())
    subprocess.check_call([exe, "apply", inp, outp])
    raw = open(outp, "rb").read()
    return np.frombuffer(raw[:len(recs) * 64], dtype=OUT_DTYPE), [int(x) for x in np.frombuffer(raw[len(recs) * 64:], dtype="<u8")]


@pytest.mark.parametrize("paired", [0, 1])
def test_selection_requests_marking_and_mates(harness, tmp_path, paired):
    recs, constrained = records(paired)
    out, counts = run_apply(harness, tmp_path, paired, recs, constrained)
    h0 = recs["hit"]
    sel = (h0["nar"] == ACCEPTED) & np.isin(h0["chrom_id"], [1, 3, 4])
    assert np.array_equal(out["selected"].astype(bool), sel) and 100 < sel.sum() < len(recs) - 100
    own = sel & (recs["status"] == cr.VIOLATED)
    marked = own.copy()
    if paired:
        pair = own.reshape(-1, 2).any(axis=1)
        marked = np.repeat(pair, 2)
    assert counts == [int(own.sum()), int(marked.sum() - own.sum())] and own.sum() > 50 and (not paired or counts[1] > 20)
    for i in range(len(recs)):
        q, h1 = out["req"][i], out["hit"][i]
        if sel[i]:
            two = bool(recs["has_seg2"][i])
            assert (q["read_ofs"], q["chrom_id"], q["read_len"], q["strand"], q["n_segs"]) == (recs["read_ofs"][i], h0["chrom_id"][i], recs["read_len"][i], h0["strand"][i], 2 if two else 1)
            assert tuple(q["seg"][0]) == (recs["a_start"][i], recs["a_len"][i], recs["trim_left"][i])
            assert tuple(q["seg"][1]) == ((recs["seg2"]["match_loci"][i], recs["seg2"]["match_len"][i], recs["seg2"]["read_ofs"][i]) if two else (0, 0, 0))
            assert out["rc"][i] == int(own[i])
        else:
            assert not q.tobytes().strip(b"\0") and out["rc"][i] == 0
        if marked[i]:
            assert (h1["nar"], h1["num_hits"], h1["low_hit_instances"]) == (cr.NAR_LC, 0, 0)
            for f in ("chrom_id", "match_loci", "match_len", "strand", "low_mm", "mismatches", "flags", "rslt", "nxt_low_mm"):
                assert h1[f] == h0[f][i]
        else:
            assert h1.tobytes() == h0[i].tobytes()


def test_a_flagged_answer_is_an_error(harness, tmp_path):
    recs, constrained = records(0)
    i = int(np.flatnonzero((recs["hit"]["nar"] == ACCEPTED) & (recs["hit"]["chrom_id"] == 1))[0])
    for status in (cr.BAD, 3, 0xA5):
        one = recs[i:i + 1].copy()
        one["status"] = status
        out, counts = run_apply(harness, tmp_path, 0, one, constrained)
        assert out["rc"][0] == -1 and counts == [0, 0] and out["hit"][0].tobytes() == one["hit"][0].tobytes()


needs_bin = pytest.mark.skipif(not os.path.exists(BIN), reason="the command line has not been built (python -c 'import __graft_entry__ as g; g.build()')")


def run_cli(args, cwd=None):
    r = subprocess.run([BIN, "align", "-i", "none.fa", "-I", "none.sfx", "-o", "none.sam"] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    return r.returncode, r.stdout


@needs_bin
@pytest.mark.parametrize("args", [["-5", "some.csv"], ["--lociconstraints", "some.csv"], ["-5some.csv", "-r5", "-R5"]])
def test_option_is_accepted(args, tmp_path):
    """the run gets as far as the index that is not there: the option itself is taken, and says so the way the reference does"""
    rc, out = run_cli(args, cwd=str(tmp_path))
    assert "unknown option" not in out, out
    assert "Loci base constraints file: 'some.csv'\n" in out, out
    assert "Loading suffix array file" in out, out


@needs_bin
def test_without_the_option_nothing_is_said(tmp_path):
    rc, out = run_cli(["-s2"], cwd=str(tmp_path))
    assert "constraint" not in out.lower() and "Loading suffix array file" in out, out
