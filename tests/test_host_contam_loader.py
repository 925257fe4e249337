"""The loaders of `biokanga align -H` (host/read_loader.cpp) without a GPU: a host stand-in for the device matcher behind the loaders'
matcher interface (tests/cpp/contam_loader_harness.cpp).  The store every path makes - record loops, whole-file parses, -# sampling, mates -
must be the store the rule (contam_rule.py, held to the reference's runs by test_host_contaminants.py) predicts, scores cut with their
bases; and a second load that replays the kept cuts - the reload after a declined device SAM pass - must make the same store without
matching anything, whichever path either load takes."""
import gzip
import os
import subprocess

import pytest

import contam_rule as cr
import helpers


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cl") / "contam_loader_harness")
    host = os.path.join(helpers.ROOT, "biokanga_amd", "csrc", "host")
    src = [os.path.join(helpers.ROOT, "tests", "cpp", "contam_loader_harness.cpp")] + \
          [os.path.join(host, f) for f in ("read_loader.cpp", "contaminants.cpp", "fasta.cpp", "fast_inflate.cpp")]
    subprocess.check_call(helpers.cxx() + ["-pthread", "-o", exe] + src + ["-lz"])
    return exe


def load(harness, tmp_path, case, files, threads, reload_threads=0, qmode=3):
    """(store of the first load, store of the reload or None, files parsed whole after each load, reads matched in each load, log)"""
    fl = case["flags"]
    prefix = str(tmp_path / f"d{threads}_{reload_threads}")
    args = ["pe" if len(files) == 2 else "se", threads, reload_threads, cr.flag_value(fl, "-y", 0), cr.flag_value(fl, "-Y", 0), cr.flag_value(fl, "-l", 50),
            cr.flag_value(fl, "-L", 500), qmode, cr.flag_value(fl, "-#", 1), os.path.join(cr.CONTAM, case["contaminants"]), prefix] + files
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "rc " not in r.stdout and "replay left" not in r.stdout, r.stdout[-2000:]
    err = r.stderr.split()
    whole = [int(err[i + 1]) for i, w in enumerate(err) if w == "whole"]
    matched = [int(err[i + 1]) for i, w in enumerate(err) if w == "matched"]
    rd = lambda p: [tuple(l.rstrip("\n").split("\t")) for l in open(p)]
    return rd(prefix + ".load"), rd(prefix + ".reload") if reload_threads else None, whole, matched, r.stdout


def files_of(case, tmp_path, times=1):
    out = []
    for key in ("reads", "mates"):
        if key in case:
            p = str(tmp_path / f"x{times}_{case[key]}")
            if not os.path.exists(p):
                open(p, "wb").write(gzip.open(os.path.join(cr.CONTAM, case[key] + ".gz"), "rb").read() * times)
            out.append(p)
    return out


def predicted(case, times=1, sanger=False):
    kept, counts = cr.expected_store(case)
    score = lambda q: "0" * 0 if q is None else "".join("0123456789abcdef"[min(15, ((ord(c) - 33 + 2) * 15) // 40)] for c in q)
    rows = [(n, cr.norm(s), score(q) if sanger else "0" * len(s)) for n, s, q, _ in kept]
    return rows * times, [c * times for c in counts]


def count_lines(log):
    return [l.split(") ", 1)[-1] for l in log.splitlines() if "contaminate trimmed" in l or "contaminant trimmed" in l]


@pytest.mark.parametrize("tag", sorted(cr.cases()))
def test_record_loops_make_the_store_the_rule_predicts(harness, tmp_path, tag):
    case = cr.cases()[tag]
    qmode = 0 if "-g0" in case["flags"] else 3
    got, _, whole, matched, log = load(harness, tmp_path, case, files_of(case, tmp_path), 1, qmode=qmode)
    rows, counts = predicted(case, sanger=qmode == 0)
    assert got == rows and whole == [0]
    assert count_lines(log) == open(os.path.join(cr.CONTAM, tag + ".contam.txt")).read().splitlines()
    if qmode == 0:
        assert any(set(r[2]) - {"0"} for r in got)                # (scores present, and cut where the bases were cut)


@pytest.mark.parametrize("tag,whole_files", [("se13y3Y5", 1), ("se13l15", 1), ("fqg0", 1), ("pe24", 2), ("many", 1)])
def test_whole_file_parses_make_the_store_the_rule_predicts(harness, tmp_path, tag, whole_files):
    """files of a few MB by eight threads: accept_chunks / accept_pairs took them (the loaders' own count says so)"""
    case = cr.cases()[tag]
    qmode = 0 if "-g0" in case["flags"] else 3
    times = 40
    files = files_of(case, tmp_path, times)
    assert all(os.path.getsize(f) > (2 << 20) for f in files)
    got, _, whole, matched, log = load(harness, tmp_path, case, files, 8, qmode=qmode)
    rows, counts = predicted(case, times, sanger=qmode == 0)
    assert whole == [whole_files]
    assert got == rows
    want = [f"Load: total of {counts[0]} sequences PE1 sequences were 5' contaminate trimmed", f"Load: total of {counts[1]} sequences PE1 sequences were 3' contaminate trimmed"]
    if whole_files == 2:
        want += [f"Load: total of {counts[2]} sequences PE1 sequences were 5' contaminant trimmed", f"Load: total of {counts[3]} sequences PE1 sequences were 3' contaminant trimmed"]
    assert count_lines(log) == want


@pytest.mark.parametrize("tag", ["se13y3Y5", "pe24", "se13n2"])
@pytest.mark.parametrize("threads,reload_threads", [(8, 1), (1, 8), (8, 8), (1, 1)])
def test_reload_replays_the_kept_cuts(harness, tmp_path, tag, threads, reload_threads):
    """first load by one path, reload by the other (and by the same): the same store, nothing matched the second time"""
    case = cr.cases()[tag]
    files = files_of(case, tmp_path, 40)
    first, again, whole, matched, _ = load(harness, tmp_path, case, files, threads, reload_threads)
    rows, _ = predicted(case, 40)
    assert first == rows and again == rows
    assert matched[0] > 0 and matched[1] == 0
    if "-#2" not in case["flags"]:                                # (sampling keeps both loads in the record loops)
        per = len(files)
        assert whole == [per * (threads == 8), per * (threads == 8) + per * (reload_threads == 8)]
    else:
        assert whole == [0, 0]


def test_sampling_comes_before_the_match(harness, tmp_path):
    """-#2: every second raw read is matched and kept, the others are never looked at"""
    case = cr.cases()["se13n2"]
    files = files_of(case, tmp_path)
    got, _, whole, matched, _ = load(harness, tmp_path, case, files, 8)
    n_raw = open(files[0], "rb").read().count(b">")
    assert matched == [(n_raw + 1) // 2] and got == predicted(case)[0]
