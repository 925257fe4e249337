"""Host logic on CPU: site_prefs.h - the sequential half of CAligner::ProcessSiteProbabilites, the scaling through the reference-order
sort and WriteSitePrefs - fed the (codes, site) stream a numpy restatement of the gather derives from the golden genome for the reads
of the reference's own SAM, must write the reference's preference table byte for byte (tests/golden/siteprefs); and the `-8` / `-9`
option checks that end before anything touches a device."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import siteprefs_ref as sr

BIN = os.path.join(helpers.ROOT, "biokanga_amd", "bin", "biokanga")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("h") / "siteprefs_harness")
    subprocess.check_call(helpers.cxx() + ["-pthread", "-o", exe, os.path.join(helpers.ROOT, "tests", "cpp", "siteprefs_harness.cpp")])
    return exe


@pytest.fixture(scope="module")
def stream():
    g = sr.Genome()
    return g, sr.visits_from_sam(g, "dflt.sam.gz")


def run_harness(harness, tmp_path, reqs, res):
    rec = np.zeros(len(reqs), dtype=np.dtype([("q", reqs.dtype), ("r", res.dtype)]))
    rec["q"], rec["r"] = reqs, res
    assert rec.dtype.itemsize == 20
    inp, csv, sc = (str(tmp_path / n) for n in ("stream.bin", "prefs.csv", "scores.bin"))
    rec.tofile(inp)
    subprocess.check_call([harness, inp, csv, sc])
    return open(csv, "rb").read(), np.fromfile(sc, dtype=np.int32)


def test_the_planted_cases_are_in_the_stream(stream):
    """what the fixture was built to exercise is really there under the default offset"""
    g, reqs = stream
    res = sr.ref_octamers(g, reqs, -4)
    nothing = (res["codes"] & sr.NOTHING) != 0
    assert not nothing[0]
    assert nothing.sum() >= 4 and np.all(reqs["chrom_id"][nothing] == 2) and np.all(reqs["match_loci"][nothing] < 4)      # the wrapped sites
    clamped = res["site"] == g.lens[reqs["chrom_id"]] - 9
    assert clamped[reqs["strand"] == ord("-")].sum() >= 4
    b = (res["codes"][~nothing, None] >> (21 - 3 * np.arange(8, dtype=np.uint32))[None, :]) & 7
    assert (b > 3).any(axis=1).sum() >= 6                                                                                   # windows over the N run
    same = (res["site"][1:] == res["site"][:-1]) & (reqs["chrom_id"][1:] == reqs["chrom_id"][:-1])
    assert (same & (reqs["strand"][1:] != reqs["strand"][:-1])).sum() >= 1                                                  # '+' and '-' on one site
    assert same.sum() >= 40


@pytest.mark.parametrize("tag", ["dflt", "ofs0", "ofs7", "ofsm100"])
def test_host_pass_writes_the_reference_table(harness, stream, tmp_path, tag):
    g, reqs = stream
    c = sr.cases()[tag]
    csv, _ = run_harness(harness, tmp_path, reqs, sr.ref_octamers(g, reqs, c["ofs"]))
    assert csv == sr.golden(f"{c['prefs']}.siteprefs.csv.gz")


def test_scores_are_the_reference_bed_column(harness, stream, tmp_path):
    """-M4: the score of every record (Aligner.cpp:6447), looked up under the 8 bits the reference keeps of a read's SiteIdx"""
    g, reqs = stream
    _, scores = run_harness(harness, tmp_path, reqs, sr.ref_octamers(g, reqs, -4))
    bed = [l.split("\t") for l in sr.golden("m4.bed.gz").decode().splitlines()[1:]]
    assert len(bed) == len(reqs)
    assert [int(t[1]) for t in bed] == reqs["match_loci"].tolist()
    exp = np.array([int(t[4]) for t in bed])
    assert np.array_equal(scores, exp) and (exp > 0).sum() > 20


def test_first_read_out_of_range_is_skipped(harness, stream, tmp_path):
    """the reference's buffer is uninitialised there: the read is left out, the rest goes on as if it had not been visited"""
    g, reqs = stream
    res = sr.ref_octamers(g, reqs, -4)
    first = np.zeros(1, dtype=reqs.dtype)
    first[0] = (1, 0, 60, ord("+"), 0)
    r0 = sr.ref_octamers(g, first, -4)
    assert r0["codes"][0] == sr.NOTHING
    csv, _ = run_harness(harness, tmp_path, np.concatenate([first, reqs]), np.concatenate([r0, res]))
    assert csv == sr.golden("dflt.siteprefs.csv.gz")


needs_bin = pytest.mark.skipif(not os.path.exists(BIN), reason="the command line has not been built (python -c 'import __graft_entry__ as g; g.build()')")


def run_cli(args):
    r = subprocess.run([BIN, "align", "-i", "none.fa", "-I", "none.sfx", "-o", "none.sam"] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    return r.returncode, r.stdout


@needs_bin
@pytest.mark.parametrize("args,ofs", [(["-9", "101"], 101), (["-9-101"], -101), (["--siteprefsofs", "250", "-8", "p.csv"], 250)])
def test_offset_range_error(args, ofs, tmp_path):
    rc, out = run_cli(args)
    assert rc == 1, out
    assert f"Error: offset read start sites '-9{ofs}' when processing site octamer preferencing must be in range -100..100" in out, out
    assert "Exit code: 1" in out


@needs_bin
@pytest.mark.parametrize("args,ofs", [(["-8", "p.csv"], -4), (["--siteprefs", "p.csv", "-9", "-100"], -100), (["-8p.csv", "-9100"], 100)])
def test_options_are_accepted(args, ofs, tmp_path):
    """the run gets as far as the index that is not there: the options themselves are taken"""
    r = subprocess.run([BIN, "align", "-i", "none.fa", "-I", "none.sfx", "-o", "none.sam"] + args, cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=60)
    assert "unknown option" not in r.stdout and "must be in range" not in r.stdout, r.stdout
    assert f"Offset read start sites when processing site octamer preferencing: {ofs}\n" in r.stdout, r.stdout
    assert "Aligned read octamer site preferencing into this file: 'p.csv'" in r.stdout, r.stdout
    assert "Loading suffix array file" in r.stdout, r.stdout
