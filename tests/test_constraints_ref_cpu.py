"""The restatement of the loci base constraints (constraints_ref.py: CAligner::LoadLociConstraints, AcceptBaseConstraint,
AcceptLociConstraints, IdentifyConstraintViolations) against the reference binary's own output: every run of tests/golden/constraints
is replayed from the SAM of the run WITHOUT -5 plus the genome and the constraints file, and must mark exactly the records the
reference marked LC - with -U the mates too; the loader must refuse every recorded file with the reference's words.  No GPU: this pins
the yardstick the GPU tests use."""
import os

import numpy as np
import pytest

import helpers
import constraints_ref as cr

CASES = cr.spec()["cases"]
M6 = sorted(t for t, c in CASES.items() if c.get("m6", True))
NAMES, LENS = ["lcA", "lc,B", "lcC"], [28000, 18000, 10000]
MANY = [f"m{k:02d}" for k in range(cr.MAX_CHROMS + 2)]


@pytest.fixture(scope="module")
def genome():
    g = cr.Genome(os.path.join(cr.DIR, "genome.fa.gz"))
    assert g.names == NAMES and [g.length(i) for i in (1, 2, 3)] == LENS
    return g


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    path = helpers.gunzip_to(os.path.join(cr.DIR, "main.csv.gz"), str(tmp_path_factory.mktemp("c") / "main.csv"))
    return cr.load_constraints(path, NAMES, LENS)


def test_the_cases_cover_what_they_are_for():
    assert set(CASES) >= {"s3", "c50", "a5", "A1000", "r3", "r5", "U3", "U2", "k", "p6", "x3", "Z", "snp"}
    for tag, c in CASES.items():
        if c.get("m6", True):
            assert c["lc"] >= 20 and c["stay"] >= 20 and c["identified"] == c["lc"], tag
    for tag in ("c50", "a5", "A1000"):
        assert CASES[tag]["decided_lc"] >= 1 and CASES[tag]["decided_stay"] >= 1, tag
    largest = max(os.path.getsize(os.path.join(helpers.GOLDEN, "primer", f)) for f in os.listdir(os.path.join(helpers.GOLDEN, "primer")))
    assert all(os.path.getsize(os.path.join(cr.DIR, f)) <= largest for f in os.listdir(cr.DIR))


def test_the_main_file_as_loaded(table):
    """header line skipped, quoted names, blanks around fields and inside the bases field, a fifth field, the name without case; sorted"""
    assert len(table) == 20 and table == sorted(table)
    assert (1, 0, 0, 0x03) in table and (1, 1500, 1500, 0x01) in table and (1, 5100, 5139, 0x10) in table and (1, 27999, 27999, 0x14) in table
    assert (2, 3010, 3020, 0x03) in table and (2, 12000, 12000, 0x0a) in table and (2, 17999, 17999, 0x10) in table
    assert (3, 4000, 4000, 0x04) in table and (3, 4000, 4000, 0x10) in table and (3, 9999, 9999, 0x0a) in table


def test_the_reader_on_hand_made_lines():
    lines = cr.csv_lines('  a , "b ""q"" , c" x,,\r\n# gone\n\n"only"\n1,2')
    assert [[f for f in ln[0]] for ln in lines] == [[("a", False), ('b "q" , c', True), ("", False), ("", False)], [("only", True)], [("1", False), ("2", False)]]
    # (a line ended by CR LF is parsed up to the CR: its line feed is counted when the next line is looked for)
    assert [ln[1] for ln in lines] == [0, 4, 4]
    assert cr.likely_header([("Seq", False), ("Start", False)]) and cr.likely_header([("1", True), ("", False)])
    assert not cr.likely_header([("lcA", False), ("5", False)]) and not cr.likely_header([("a", False), ("1e3", False)])
    assert not cr.likely_header([("", False)] * 3 + [("a", False)])
    assert [cr.atoi(s) for s in ("12", " -5x", "x", "+7", "")] == [12, -5, 0, 7, 0]


def test_accept_base_on_hand_made_constraints(genome):
    t = [(1, 10, 10, 0x0a), (1, 20, 27, 0x10), (1, 22, 22, 0x01), (2, 8000, 8019, 0x10)]
    tgt = int(genome.codes[1][10])
    assert [cr.accept_base(genome, t, 1, 10, b) for b in range(5)] == [-1, 1, -1, 1, -1]
    assert cr.accept_base(genome, t, 1, 11, 4) == 1 and cr.accept_base(genome, t, 3, 10, 0) == 0
    # R: the target's base, nothing else; a second constraint on the locus must hold too
    at20, at22 = int(genome.codes[1][20]), int(genome.codes[1][22])
    assert [cr.accept_base(genome, t, 1, 20, b) for b in range(5)] == [1 if b == at20 else -1 for b in range(5)]
    assert [cr.accept_base(genome, t, 1, 22, b) for b in range(5)] == [1 if (b == at22 and b == 0) else -1 for b in range(5)]
    # a read N equals a target N under R
    assert int(genome.codes[2][8000]) == 4 and cr.accept_base(genome, t, 2, 8000, 4) == 1 and cr.accept_base(genome, t, 2, 8000, 0) == -1
    assert tgt in range(4)


def test_request_restatements_agree(genome, table):
    """the requests the GPU tests use: the per-base walk and the all-at-once form give the same statuses, of every kind; bad ones flagged"""
    reqs, bases = cr.make_requests(genome, table)
    st = cr.ref_check(genome, table, reqs, bases)
    assert np.array_equal(st, cr.ref_check(genome, table, reqs, bases, per_base=True))
    assert (st == cr.UNTOUCHED).sum() > 500 and (st == cr.TOUCHED).sum() > 100 and (st == cr.VIOLATED).sum() > 200 and not (st == cr.BAD).any()
    two = reqs["n_segs"] == 2
    first_clear = np.array([cr.ref_check(genome, table, r.reshape(1), bases)[0] for r in _first_segment_only(reqs[two])])
    assert ((st[two] == cr.VIOLATED) & (first_clear == cr.UNTOUCHED)).sum() > 5 and ((st[two] == cr.TOUCHED) & (first_clear == cr.UNTOUCHED)).sum() > 5
    bad = reqs[:6].copy()
    bad["chrom_id"][0], bad["strand"][1], bad["n_segs"][2], bad["read_ofs"][3] = 9, ord("x"), 3, len(bases)
    bad["seg"]["start"][4, 0], bad["seg"]["read_idx"][5, 0] = genome.length(int(bad["chrom_id"][4])) - 3, 60000
    assert list(cr.ref_check(genome, table, bad, bases)) == [cr.BAD] * 6


def _first_segment_only(reqs):
    r = reqs.copy()
    r["n_segs"] = 1
    r["seg"][:, 1] = (0, 0, 0)
    return r


@pytest.mark.parametrize("tag", M6)
def test_replay_gives_the_reference_run(genome, table, tag):
    c = CASES[tag]
    _, base = helpers.parse_sam(os.path.join(cr.DIR, f"{c.get('replay', tag)}.base.m6.sam.gz"))
    _, with5 = helpers.parse_sam(os.path.join(cr.DIR, f"{tag}.m6.sam.gz"))
    lc, stay = cr.replay(genome, table, base, bool(c.get("pe")), untrim=bool(c.get("untrim")))
    assert lc == cr.lc_records(with5, base if c.get("untrim") else None)
    assert (len(lc), len(stay)) == (c["lc"], c["stay"])
    # what stays is still aligned in the runs nothing else takes records from (-r5 has several records of a read: names do not tell them apart)
    if "replay" not in c and not c.get("untrim") and tag != "r5":
        aligned = {r["qname"] for r in with5 if not r["flag"] & 4}
        assert set(stay) <= aligned and not set(lc) & aligned


def test_the_snp_run_holds_the_records_that_stay():
    _, mine = helpers.parse_sam(os.path.join(cr.DIR, "snp.m5.sam.gz"))
    _, full = helpers.parse_sam(os.path.join(cr.DIR, "s3.m6.sam.gz"))
    assert sorted(r["qname"] for r in mine) == sorted(r["qname"] for r in full if not r["flag"] & 4)
    assert cr.golden("snp.snp.csv.gz") != cr.golden("snp.base.snp.csv.gz")


@pytest.mark.parametrize("tag", sorted(cr.spec()["errors"]))
def test_loader_refuses_with_the_reference_words(tmp_path, monkeypatch, tag):
    e = cr.spec()["errors"][tag]
    monkeypatch.chdir(tmp_path)
    if tag != "e_missing":
        helpers.gunzip_to(os.path.join(cr.DIR, e["file"] + ".gz"), e["file"])
    names, lens = (NAMES, LENS) if e["index"] == "genome" else (MANY, [120] * len(MANY))
    with pytest.raises(cr.LoadError) as err:
        cr.load_constraints(e["file"], names, lens)
    assert e["messages"][-1] == "Unable to load loci constraints" and e["exit"] == 1
    assert str(err.value) == e["messages"][-2]


def test_loader_takes_the_limits_themselves(tmp_path):
    p = str(tmp_path / "full.csv")
    with open(p, "w") as f:
        f.write("".join(f"lcA,{k},{k},A\n" for k in range(cr.MAX_LOCI)))
    assert len(cr.load_constraints(p, NAMES, LENS)) == cr.MAX_LOCI
    with open(p, "w") as f:
        f.write("".join(f"m{k:02d},5,5,A\n" for k in range(cr.MAX_CHROMS)))
    assert len(cr.load_constraints(p, MANY, [120] * len(MANY))) == cr.MAX_CHROMS
