"""The restatement of CAligner::PCR5PrimerCorrect (primer_ref.py) against the reference binary's own output: every `-M6` case of
tests/golden/primer is replayed from the SAM of the run WITHOUT -6 at the initial rate plus the genome, and must give the SEQ of every
record of the -6 run, its rejected reads and the three counts of its log line.  No GPU: this pins the yardstick the GPU tests use."""
import os

import pytest

import helpers
import primer_ref as pr

M6 = sorted(t for t, c in pr.cases().items() if c.get("m6", True))


@pytest.fixture(scope="module")
def genome():
    return pr.Genome()


def _rates(flags):
    s = next(int(f[2:]) for f in flags if f.startswith("-s"))
    n = int(flags[flags.index("-6") + 1])
    return s, n


def test_the_cases_cover_what_they_are_for():
    cs = pr.cases()
    assert set(cs) >= {"s2p3", "s2p5", "s12p5", "s0p2", "s2p3x3", "s2p3k", "s2p3Q1", "s2p3snp", "U3", "U2", "r3"}
    for tag, c in cs.items():
        assert c["counts"][0] > 0 and c["counts"][1] >= c["counts"][0] and c["counts"][2] > 0, tag
    # -6 5 reaches reads -6 3 does not; the cap: -s12 -6 5 aligns at 15, not 17
    assert cs["s2p5"]["counts"] != cs["s2p3"]["counts"]
    assert pr.spec()["bases"][cs["s12p5"]["base"]] == ["-s15"]
    assert len(cs["U3"]["orphans_differ"]) >= 12 and cs["U2"]["orphans_differ"] == []


def test_initial_rate_and_max_mms():
    assert [pr.initial_subs(s, n) for s, n in ((2, 3), (12, 5), (15, 1), (0, 2), (7, 0))] == [5, 15, 15, 2, 7]
    assert [pr.max_mms(2, ln) for ln in (24, 25, 50, 74, 75, 100)] == [0, 1, 1, 1, 2, 2]
    assert pr.max_mms(0, 100) == 0


def test_the_loops_on_hand_made_windows():
    t = [0, 1, 2, 3] * 3
    r = list(t)
    r[2], r[5], r[9] = 3, 0, 2                       # three 5' mismatches
    # five in all, two allowed: all three go
    assert pr.correct(r, t, 5, 2) == (pr.CORRECTED, 2, t, [2, 5, 9])
    # four in all: the count is there at the second, the third stays
    st, cur, after, fixed = pr.correct(r, t, 4, 2)
    assert (st, cur, fixed) == (pr.CORRECTED, 2, [2, 5]) and after[9] == 2 and after[:9] == t[:9]
    # six in all: one short
    assert pr.correct(r, t, 6, 2) == (pr.REJECTED, 6, r, [])
    assert pr.correct(r, t, 2, 2) == (pr.UNTOUCHED, 2, r, [])
    # a read N never equals a base and takes it; a target N goes into the read; N on N is no mismatch
    rn, tn = list(t), list(t)
    rn[0], tn[1], rn[4], tn[4] = 4, 4, 4, 4
    st, cur, after, fixed = pr.correct(rn, tn, 3, 0)
    assert (st, cur, fixed) == (pr.REJECTED, 3, [])
    st, cur, after, fixed = pr.correct(rn, tn, 2, 0)
    assert (st, cur, fixed, after[0], after[1], after[4]) == (pr.CORRECTED, 0, [0, 1], 0, 4, 4)


@pytest.mark.parametrize("tag", M6)
def test_replay_gives_the_reference_run(genome, tag):
    c = pr.cases()[tag]
    s, n = _rates(c["flags"])
    assert pr.spec()["bases"][c["base"]][[f[:2] for f in pr.spec()["bases"][c["base"]]].index("-s")] == f"-s{pr.initial_subs(s, n)}"
    _, base = helpers.parse_sam(os.path.join(pr.DIR, f"{c['base']}.m6.sam.gz"))
    _, with6 = helpers.parse_sam(os.path.join(pr.DIR, f"{tag}.m6.sam.gz"))
    assert len(base) == len(with6)
    got = {r["qname"]: r for r in with6}
    # paired ends: the orphan recovery of the -6 run looks for cores of the user's rate, the run at the initial rate for shorter ones -
    # the mates only that one recovers never reach the correction pass (the generator planted and checked them)
    skip = set(c.get("orphans_differ", []))
    for q in skip:
        assert got[q]["flag"] & 4 and got[q]["nar"] != "NL"
    base = [r for r in base if r["qname"] not in skip]
    seqs, rejected, counts = pr.replay(genome, base, s)
    assert counts == c["counts"]
    was_aligned = {r["qname"] for r in base if not r["flag"] & 4}
    now_nl = {q for q in was_aligned if got[q]["nar"] == "NL"}
    assert now_nl == rejected
    for r in base:
        g = got[r["qname"]]
        want = seqs[r["qname"]]
        if not r["flag"] & 4 and g["flag"] & 4:       # left the set behind the pass (-k, -x, the pass itself): the read as loaded, corrected or not
            fwd = pr.revcomp(want) if r["flag"] & 16 else want
            assert g["seq"] in (want, fwd), r["qname"]
        else:
            assert g["seq"] == want, r["qname"]
    # corrected reads stay aligned where they were (-x moves the written start)
    trimmed = any(f.startswith("-x") for f in c["flags"])
    kept = [r for r in base if r["qname"] in was_aligned - rejected and not got[r["qname"]]["flag"] & 4]
    assert all((got[r["qname"]]["rname"], got[r["qname"]]["flag"] & 16) == (r["rname"], r["flag"] & 16) for r in kept)
    assert trimmed or all(got[r["qname"]]["pos"] == r["pos"] for r in kept)
