"""Pins the oracle's paired-end restatement on the edges of the pair rules and of the orphan recovery against the real reference
(tests/golden/peedge, written by tests/golden/make_golden_peedge.py): inserts exactly at -d / -D and one beside them, unique mates placed
every few bases over the range where AlignPairedRead gives up or clamps its window at locus 0, partners unaligned as ML, NL and EN or
uniquely aligned beside near copies, -E, the widest offset scan and the narrowest window that goes through core lookups, and -Z / -z from both sides in
every -U mode."""
import os

import numpy as np
import pytest

import helpers
from test_oracle_pe import check_pe_hits_against_sam, filt_by_chroms

DIR = os.path.join(helpers.GOLDEN, "peedge")
CHROMS = ["peA", "peB", "peC"]
CHROM_LENS = {"peA": 7000, "peB": 6500, "peC": 6000}
# safe: the run holds the pairs of core_safe() only (make_golden_peedge.py: the reference does not return from the others)
RUNS = {"U1": dict(pe=1), "U2": dict(pe=2), "U3": dict(pe=3), "U4": dict(pe=4), "U3E": dict(pe=3, E=True), "U3D1149": dict(pe=3, d=150, D=1149),
        "U3D1150": dict(pe=3, d=150, D=1150, safe=True)}
RUNS.update({f"U{u}ZpeA": dict(pe=u, Z=["peA"]) for u in (1, 2, 3, 4)})
RUNS.update({f"U{u}zpeA": dict(pe=u, z=["peA"]) for u in (1, 2, 3, 4)})


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("peedge")
    return {n: helpers.gunzip_to(os.path.join(DIR, n + ".gz"), str(d / n)) for n in ("genome.sfx", "reads_1.fa", "reads_2.fa")}


@pytest.fixture(scope="module")
def reads(files):
    return helpers.interleave_pe(files["reads_1.fa"], files["reads_2.fa"])


def core_safe(name):
    t = name.split("/")[0].split("_")
    return not (t[1].startswith("oR") and int(t[4]) == CHROM_LENS[t[2]] - 100)


def run_reads(reads, cfg):
    """the reads of a run: all of them, or the pairs of core_safe()"""
    if not cfg.get("safe"):
        return reads
    names, bases, offs, lens = reads
    keep = [i for i in range(len(names)) if core_safe(names[i])]
    assert 0 < len(names) - len(keep) < 400 and len(keep) % 2 == 0
    return [names[i] for i in keep], bases, offs[keep], lens[keep]


@pytest.fixture(scope="module")
def se_hits(files, reads):
    """the oracle's single-end records, of all pairs (False) and of the pairs of core_safe() (True)"""
    out = {}
    o = helpers.OracleSfx(files["genome.sfx"])
    for safe in (False, True):
        names, bases, offs, lens = run_reads(reads, dict(safe=safe))
        hits, _ = o.align(bases, offs, lens, helpers.make_params(max_subs=5), nthreads=8)
        hits.setflags(write=False)
        out[safe] = hits
    o.close()
    return out


def oracle_run(sfx_path, reads, se_by, cfg):
    """-> (records as ProcessPairedEnds leaves them, the same after FiltByChroms)"""
    names, bases, offs, lens = run_reads(reads, cfg)
    se = se_by[bool(cfg.get("safe"))]
    o = helpers.OracleSfx(sfx_path)
    accept = None
    if "Z" in cfg or "z" in cfg:
        accept = helpers.chrom_accept_table(CHROMS, exclude=cfg.get("Z", ()), include=cfg.get("z", ()))
    hits = se.copy()
    helpers.oracle_process_pe(o, helpers.make_params(max_subs=5), cfg["pe"], cfg.get("d", 200), cfg.get("D", 400), cfg.get("E", False),
                              bases, offs, lens, hits, accept=accept)
    o.close()
    final = hits.copy()
    if accept is not None:
        filt_by_chroms(final, CHROMS, cfg.get("Z", ()), cfg.get("z", ()))
    return hits, final


def check_nar_summary(final, tag):
    exp = {}
    with open(os.path.join(DIR, f"{tag}.nar.txt")) as f:
        for line in f:
            t = line.split()
            exp[t[1].strip("()")] = int(t[0])
    got = np.bincount(final["nar"], minlength=20)
    for k, tg in enumerate(helpers.NAR_TAGS):
        assert got[k] == exp[tg], (tag, tg, got[k], exp[tg])


def test_fixture_holds_the_planted_kinds(reads, se_hits):
    names = reads[0]
    kinds = {}
    for i in range(0, len(names), 2):
        k = names[i].split("_")[1].split("/")[0]
        kinds[k] = kinds.get(k, 0) + 1
    for ins in (199, 200, 201, 399, 400, 401):
        for o in ("fr", "rf", "ff", "rr"):
            assert kinds.get(f"ins{ins}{o}", 0) >= 3, (ins, o)
    for end in "RL":
        for route in ("ml", "nl", "en", "nc"):
            for a in "12":
                assert kinds.get(f"o{end}{route}{a}", 0) >= 20, (end, route, a)
    # the partners are unaligned by the routes they were planted for
    # (nc: one exact placement, two others one substitution away - accepted as unique)
    for route, nar in (("ml", 5), ("nl", 3), ("en", 2), ("nc", 1)):
        idx = [i + (1 if f"{route}1" in names[i] else 0) for i in range(0, len(names), 2) if names[i].split("_")[1][2:4] == route]
        got = se_hits[False]["nar"][idx]
        assert len(idx) >= 80 and np.all(got == nar), (route, np.bincount(got))


@pytest.mark.parametrize("tag", sorted(RUNS))
def test_oracle_pe_edges_match_reference(files, reads, se_hits, tag):
    hits, final = oracle_run(files["genome.sfx"], reads, se_hits, RUNS[tag])
    check_pe_hits_against_sam(run_reads(reads, RUNS[tag])[0], final, tag, CHROMS, "peedge")
    check_nar_summary(final, tag)
    if tag == "U3D1150":                                                     # core lookups recover at both ends of the sequences
        rec = [n for n, h, s in zip(run_reads(reads, RUNS[tag])[0], final, se_hits[True]) if h["nar"] == 1 and s["nar"] == 5]
        assert sum("_oR" in n for n in rec) >= 50 and sum("_oL" in n for n in rec) >= 50, len(rec)
