"""microInDels (-a) and splice junctions (-A) at their edges, on CPU: the oracle's restatement of LocateInDels / LocateSpliceJuncts and
their Explore* routines against what the real reference reported for tests/golden/indeledge (tests/golden/make_golden_indel_edges.py):
flank and length limits, sequence and concatenation ends, read lengths of 30..1000, mismatch budgets, Ns, ties, anchor cores of 80..6000
copies.  For every run of cases.json every read is compared: both segments of a read reported in two ("ari" / "arj": sequence, start,
end, length, strand, mismatches) from the -M0 CSV, the not-aligned reason of every other read from the -M6 SAM, and the per-class and per-case counts."""
import gzip
import json
import os

import pytest

import helpers

with open(os.path.join(helpers.GOLDEN, "indeledge", "cases.json")) as _f:
    TAGS = sorted(json.load(_f)["cases"])


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    return helpers.indel_edge_fixture(str(tmp_path_factory.mktemp("indeledge")))


def oracle_run(sfx_path, rd, flags):
    """-> (names, hits, seg2) of the reads the run's length limits accept, the orphan filters applied"""
    kw, lo, hi = helpers.indel_edge_params(flags)
    names, bases, offs, lens = rd
    keep = helpers.filter_reads_by_len(names, bases, offs, lens, lo, hi)
    sfx = helpers.OracleSfx(sfx_path)
    if kw.get("max_ml", 0) > 1:
        hits, _, _, seg2 = helpers.oracle_align_multi_indel(sfx, bases, offs[keep], lens[keep], helpers.make_params(**kw))
    else:
        hits, seg2 = helpers.oracle_align_indel(sfx, bases, offs[keep], lens[keep], helpers.make_params(**kw))
    sfx.close()
    if kw.get("splice_junct_len"):
        helpers.remove_orphan_splices(hits, seg2)
    if kw.get("micro_indel_len"):
        helpers.remove_orphan_indels(hits, seg2)
    return [names[i] for i in keep], hits, seg2


def two_segment_rows(names, hits, seg2, chrom):
    got = {}
    for i, nm in enumerate(names):
        h = hits[i]
        if h["nar"] != 1 or not (seg2["flags"][i] & 5):
            continue
        kind = "arj" if seg2["flags"][i] & 4 else "ari"
        st, ln, s1, l1 = int(h["match_loci"]), int(h["match_len"]), int(seg2["match_loci"][i]), int(seg2["match_len"][i])
        got[nm] = [(kind, chrom[int(h["chrom_id"])], st, st + ln - 1, ln, chr(h["strand"]), int(h["mismatches"])),
                   (kind, chrom[int(h["chrom_id"])], s1, s1 + l1 - 1, l1, chr(h["strand"]), int(seg2["mismatches"][i]))]
    return got


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_matches_reference_on_indel_edges(fixture, tag):
    cases, sfx, reads = fixture
    cs = cases["cases"][tag]
    names, hits, seg2 = oracle_run(sfx[cs["genome"]], reads[cs["reads"]], cs["flags"])
    hdr, recs = helpers.parse_sam(os.path.join(helpers.GOLDEN, "indeledge", f"{tag}.m6.sam.gz"))
    chrom = {i + 1: [t[3:] for t in l.split("\t") if t.startswith("SN:")][0] for i, l in enumerate(l for l in hdr if l.startswith("@SQ"))}
    exp = {}
    for line in gzip.open(os.path.join(helpers.GOLDEN, "indeledge", f"{tag}.m0.csv.gz"), "rt"):
        f = line.rstrip("\n").split(",")
        if f[1].strip('"') in ("arj", "ari"):
            exp.setdefault(f[13].strip('"'), []).append((f[1].strip('"'), f[3].strip('"'), int(f[4]), int(f[5]), int(f[6]), f[7].strip('"'), int(f[11])))
    got = two_segment_rows(names, hits, seg2, chrom)
    assert set(got) == set(exp), sorted(set(got) ^ set(exp))[:10]
    bad = [(k, got[k], exp[k]) for k in exp if got[k] != exp[k]]
    assert not bad, bad[:5]
    # the not-aligned reason of everything else (a read aligned in one piece may have been flank-trimmed away by the reference: -A
    # switches -x on - the allowance of tests/test_oracle_splice.py, made for the runs with -A only)
    tags = {r["qname"]: r["nar"] for r in recs}
    trims = any(f.startswith("-A") for f in cs["flags"])
    assert len(tags) == len(names)
    for i, nm in enumerate(names):
        g, e = helpers.NAR_TAGS[hits["nar"][i]], tags[nm]
        assert g == e or (trims and g == "AA" and e == "ET"), (nm, hits[i], seg2[i], e)
    # per class: reads, reads in two segments, those of them at the planted place
    counts, case_counts = {}, {}
    for nm in names:
        c, case, _, ch, start, end = nm.split("|")[:6]
        for n in (counts.setdefault(c, [0, 0, 0]), case_counts.setdefault(f"{c}|{case}", [0, 0, 0])):
            n[0] += 1
            if nm in got:
                n[1] += 1
                n[2] += 1 if (got[nm][0][1], got[nm][0][2], got[nm][1][3]) == (ch, int(start), int(end)) else 0
    assert counts == cs["counts"]
    assert case_counts == cs["case_counts"]
