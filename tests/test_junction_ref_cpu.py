"""The plain-Python statement of the junction rule (tests/junction_ref.py) against lines worked by hand, and over the splice golden files:
what every other --junctions / --splice-strand test compares with must itself be right, and the golden files must hold enough of every
case for those tests to mean something."""
import os

import numpy as np
import pytest

import helpers
import junction_ref as jr
import samtags_ref as sr

#           0         1         2         3         4         5         6
#           0123456789012345678901234567890123456789012345678901234567890123456789
SEQ_ONE = "AAAAAAAAAAGTCCCCCCAGAAAAACTCCCCACAAAAAGCCCAGAAAACTCCGCAAAATCCACAAGTCAT"
SEQ_TWO = "CCCCCGTNNAGCCCCCGTAGCCCCCCCCGTAAAGCC"


@pytest.fixture(scope="module")
def genome():
    g = sr.Genome(seqs={7: ("one", SEQ_ONE), 3: ("two", SEQ_TWO)})       # (index order: "one" first, whatever the ids)
    assert list(g.codes) == [7, 3]
    return g


def line(rname, pos, cigar, flag=0, qname="r"):
    return dict(qname=qname, flag=flag, rname=rname, pos=pos, cigar=cigar)


def test_motifs_by_hand(genome):
    c = genome.codes[7]
    assert SEQ_ONE[10:12] == "GT" and SEQ_ONE[18:20] == "AG"
    assert jr.motif_of(c, 10, 20) == 1
    assert SEQ_ONE[25:27] == "CT" and SEQ_ONE[31:33] == "AC" and jr.motif_of(c, 25, 33) == 2
    assert SEQ_ONE[38:40] == "GC" and SEQ_ONE[42:44] == "AG" and jr.motif_of(c, 38, 44) == 3
    assert SEQ_ONE[48:50] == "CT" and SEQ_ONE[52:54] == "GC" and jr.motif_of(c, 48, 54) == 4
    assert SEQ_ONE[57:59] == "AT" and SEQ_ONE[61:63] == "AC" and jr.motif_of(c, 57, 63) == 5
    assert SEQ_ONE[65:67] == "GT" and SEQ_ONE[68:70] == "AT" and jr.motif_of(c, 65, 70) == 6
    assert jr.motif_of(c, 10, 19) == 0 and jr.motif_of(c, 11, 20) == 0             # one base off at either end
    assert jr.motif_of(c, 10, 44) == 1 and jr.motif_of(c, 38, 20 + 0) == 0         # GT .. the AG of another intron; end < start
    assert [chr(jr.strand_of(m)) for m in range(7)] == list(".+-+-+-")
    two = genome.codes[3]
    assert jr.motif_of(two, 5, 11) == 1                                            # GT NN AG: the n lies inside
    assert jr.motif_of(two, 6, 11) == 0 and jr.motif_of(two, 5, 10) == 0           # an n in the donor pair; in the acceptor pair
    assert SEQ_TWO[16:20] == "GTAG" and jr.motif_of(two, 16, 20) == 1              # a gap of 4 is decided by its bases
    assert jr.motif_of(two, 16, 19) == 0 and jr.motif_of(two, 17, 19) == 0 and jr.motif_of(two, 18, 19) == 0     # gaps of 3, 2, 1
    assert SEQ_TWO[28:32] == "GTAA" and jr.motif_of(two, 28, 32) == 0


def test_requests_from_lines_by_hand(genome):
    lines = [line("one", 3, "8M10N20M"),                   # start 2 + 8 = 10, end 20, overhang 8
             line("one", 1, "2S10M3S10N5M", flag=16),      # clips move nothing: start 10, end 20, overhang 5
             line("one", 6, "20M8N12M", flag=16),          # start 25, end 33
             line("one", 3, "8M"), line("one", 3, "8M3D9M"), line("one", 3, "8M2I9M"),
             line("*", 0, "30M", flag=4), line("two", 1, "5M6N9M")]
    reqs, line_of = jr.requests_of_sam(lines, genome.ids)
    assert line_of == [0, 1, 2, 7]
    assert [tuple(int(q[f]) for f in ("chrom_id", "start", "end", "overhang")) for q in reqs] == [(7, 10, 20, 8), (7, 10, 20, 5), (7, 25, 33, 12), (3, 5, 11, 5)]
    table, strands, tot = jr.junctions(reqs, genome)
    assert [tuple(int(x) for x in j) for j in table] == [(7, 10, 20, 2, 8, 1, ord("+")), (7, 25, 33, 1, 12, 2, ord("-")), (3, 5, 11, 1, 5, 1, ord("+"))]
    assert bytes(strands) == b"++-+"
    assert tot == dict(requests=4, junctions=3, flagged=0, max_reads=2, by_motif=[0, 2, 1, 0, 0, 0, 0])
    assert jr.table_text(table, genome) == "one\t11\t20\t1\t1\t0\t2\t0\t8\none\t26\t33\t2\t2\t0\t1\t0\t12\ntwo\t6\t11\t1\t1\t0\t1\t0\t5\n"
    assert jr.expected_xs(lines, genome) == ["+", "+", "-", None, None, None, None, "+"]
    assert jr.log_line(tot) == "Junctions: 4 spliced records, 3 junctions (3 GT/AG, 0 other canonical, 0 non-canonical), most reads at one junction 2"


def test_flagged_requests_and_order(genome):
    n1, n2 = len(SEQ_ONE), len(SEQ_TWO)
    good = [(3, 16, 20, 9), (7, 65, n1 - 1, 4), (7, 10, 20, 3), (7, 10, 19, 3), (7, 9, 20, 3), (3, 10, 20, 7)]
    bad = [(1, 10, 20, 5), (0, 10, 20, 5), (7, 0, 20, 5), (7, 20, 20, 5), (7, 21, 20, 5), (7, 65, n1, 5), (3, 16, n2 + 5, 5), (7, 10, 20, 0)]
    reqs = jr.make_reqs(good[:3] + bad[:4] + good[3:] + bad[4:])
    table, strands, tot = jr.junctions(reqs, genome)
    alone = jr.junctions(jr.make_reqs(good), genome)
    assert np.array_equal(table, alone[0]) and tot["flagged"] == 8 and tot["junctions"] == 6
    assert {k: v for k, v in tot.items() if k not in ("requests", "flagged")} == {k: v for k, v in alone[2].items() if k not in ("requests", "flagged")}
    assert [(int(j["chrom_id"]), int(j["start"]), int(j["end"])) for j in table] == [(7, 9, 20), (7, 10, 19), (7, 10, 20), (7, 65, n1 - 1), (3, 10, 20), (3, 16, 20)]
    assert SEQ_TWO[10:12] + SEQ_TWO[18:20] == "GCAG" and SEQ_ONE[65:67] + SEQ_ONE[67:69] == "GTCA"
    assert bytes(strands) == b"+\0+" + b"\0\0\0\0" + b"\0\0+" + b"\0\0\0\0"       # GTAG, GT..CA, GT..AG | flagged | GT..CA, AG..AG, GC..AG | flagged
    assert all(jr.is_flagged(q, genome) for q in jr.make_reqs(bad)) and not any(jr.is_flagged(q, genome) for q in jr.make_reqs(good))


@pytest.mark.parametrize("tag,spliced,n_junctions,largest,plus,minus,none", [("A5000", 153, 87, 3, 30, 49, 74), ("A500s5", 119, None, None, 27, 43, 49)])
def test_the_golden_files_hold_every_case(tag, spliced, n_junctions, largest, plus, minus, none):
    g = sr.Genome(os.path.join(helpers.GOLDEN, "splice", "genome.sfx.gz"))
    _, recs = helpers.parse_sam(os.path.join(helpers.GOLDEN, "splice", f"{tag}.m6.sam.gz"))
    reqs, line_of = jr.requests_of_sam(recs, g.ids)
    assert len(reqs) == spliced == sum(1 for r in recs if "N" in r["cigar"] and not r["flag"] & 4)
    table, strands, tot = jr.junctions(reqs, g)
    print(tot)
    assert tot["flagged"] == 0 and int(table["reads"].sum()) == spliced
    assert (int((strands == jr.PLUS).sum()), int((strands == jr.MINUS).sum()), int((strands == 0).sum())) == (plus, minus, none)
    if n_junctions is not None:
        assert (tot["junctions"], tot["max_reads"]) == (n_junctions, largest)
    # what keeps the GPU tests from passing vacuously
    assert tot["junctions"] >= 50 and tot["max_reads"] > 1 and min(plus, minus, none) >= 10
    xs = jr.expected_xs(recs, g)
    assert sum(1 for k in line_of if xs[k] and recs[k]["flag"] & 16) >= 10 and sum(1 for k in line_of if xs[k] and not recs[k]["flag"] & 16) >= 10
    keys = [(int(j["chrom_id"]), int(j["start"]), int(j["end"])) for j in table]
    assert keys == sorted(set(keys))                       # (ids are in index order in this index)
    # the table against the sequence's letters, one junction at a time
    for j in table:
        c = g.codes[int(j["chrom_id"])]
        pair = "".join(sr.LETTERS[x] for x in (c[j["start"]], c[j["start"] + 1], c[j["end"] - 2], c[j["end"] - 1]))
        assert jr.MOTIFS.get(int(j["motif"]), None) == ((pair[:2], pair[2:]) if j["motif"] else None) and (j["motif"] or (pair[:2], pair[2:]) not in jr.MOTIFS.values())
