"""tests/dup_ref.py - the plain-Python statement of the duplicate marking rule - on cases whose answers are written out by hand."""
import numpy as np

import dup_ref as dr


def line(qname, flag, rname, pos, cigar):
    return dict(qname=qname, flag=flag, rname=rname, pos=pos, cigar=cigar)


def test_unclipped_5_prime_end_by_hand():
    # '+': the first M base is at 0-based 99; three clipped bases in front of it
    assert dr.end_of_line(line("a", 0, "c", 100, "3S90M7S")) == (96, dr.PLUS, 90)
    # '-': [2S] 50M [4S] 7D 40M from POS 1000: p = 999, span = 50 + 7 + 40 = 97, last M base 1095, four clipped bases behind it
    assert dr.end_of_line(line("a", 16, "c", 1000, "2S50M4S7D40M")) == (999 + 97 - 1 + 4, dr.MINUS, 90)
    # N skips its gap as D does
    assert dr.end_of_line(line("a", 16, "c", 1000, "50M4S1500N40M")) == (999 + 50 + 1500 + 40 - 1 + 4, dr.MINUS, 90)
    # I takes no target base: span = 50 + 40
    assert dr.end_of_line(line("a", 16, "c", 1000, "2S50M3I40M")) == (999 + 90 - 1, dr.MINUS, 90)
    # on '+' neither the second segment nor the right clip moves the 5' end
    assert dr.end_of_line(line("a", 0, "c", 1000, "2S50M4S7D40M")) == (997, dr.PLUS, 90)
    # a clip longer than POS - 1: negative, and legitimate
    assert dr.end_of_line(line("a", 0, "c", 3, "10S90M")) == (-8, dr.PLUS, 90)


def test_same_position_other_strand_is_no_duplicate():
    out, tot = dr.mark(dr.make_reqs([(1, 500, "+", 100), (1, 500, "-", 100), (1, 500, "+", 100)]))
    assert out.tolist() == [0, 0, 1]
    assert tot == dict(templates=3, groups=2, duplicates=1, max_group=2, flagged=0)


def test_negative_positions_and_other_sequences():
    out, tot = dr.mark(dr.make_reqs([(1, -8, "+", 90), (1, -8, "+", 95), (2, -8, "+", 90), (1, 8, "+", 90), (1, -8, "+", 95)]))
    assert out.tolist() == [1, 0, 0, 0, 1]
    assert tot == dict(templates=5, groups=3, duplicates=2, max_group=3, flagged=0)


def test_a_fragment_at_a_pairs_end_is_not_grouped_with_it():
    reqs = dr.make_reqs([(1, 100, "+", 200, 400, "-"), (1, 100, "+", 100), (1, 400, "-", 100), (1, 100, "+", 200, 0, "+")])
    out, tot = dr.mark(reqs)
    # (the last one: a pair whose other end is at 0 '+' - not the fragment at 100 '+', whose unused mate field is 0 too)
    assert out.tolist() == [0, 0, 0, 0] and tot["groups"] == 4 and tot["duplicates"] == 0


def test_a_mirrored_pair_is_grouped():
    # F1R2 and F2R1 at the same two ends
    reqs = dr.make_reqs([(1, 100, "+", 200, 400, "-"), (1, 400, "-", 200, 100, "+"), (1, 400, "+", 200, 100, "-")])
    out, tot = dr.mark(reqs)
    assert out.tolist() == [0, 1, 0]
    assert dr.key_of(reqs[0]) == dr.key_of(reqs[1]) == (1, (100, False), (400, True))
    assert dr.key_of(reqs[2]) == (1, (100, True), (400, False))
    # equal positions: '+' sorts in front of '-'
    assert dr.key_of(dr.make_reqs([(1, 7, "-", 1, 7, "+")])[0]) == (1, (7, False), (7, True))
    assert tot == dict(templates=3, groups=2, duplicates=1, max_group=2, flagged=0)


def test_score_beats_order_and_order_breaks_ties():
    assert dr.mark(dr.make_reqs([(1, 5, "+", 90), (1, 5, "+", 100), (1, 5, "+", 95)]))[0].tolist() == [1, 0, 1]
    assert dr.mark(dr.make_reqs([(1, 5, "+", 100), (1, 5, "+", 90), (1, 5, "+", 100)]))[0].tolist() == [0, 1, 1]
    assert dr.mark(dr.make_reqs([(1, 5, "-", 7)] * 4))[0].tolist() == [0, 1, 1, 1]


def test_flagged_requests_take_part_in_nothing():
    reqs = dr.make_reqs([(1, 5, "+", 90), (9, 5, "+", 99), (1, 5, "?", 99), (1, 5, "+", 99, 5, "x"), (1, 5, "+", 80), (0, 5, "+", 1)])
    out, tot = dr.mark(reqs, chroms={1, 2, 3})
    assert out.tolist() == [0, 2, 2, 2, 1, 2]
    assert tot == dict(templates=6, groups=1, duplicates=1, max_group=2, flagged=4)
    assert dr.mark(reqs[:0])[1] == dict(templates=0, groups=0, duplicates=0, max_group=0, flagged=0)


def test_templates_and_flags_of_sam_lines():
    load = {n: k for k, n in enumerate(["p0/1", "p0/2", "p1/1", "p1/2", "p2/1", "p2/2", "p3/1", "p3/2"])}
    lines = [
        line("p1/2", 0x1 | 0x2 | 0x80 | 0x20, "c", 100, "100M"),                # pair p1, F2R1: '+' end at 99, '-' end at 300 + 98 - 1 + 2 = 399
        line("p0/1", 0x1 | 0x2 | 0x40 | 0x20, "c", 100, "3S97M"),               # pair p0: its '+' end is 99 - 3 = 96: nobody's duplicate
        line("p3/1", 0x1 | 0x2 | 0x40 | 0x20 | 0x400, "c", 100, "100M"),        # p3: as p1, PE1 and PE2 swapped; a stale 0x400 is masked off
        line("p2/1", 0x1 | 0x2 | 0x40 | 0x8, "c", 100, "100M"),                 # an orphan end: a fragment at a pair's end
        line("p2/2", 0x1 | 0x2 | 0x80 | 0x4, "*", 0, "100M"),                   # .. whose mate is not aligned
        line("p0/2", 0x1 | 0x2 | 0x80 | 0x10, "c", 301, "100M"),
        line("p1/1", 0x1 | 0x2 | 0x40 | 0x10, "c", 301, "98M2S"),
        line("p3/2", 0x1 | 0x2 | 0x80 | 0x10, "c", 303, "98M"),
    ]
    reqs, members = dr.requests_of_sam(lines, load)
    assert members == [[1, 5], [6, 0], [3], [2, 7]]
    assert reqs.tolist() == dr.make_reqs([(1, 96, "+", 197, 399, "-"), (1, 399, "-", 198, 99, "+"), (1, 99, "+", 100), (1, 99, "+", 198, 399, "-")]).tolist()
    assert dr.key_of(reqs[1]) == dr.key_of(reqs[3]) == (1, (99, False), (399, True))
    # p1 and p3 share both ends and score 198 each: p1 was loaded first
    flags = dr.expected_flags(lines, load)
    assert [f & 0x400 for f in flags] == [0, 0, 0x400, 0, 0, 0, 0, 0x400]
    assert [f & ~0x400 for f in flags] == [r["flag"] & ~0x400 for r in lines]
    # one M base less on p1: p3 stays
    lines[0]["cigar"] = "99M1S"
    assert [f & 0x400 for f in dr.expected_flags(lines, load)] == [0x400, 0, 0, 0, 0, 0, 0x400, 0]
