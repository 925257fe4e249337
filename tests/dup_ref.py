"""Shared by the --mark-duplicates tests: the rule of bk_mark_duplicates (include/biokanga_amd.h) in plain Python.

    A request is one TEMPLATE: a fragment (chrom, pos5, strand; strand_mate 0) or a pair (both ends).  A pair's ends are put into
    canonical order - (pos5_a, strand_a) <= (pos5_b, strand_b), '+' < '-' - so which end came first is no part of the key; pairs and
    fragments never share a group.  Within a group of equal keys the template with the highest score is kept, the earlier request
    among equal scores; every other one is a duplicate.  A request is FLAGGED - and takes part in no group - when its sequence does
    not exist, its strand is not '+' / '-' or its strand_mate is none of 0, '+', '-'.

    The unclipped 5' position of a SAM line [cL S] m M [cR S] [gap N|I|D m2 M] at POS: p = POS - 1, span = m + (N or D: gap) + m2;
    '+': p - cL; '-': p + span - 1 + cR.  Score of a line: m + m2.

A dict over canonical keys, max by (score, -index).  Also: the templates of the accepted lines of a SAM file, and the FLAGs they get."""
import re

import numpy as np

# include/biokanga_amd.h: bk_dup_req (16 bytes)
DUP_REQ_DTYPE = np.dtype([("chrom_id", "<u4"), ("pos5", "<i4"), ("pos5_mate", "<i4"), ("strand", "u1"), ("strand_mate", "u1"), ("score", "<u2")])
assert DUP_REQ_DTYPE.itemsize == 16
KEPT, DUPLICATE, FLAGGED = 0, 1, 2
PLUS, MINUS = ord("+"), ord("-")
_SHAPE = re.compile(r"^(?:(\d+)S)?(\d+)M(?:(\d+)S)?(?:(\d+)([NID])(\d+)M)?$")


def make_reqs(rows):
    """[(chrom_id, pos5, strand, score[, pos5_mate, strand_mate])], strands as '+' / '-' or numbers -> request array"""
    out = np.zeros(len(rows), dtype=DUP_REQ_DTYPE)
    code = lambda s: ord(s) if isinstance(s, str) else int(s)
    for k, r in enumerate(rows):
        out[k]["chrom_id"], out[k]["pos5"], out[k]["strand"], out[k]["score"] = r[0], r[1], code(r[2]), r[3]
        if len(r) > 4:
            out[k]["pos5_mate"], out[k]["strand_mate"] = r[4], code(r[5])
    return out


def key_of(q):
    """the canonical key of one request, or None when it is flagged for its strands"""
    st, sm = int(q["strand"]), int(q["strand_mate"])
    if st not in (PLUS, MINUS) or sm not in (0, PLUS, MINUS):
        return None
    a = (int(q["pos5"]), st == MINUS)
    if sm == 0:
        return (int(q["chrom_id"]), a)
    b = (int(q["pos5_mate"]), sm == MINUS)
    return (int(q["chrom_id"]),) + tuple(sorted([a, b]))


def mark(reqs, chroms=None):
    """chroms: the sequence ids that exist (None: every id does) -> (a byte per request, totals as bk_dup_totals has them)"""
    out = np.zeros(len(reqs), dtype=np.uint8)
    best, count = {}, {}
    for i, q in enumerate(reqs):
        k = key_of(q)
        if k is None or (chroms is not None and int(q["chrom_id"]) not in chroms):
            out[i] = FLAGGED
            continue
        cand = (int(q["score"]), -i)
        if k not in best or cand > best[k]:
            best[k] = cand
        count[k] = count.get(k, 0) + 1
        out[i] = DUPLICATE
    for k, (_, neg) in best.items():
        out[-neg] = KEPT
    flagged = int((out == FLAGGED).sum())
    return out, dict(templates=len(reqs), groups=len(best), duplicates=len(reqs) - flagged - len(best), max_group=max(count.values(), default=0), flagged=flagged)


def end_of_line(rec):
    """a record of helpers.parse_sam -> (pos5, strand, M bases) of its line"""
    m = _SHAPE.match(rec["cigar"])
    assert m is not None, rec["cigar"]
    c_left, m1, c_right = int(m.group(1) or 0), int(m.group(2)), int(m.group(3) or 0)
    span, m2 = m1, 0
    if m.group(5):
        m2 = int(m.group(6))
        span += m2 + (int(m.group(4)) if m.group(5) in "ND" else 0)
    p = rec["pos"] - 1
    minus = bool(rec["flag"] & 16)
    return (p + span - 1 + c_right if minus else p - c_left), (MINUS if minus else PLUS), m1 + m2


def requests_of_sam(lines, load_order, ids=None):
    """The templates of the accepted lines (records of helpers.parse_sam), rebuilt from the lines alone: RNAME, POS, CIGAR, FLAG (0x400
    masked off) and QNAME -> load number (load_order: {qname: number of the read in load order; mates of a pair are 2 p and 2 p + 1}).
    A pair: both mates' lines have FLAG & 1 set and FLAG & 4 and FLAG & 8 clear.  ids: {sequence name: chrom_id} (None: numbered by name).
    -> (requests in load order of their first read, for each the indexes of its lines)"""
    if ids is None:
        ids = {n: k + 1 for k, n in enumerate(sorted({r["rname"] for r in lines if not r["flag"] & 4}))}
    by_load = {}
    for k, r in enumerate(lines):
        if r["flag"] & 4:
            continue
        assert load_order[r["qname"]] not in by_load, "one line per read"
        by_load[load_order[r["qname"]]] = k
    paired = lambda k: (lines[k]["flag"] & 1) and not (lines[k]["flag"] & 8)
    rows, members = [], []
    for ld in sorted(by_load):
        k = by_load[ld]
        pos5, strand, score = end_of_line(lines[k])
        mate = by_load.get(ld ^ 1)
        if paired(k) and mate is not None and paired(mate):
            if ld & 1:
                continue                    # (made with its first end)
            p2, s2, sc2 = end_of_line(lines[mate])
            assert lines[mate]["rname"] == lines[k]["rname"]
            rows.append((ids[lines[k]["rname"]], pos5, strand, score + sc2, p2, s2))
            members.append([k, mate])
        else:
            rows.append((ids[lines[k]["rname"]], pos5, strand, score))
            members.append([k])
    return make_reqs(rows), members


def expected_flags(lines, load_order):
    """-> the FLAG every line must carry: its own with 0x400 masked off, 0x400 added on the lines of duplicate templates"""
    reqs, members = requests_of_sam(lines, load_order)
    out, _ = mark(reqs)
    assert not (out == FLAGGED).any()
    flags = [r["flag"] & ~0x400 for r in lines]
    for t, ks in enumerate(members):
        if out[t] == DUPLICATE:
            for k in ks:
                flags[k] |= 0x400
    return flags
