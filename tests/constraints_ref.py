"""Shared by the loci base constraint tests (`align -5`, tests/golden/constraints): the loader of the constraints CSV with the
reference's refusals (CAligner::LoadLociConstraints, Aligner.cpp:1267-1439, over the parts of CCSVFile its files exercise), a plain
per-base restatement of the check (AcceptBaseConstraint / AcceptLociConstraints, :2480-2595), the record layouts of bk_constraints_*,
and the replay of a whole `-5` run from the SAM of the run without it."""
import gzip
import json
import os
import re

import numpy as np

import helpers
from primer_ref import LUT, Genome  # noqa: F401  (the genome as base codes by EntryID)

DIR = os.path.join(helpers.GOLDEN, "constraints")
MAX_CHROMS, MAX_LOCI = 64, 6400                      # cMaxConstrainedChroms, cMaxConstrainedLoci (Aligner.h:74-75)
UNTOUCHED, TOUCHED, VIOLATED, BAD = 0, 1, 2, 0x80
NAR_LC = 19                                          # eNARLociConstrained
# include/biokanga_amd.h: bk_constraint (16 bytes), bk_constraint_req (32 bytes)
CONSTRAINT_DTYPE = np.dtype([("chrom_id", "<u4"), ("start", "<u4"), ("end", "<u4"), ("mask", "u1"), ("_r", "u1", (3,))])
SEG_DTYPE = np.dtype([("start", "<u4"), ("len", "<u2"), ("read_idx", "<u2")])
CONSTRAINT_REQ_DTYPE = np.dtype([("read_ofs", "<u8"), ("chrom_id", "<u4"), ("read_len", "<u2"), ("strand", "u1"), ("n_segs", "u1"), ("seg", SEG_DTYPE, (2,))])
assert CONSTRAINT_DTYPE.itemsize == 16 and CONSTRAINT_REQ_DTYPE.itemsize == 32


def spec():
    with open(os.path.join(DIR, "cases.json")) as f:
        return json.load(f)


def golden(name):
    path = os.path.join(DIR, name)
    return gzip.open(path, "rb").read() if name.endswith(".gz") else open(path, "rb").read()


# ------------------------------------------------------------------------------------------------
# the CSV reader: CCSVFile::NextLine / ParseField / IsLikelyHeaderLine (CSVFile.cpp:439-771) with its defaults - ',' '"' '#'

def _parse_field(t, pos):
    """-> (value, quoted, how it ended: 0 separator | 1 end of line | 2 end of text, next position, line feeds consumed)"""
    val, quoted, state, nl = [], False, 0, 0
    while pos < len(t):
        ch = t[pos]
        pos += 1
        if state == 0:
            if ch in " \t":
                continue
            if ch == '"':
                quoted, state = True, 2
            elif ch in "\r\n":
                return "".join(val), quoted, 1, pos, int(ch == "\n")
            elif ch == ",":
                return "".join(val), quoted, 0, pos, 0
            else:
                val.append(ch)
                state = 1
        elif state == 1:
            if ch in ",\r\n":
                return "".join(val).rstrip(" \t"), quoted, 0 if ch == "," else 1, pos, int(ch == "\n")
            val.append(ch)
        elif state == 2:
            if ch == '"':
                if pos < len(t) and t[pos] == '"':
                    pos += 1
                else:
                    state = 3
                    continue
            val.append(ch)
        else:
            if ch == ",":
                return "".join(val), quoted, 0, pos, 0
            if ch in "\r\n":
                return "".join(val), quoted, 1, pos, int(ch == "\n")
    v = "".join(val)
    return (v.rstrip(" \t") if state == 1 else v), quoted, 2, pos, 0


def csv_lines(text):
    """-> [(fields [(value, quoted)], the reader's line number behind the line)]: blank lines, leading blanks and '#' comment lines skipped"""
    t = text.split("\0")[0]
    pos, line_num, in_comment, out = 0, 0, False, []
    while pos < len(t):
        ch = t[pos]
        if ch < " " and ch not in "\t\n\r":
            break
        if ch in "\r\n":
            pos += 1
            if ch == "\r" and pos < len(t) and t[pos] == "\n":
                line_num += 1
                pos += 1
            elif ch == "\n":
                line_num += 1
            in_comment = False
            continue
        if in_comment or ch in " \t":
            pos += 1
            continue
        if ch == "#":
            in_comment = True
            pos += 1
            continue
        fields = []
        while len(fields) < 100:
            v, q, how, pos, nl = _parse_field(t, pos)
            line_num += nl
            fields.append((v[:199], q))
            if how:
                break
        out.append((fields, line_num))
    return out


_STRTOD = re.compile(r"^[ \t\n\v\f\r]*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?|0[xX]([0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)([pP][+-]?\d+)?"
                     r"|[iI][nN][fF]([iI][nN][iI][tT][yY])?|[nN][aA][nN](\([0-9a-zA-Z_]*\))?)$")


def likely_header(fields):
    empty = 0
    for v, q in fields:
        if q:
            continue
        if not v:
            empty += 1
            if empty > 2:
                return False
            continue
        if _STRTOD.match(v):
            return False
    return True


def atoi(s):
    m = re.match(r"^[ \t\n\v\f\r]*([+-]?\d+)", s)
    return max(-2 ** 31, min(2 ** 31 - 1, int(m.group(1)))) if m else 0


class LoadError(Exception):
    pass


def load_constraints(path, names, lengths):
    """-> [(chrom_id, start, end, mask)] sorted by them, as LoadLociConstraints leaves its table; LoadError(message) where it refuses.
    `names` / `lengths`: the index's sequences, EntryID 1.. in order"""
    try:
        with open(path, "rb") as f:
            text = f.read().decode("latin-1")
    except OSError:
        raise LoadError(f"Unable to open '{path}' for processing")
    if len(text) < 5 or not csv_lines(text):
        raise LoadError(f"Unable to open '{path}' for processing")
    out, chroms = [], []
    for n_line, (fields, at) in enumerate(csv_lines(text)):
        if len(fields) < 4:
            raise LoadError(f"Expected at least 4 fields at line {at} in '{path}', GetCurFields() returned '{len(fields)}'")
        if n_line == 0 and likely_header(fields):
            continue
        name, start, end, bases = fields[0][0], atoi(fields[1][0]), atoi(fields[2][0]), fields[3][0]
        name = name[:80]
        cid = next((i + 1 for i, n in enumerate(names) if n.lower() == name.lower()), 0)
        if not cid:
            raise LoadError(f"Unable to find matching indexed identifier for '{name}' at line {at} in '{path}'")
        if start < 0 or start > end:
            raise LoadError(f"Start loci must be >= 0 and <= end loci for '{name}' at line {at} in '{path}'")
        if end >= lengths[cid - 1]:
            raise LoadError(f"End loci must be > targeted sequence length for '{name}' at line {at} in '{path}'")
        mask = 0
        for ch in bases:
            if ch in " \t":
                continue
            k = "ACGTR".find(ch.upper())
            if k < 0:
                raise LoadError(f"Illegal base specifiers for '{name}' at line {at} in '{path}'")
            mask |= 1 << k
        if not mask:
            raise LoadError(f"Illegal base specifiers for '{name}' at line {at} in '{path}'")
        if cid not in chroms:
            if len(chroms) == MAX_CHROMS:
                raise LoadError(f"Number of constrained chroms would be more than max ({MAX_CHROMS}) allowed for '{name}' at line {at} in '{path}'")
            chroms.append(cid)
        if len(out) == MAX_LOCI:
            raise LoadError(f"Number of constrained loci would be more than max ({MAX_LOCI}) allowed for '{name}' at line {at} in '{path}'")
        out.append((cid, start, end, mask))
    return sorted(out)


# ------------------------------------------------------------------------------------------------
# the check

def accept_base(g, table, chrom_id, loci, base):
    """AcceptBaseConstraint (:2480-2526): -1 a constraint over the locus turns the base down, 0 no constraint on the sequence, 1 accepted"""
    rslt = 0
    for c, s, e, mask in table:
        if c < chrom_id:
            continue
        if c > chrom_id:
            break
        rslt = 1
        if s <= loci <= e:
            if mask & 0x10 and int(g.codes[chrom_id][loci]) == base:
                continue
            if base < 4 and mask >> base & 1:
                continue
            return -1
    return rslt


def accept_segments(g, table, chrom_id, strand, read_codes, segs):
    """AcceptLociConstraints (:2529-2595) over segments (first locus, loci, index of the first one's base in the read as aligned): the
    read `& 7`, reverse-complemented as a whole for '-'.  -> (accepted, a constraint covered a walked locus)"""
    r = np.asarray(read_codes) & 7
    if strand == "-":
        r = np.where(r[::-1] < 4, 3 - r[::-1], r[::-1])
    touched = False
    for start, n, idx in segs:
        for j in range(n):
            touched = touched or any(c == chrom_id and s <= start + j <= e for c, s, e, _ in table)
            rs = accept_base(g, table, chrom_id, start + j, int(r[idx + j]))
            if rs != 1:
                return rs != -1, touched
    return True, touched


def ref_check(g, table, reqs, bases, per_base=False):
    """statuses of CONSTRAINT_REQ_DTYPE requests as bk_constraints_check answers them, bad ones flagged as the kernel flags them.  The
    walk of a served request: every walked locus against every constraint of its sequence at once (per_base: accept_segments instead)"""
    out = np.zeros(len(reqs), dtype=np.uint8)
    by_chrom = {}
    for row in table:
        by_chrom.setdefault(row[0], []).append(row)
    arrays = {c: tuple(np.array([r[k] for r in rows], dtype=np.int64)[:, None] for k in (1, 2, 3)) for c, rows in by_chrom.items()}
    for i, q in enumerate(reqs):
        c, ln, strand, ns, ofs = int(q["chrom_id"]), int(q["read_len"]), chr(int(q["strand"])), int(q["n_segs"]), int(q["read_ofs"])
        segs = [(int(s["start"]), int(s["len"]), int(s["read_idx"])) for s in q["seg"][:max(0, min(ns, 2))]]
        if g.length(c) == 0 or strand not in "+-" or ns not in (1, 2) or ofs + ln > len(bases) or \
                any(s + n > g.length(c) or k + n > ln for s, n, k in segs):
            out[i] = BAD
            continue
        if c not in by_chrom:
            continue
        if per_base:
            ok, touched = accept_segments(g, by_chrom[c], c, strand, bases[ofs:ofs + ln], segs)
            out[i] = VIOLATED if not ok else (TOUCHED if touched else UNTOUCHED)
            continue
        r = np.asarray(bases[ofs:ofs + ln]).astype(np.int64) & 7
        if strand == "-":
            r = np.where(r[::-1] < 4, 3 - r[::-1], r[::-1])
        loci = np.concatenate([np.arange(s, s + n) for s, n, _ in segs] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        base = np.concatenate([r[k:k + n] for _, n, k in segs] + [np.zeros(0, dtype=np.int64)])
        s_, e_, m_ = arrays[c]
        near = ((e_ >= loci.min()) & (s_ <= loci.max()))[:, 0] if len(loci) else np.zeros(len(s_), dtype=bool)
        s_, e_, m_ = s_[near], e_[near], m_[near]    # (the others cover none of these loci)
        cover = (s_ <= loci) & (loci <= e_)
        allowed = ((m_ >> np.minimum(base, 3)) & 1).astype(bool) & (base < 4)
        allowed |= ((m_ & 0x10) != 0) & (g.codes[c][loci].astype(np.int64) == base)
        out[i] = VIOLATED if (cover & ~allowed).any() else (TOUCHED if cover.any() else UNTOUCHED)
    return out


# ------------------------------------------------------------------------------------------------
# a whole run, from the SAM of the run without -5

_CIG = re.compile(r"(\d+)([MIDNS])")


def sam_segments(rec, untrim=False):
    """the walked segments of an aligned SAM record: soft clips are Seg[0]'s trims in target order - the walk indexes the read from
    ReadOfs + TrimLeft, the READ's left trim, which for '-' is the clip at the record's right end (:2572).  untrim: the clips are the
    flank trimmer's, which ran behind the pass - the record as the pass saw it"""
    ops = [(int(n), op) for n, op in _CIG.findall(rec["cigar"])]
    clip5 = ops[0][0] if ops[0][1] == "S" else 0
    clip3 = ops[-1][0] if ops[-1][1] == "S" else 0
    body = [o for o in ops if o[1] != "S"]
    pos, segs = rec["pos"] - 1, []
    if untrim:
        body[0] = (body[0][0] + clip5, "M")
        body[-1] = (body[-1][0] + clip3, "M")
        pos, clip5, clip3 = pos - clip5, 0, 0
    q = clip3 if rec["flag"] & 16 else clip5
    first = True
    for n, op in body:
        if op == "M":
            segs.append((pos, n, q if first else qpos))
            if first:
                qpos = n          # Seg[1].ReadOfs counts from the read's start, trims apart (a two-segment read carries none)
                first = False
            pos += n
        elif op in "DN":
            pos += n
        elif op == "I":
            qpos += n
    return segs


def lc_records(recs, base=None):
    """sorted qnames of the LC records of a -M6 SAM; base: only those of reads the run without -5 (its records) left aligned"""
    aligned = None if base is None else {r["qname"] for r in base if not r["flag"] & 4}
    return sorted(r["qname"] for r in recs if r["nar"] == "LC" and (aligned is None or r["qname"] in aligned))


def replay(g, table, recs, paired, untrim=False):
    """IdentifyConstraintViolations (:2599-2646) over the records of a SAM written without -5 (helpers.parse_sam, in file order = the
    sorted order) -> (sorted qnames of the records that become LC - one per record: -r5 has several of a read -, sorted qnames of the
    accepted records that touched a constraint and stay).  Paired: both ends of a pair carry its name and go together (:2623-2639)"""
    lc, stay = [], []
    for r in recs:
        if r["flag"] & 4 or r["nar"] != "AA":
            continue
        codes = LUT[np.frombuffer(r["seq"].encode(), dtype=np.uint8)]
        # (SEQ is the read as aligned: accept_segments is given it as a '+' read)
        ok, touched = accept_segments(g, table, g.ids[r["rname"]], "+", codes, sam_segments(r, untrim))
        if not ok:
            lc.append(r["qname"])
        elif touched:
            stay.append(r["qname"])
    if paired:                                       # (the fixtures' ends are named x/1 and x/2)
        gone = {n[:-2] for n in lc}
        lc = [n + e for n in gone for e in ("/1", "/2")]
        stay = [n for n in stay if n[:-2] not in gone]
    return sorted(lc), sorted(stay)


# ------------------------------------------------------------------------------------------------
# requests for bk_constraints_check

def make_requests(g, table, ids=(1, 2, 3), seed=5, n_random=2500):
    """-> (CONSTRAINT_REQ_DTYPE requests, bases).  Around every constraint, on both strands and for segments of 50, 64, 65 and 130 loci:
    ending at start - 1 and at start, beginning at end and at end + 1, with and without a trim offset; two-segment requests whose second
    segment alone lies over the constraint; random requests anywhere.  The reads follow the target, with other bases and Ns at random
    places - and at the constrained loci more often than not -, stored as loaded: reverse-complemented for '-'"""
    rng = np.random.default_rng(seed)
    rows, reads = [], []
    sites = {c: np.zeros(g.length(c), dtype=bool) for c in ids}
    for c, s, e, _ in table:
        sites[c][s:e + 1] = True

    def add(c, strand, segs, lead):
        """segs: [(start, loci)], the read: `lead` bases, the segments' bases back to back, up to 9 more"""
        ln = lead + sum(n for _, n in segs) + int(rng.integers(0, 10))
        aligned = rng.integers(0, 4, ln).astype(np.uint8)
        at, out = lead, []
        for start, n in segs:
            t = g.codes[c][start:start + n].copy()
            hot = sites[c][start:start + n]
            change = (rng.random(n) < 0.02) | (hot & (rng.random(n) < (0.5 if hot.sum() < 4 else 0.1)))
            t[change] = rng.integers(0, 5, int(change.sum()))
            aligned[at:at + n] = t
            out.append((start, n, at))
            at += n
        as_loaded = aligned if strand == "+" else np.where(aligned[::-1] < 4, 3 - aligned[::-1], aligned[::-1])
        as_loaded = as_loaded | (rng.integers(0, 32, ln).astype(np.uint8) << 3)       # the high bits of a byte are not the base's
        rows.append((c, ln, ord(strand), len(out), out + [(0, 0, 0)] * (2 - len(out))))
        reads.append(as_loaded.astype(np.uint8))

    def inside(c, start, n):
        return start >= 0 and start + n <= g.length(c)

    for c, s, e, _ in table:
        for n in (50, 64, 65, 130):
            for start in (s - n, s - n + 1, e, e + 1):
                for strand in "+-":
                    if inside(c, start, n):
                        add(c, strand, [(start, n)], 0 if (start + n) % 3 else 7)
        for strand in "+-":                          # only the second segment over it; only the first
            if inside(c, s - 400, 25) and not sites[c][s - 400:s - 375].any():
                over = min(g.length(c) - 25, max(0, s - 10))
                add(c, strand, [(s - 400, 25), (over, 25)], 0)
                add(c, strand, [(over, 25), (min(g.length(c) - 25, e + 300), 25)], 0)
    for _ in range(n_random):
        c = ids[int(rng.integers(0, len(ids)))]
        n = int(rng.choice([20, 50, 64, 65, 100, 130, 300]))
        start = int(rng.integers(0, g.length(c) - n + 1))
        if rng.random() < 0.15:
            n2 = int(rng.integers(5, 60))
            start2 = min(g.length(c) - n2, start + n + int(rng.integers(1, 500)))
            add(c, "+-"[int(rng.integers(0, 2))], [(start, n), (start2, n2)], 0)
        else:
            add(c, "+-"[int(rng.integers(0, 2))], [(start, n)], int(rng.integers(0, 12)) if rng.random() < 0.3 else 0)
    order = rng.permutation(len(rows))
    reqs = np.zeros(len(rows), dtype=CONSTRAINT_REQ_DTYPE)
    offs = np.zeros(len(rows) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    for k, i in enumerate(order):                    # (the requests do not come in the order of their reads)
        c, ln, strand, ns, segs = rows[i]
        reqs[k] = (offs[i], c, ln, strand, ns, segs)
    return reqs, np.concatenate(reads)
