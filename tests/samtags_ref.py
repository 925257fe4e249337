"""Shared by the --sam-tags tests: NM:i and MD:Z as a literal walk of a SAM line as written, in plain Python, against the sequence AS
INDEXED (the bases of the .sfx, not the FASTA: `biokanga index` turns every 13th N of a long N run into a random base).

    POS, CIGAR and SEQ of the line (SEQ already reverse complemented for a '-' record); S and I consume SEQ only, N and D the target
    only, M both, base by base.  An M base matches when SEQ's letter equals the target's and is one of ACGT.
    NM = mismatching M bases + all I bases + all D bases.
    MD = [0-9]+(([A-Z]|\\^[A-Z]+)[0-9]+)*: run lengths always written, a mismatch writes the target's letter, D writes ^ and the
    deleted target letters, N / I / S write nothing and a match run continues across them.
    No tags (None): a number <= 0, a walk that does not consume exactly SEQ, a walk that leaves its sequence.

Also: the request records of bk_samtags for lines of the one shape the writers make, and helpers to take the tags off a line."""
import gzip
import re
import struct

import numpy as np

LETTERS = "ACGTN"
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
NONE = 0xFFFF
# include/biokanga_amd.h: bk_samtag_req (32 bytes)
SAMTAG_REQ_DTYPE = np.dtype([("read_ofs", "<u8"), ("chrom_id", "<u4"), ("pos", "<u4"), ("read_len", "<u2"), ("strand", "u1"), ("gop", "u1"),
                             ("c5", "<u2"), ("m", "<u2"), ("c3", "<u2"), ("m2", "<u2"), ("gap", "<i4")])
assert SAMTAG_REQ_DTYPE.itemsize == 32
_OP = re.compile(r"(-?\d+)([MIDNS])")
_SHAPE = re.compile(r"^(?:(\d+)S)?(\d+)M(?:(\d+)S)?(?:(-?\d+)([NID])(\d+)M)?$")
_MD = re.compile(r"^[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*$")


class Genome:
    """the sequences of an index as GetSeq answers them - a0 c1 g2 t3 n4, the lower-case flag gone - by EntryID; from a .sfx (plain or
    gzip'd: header 1224 B, block header 20 B + bases, entries 8 B + 111 B each) or from {id: (name, "ACGTN..." text)}"""

    def __init__(self, sfx=None, seqs=None):
        self.codes, self.ids, self.names = {}, {}, {}
        if seqs is not None:
            for i, (name, text) in seqs.items():
                self._add(i, name, np.array([CODE.get(c, 4) for c in text.upper()], dtype=np.uint8))
            return
        raw = (gzip.open if sfx.endswith(".gz") else open)(sfx, "rb").read()
        ent_ofs, = struct.unpack_from("<Q", raw, 20)
        blk_ofs, = struct.unpack_from("<Q", raw, 44)
        _, _, n, _ = struct.unpack_from("<IIQI", raw, blk_ofs)
        seq = np.frombuffer(raw, dtype=np.uint8, count=n, offset=blk_ofs + 20)
        n_ent, = struct.unpack_from("<I", raw, ent_ofs)
        for k in range(n_ent):
            at = ent_ofs + 8 + 111 * k
            eid, = struct.unpack_from("<I", raw, at)
            name = raw[at + 8:at + 89].split(b"\0")[0].decode()
            _, slen, start, end = struct.unpack_from("<HIQQ", raw, at + 89)
            assert end - start + 1 == slen
            self._add(eid, name, np.minimum(seq[start:end + 1] & 7, 4).astype(np.uint8))

    def _add(self, i, name, codes):
        self.codes[i], self.ids[name], self.names[i] = codes, i, name

    def length(self, chrom_id):
        return len(self.codes[chrom_id]) if chrom_id in self.codes else 0


def parse_cigar(cigar):
    """[(n, op)] in the order written, or None when the text is not a list of <number><MIDNS>"""
    ops, at = [], 0
    for m in _OP.finditer(cigar):
        if m.start() != at:
            return None
        ops.append((int(m.group(1)), m.group(2)))
        at = m.end()
    return ops if ops and at == len(cigar) else None


def walk(pos0, cigar, seq, target):
    """(NM, MD) of a line with 0-based POS `pos0` against the codes of its sequence, or None"""
    ops = parse_cigar(cigar)
    if ops is None or target is None or pos0 < 0 or any(n <= 0 for n, _ in ops):
        return None
    si, ti, nm, run, md = 0, pos0, 0, 0, []
    for n, op in ops:
        if op in "SI":
            si += n
            nm += n if op == "I" else 0
        elif op == "N":
            ti += n
        elif op == "D":
            if ti + n > len(target):
                return None
            md.append(f"{run}^" + "".join(LETTERS[c] for c in target[ti:ti + n]))
            run, ti, nm = 0, ti + n, nm + n
        else:
            if si + n > len(seq) or ti + n > len(target):
                return None
            for k in range(n):
                a, b = seq[si + k], LETTERS[target[ti + k]]
                if a == b and a in "ACGT":
                    run += 1
                else:
                    md.append(f"{run}{b}")
                    run, nm = 0, nm + 1
            si, ti = si + n, ti + n
    if si != len(seq) or ti > len(target):
        return None
    md.append(str(run))
    out = "".join(md)
    assert _MD.match(out), out
    return nm, out


def line_fields(line):
    """a SAM line (text) or a record of helpers.parse_sam -> (flag, rname, pos, cigar, seq)"""
    if isinstance(line, dict):
        return line["flag"], line["rname"], line["pos"], line["cigar"], line["seq"]
    t = line.rstrip("\n").split("\t")
    return int(t[1]), t[2], int(t[3]), t[5], t[9]


def ref_tags(line, genome):
    """(NM, MD) of an aligned SAM line, None when it gets no tags (unaligned lines included)"""
    flag, rname, pos, cigar, seq = line_fields(line)
    if flag & 4 or rname not in genome.ids:
        return None
    return walk(pos - 1, cigar, seq, genome.codes[genome.ids[rname]])


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def read_codes(seq):
    return np.array([CODE.get(c, 4) for c in seq], dtype=np.uint8)


def request(line, genome, read_ofs):
    """the bk_samtag_req of an aligned line whose CIGAR has the writers' shape [c5 S] m M [c3 S] [gap N|I|D m2 M] (else None), and the
    read as loaded (SEQ turned back for '-') as base codes"""
    flag, rname, pos, cigar, seq = line_fields(line)
    m = _SHAPE.match(cigar)
    if flag & 4 or m is None:
        return None
    r = np.zeros(1, dtype=SAMTAG_REQ_DTYPE)[0]
    r["read_ofs"], r["chrom_id"], r["pos"], r["read_len"] = read_ofs, genome.ids.get(rname, 0), pos - 1, len(seq)
    r["strand"] = ord("-" if flag & 16 else "+")
    r["c5"], r["m"], r["c3"] = int(m.group(1) or 0), int(m.group(2)), int(m.group(3) or 0)
    if m.group(5):
        r["gap"], r["gop"], r["m2"] = int(m.group(4)), ord(m.group(5)), int(m.group(6))
    return r, read_codes(revcomp(seq) if flag & 16 else seq)


def split_tags(line):
    """a SAM line as bytes or text -> (the line without NM / MD, NM or None, MD or None)"""
    text = line.decode() if isinstance(line, bytes) else line
    t = text.split("\t")
    nm = md = None
    keep = []
    for k, f in enumerate(t):
        if k >= 11 and f.startswith("NM:i:"):
            nm = int(f[5:])
        elif k >= 11 and f.startswith("MD:Z:"):
            md = f[5:]
        else:
            keep.append(f)
    out = "\t".join(keep)
    return (out.encode() if isinstance(line, bytes) else out), nm, md


def strip_body(text):
    """a SAM body (bytes, header lines allowed) -> (the same without NM / MD, [(NM, MD)] per non-header line)"""
    lines, tags = [], []
    for ln in text.split(b"\n"):
        if ln.startswith(b"@") or not ln:
            lines.append(ln)
            continue
        bare, nm, md = split_tags(ln)
        lines.append(bare)
        tags.append((nm, md))
    return b"\n".join(lines), tags
