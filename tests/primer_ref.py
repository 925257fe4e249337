"""Shared by the 5' primer correction tests (tests/golden/primer): the golden genome as base codes, a plain restatement of the per-read
half of CAligner::PCR5PrimerCorrect (Aligner.cpp:2052-2088: the window fetch and the two loops), the record layouts of
bk_primer_correct, and the replay of a whole `-6` run from the SAM of the run without it at the initial rate."""
import gzip
import json
import os

import numpy as np

import helpers

DIR = os.path.join(helpers.GOLDEN, "primer")
KLEN = 12
UNTOUCHED, CORRECTED, REJECTED, BAD = 0, 1, 2, 0x80
# include/biokanga_amd.h: bk_primer_req (24 bytes), bk_primer_res (16 bytes)
PRIMER_REQ_DTYPE = np.dtype([("codes", "<u8"), ("chrom_id", "<u4"), ("match_loci", "<u4"), ("match_len", "<u2"), ("strand", "u1"), ("low_mm", "u1"),
                             ("max_mms", "u1"), ("_r", "u1", (3,))])
PRIMER_RES_DTYPE = np.dtype([("codes", "<u8"), ("mask", "<u2"), ("status", "u1"), ("mismatches", "u1"), ("n_corrected", "u1"), ("_r", "u1", (3,))])
assert PRIMER_REQ_DTYPE.itemsize == 24 and PRIMER_RES_DTYPE.itemsize == 16
LUT = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate("ACGT"):
    LUT[ord(_ch)] = LUT[ord(_ch.lower())] = _i
LETTERS = "ACGTN"


def spec():
    with open(os.path.join(DIR, "cases.json")) as f:
        return json.load(f)


def cases():
    return spec()["cases"]


def golden(name):
    path = os.path.join(DIR, name)
    return gzip.open(path, "rb").read() if name.endswith(".gz") else open(path, "rb").read()


def max_mms(rate, read_len):
    return (rate * read_len + 50) // 100             # Aligner.cpp:2043


def initial_subs(s, n):
    return min(s + n, 15) if n > 0 else s            # Aligner.cpp:210-213


class Genome:
    """sequences of a FASTA in file order: what GetSeq answers for them - a0 c1 g2 t3 n4, the lower-case flag gone (the indexer clears
    it, SfxArrayV2.cpp:1235) - by EntryID (1.. unless `ids` renames them)"""

    def __init__(self, path=None, ids=None):
        names, seqs, cur = [], [], None
        for line in gzip.open(path or os.path.join(DIR, "genome.fa.gz"), "rt"):
            line = line.strip()
            if line.startswith(">"):
                names.append(line[1:].split()[0])
                cur = []
                seqs.append(cur)
            elif line:
                cur.append(line)
        self.text = ["".join(s) for s in seqs]
        ids = ids or list(range(1, len(names) + 1))
        self.names = names
        self.codes = {i: LUT[np.frombuffer(t.encode(), dtype=np.uint8)] for i, t in zip(ids, self.text)}
        self.ids = dict(zip(names, ids))

    def length(self, chrom_id):
        return len(self.codes[chrom_id]) if chrom_id in self.codes else 0


def pack_codes(c12):
    v = 0
    for k in range(KLEN):
        v |= (int(c12[k]) & 7) << (33 - 3 * k)
    return v


def unpack_codes(v):
    return [(int(v) >> (33 - 3 * k)) & 7 for k in range(KLEN)]


def window(g, chrom_id, loci, length, strand):
    """the first KLEN bases of GetSeq(chrom, loci, length), reverse-complemented as a whole for '-' (codes 0..3 complement, N stays)"""
    t = g.codes[chrom_id][loci:loci + length]
    if strand == "-":
        t = t[::-1]
        t = np.where(t < 4, 3 - t, t)
    return [int(x) for x in t[:KLEN]]


def correct(read12, tgt12, low_mm, mms):
    """the two loops: -> (status, new count, codes afterwards, corrected positions)"""
    if low_mm <= mms:
        return UNTOUCHED, low_mm, list(read12), []
    cur = low_mm
    for k in range(KLEN):
        if (read12[k] & 7) != tgt12[k]:
            cur -= 1
            if cur <= mms:
                break
    if cur > mms:
        return REJECTED, low_mm, list(read12), []
    out, fixed, cur = list(read12), [], low_mm
    for k in range(KLEN):
        if (out[k] & 7) != tgt12[k]:
            out[k] = tgt12[k]
            fixed.append(k)
            cur -= 1
            if cur <= mms:
                break
    return CORRECTED, cur, out, fixed


def ref_primer(g, reqs):
    """PRIMER_RES_DTYPE for PRIMER_REQ_DTYPE requests, bad ones flagged as the kernel flags them"""
    out = np.zeros(len(reqs), dtype=PRIMER_RES_DTYPE)
    for i, r in enumerate(reqs):
        c, loci, ln, strand = int(r["chrom_id"]), int(r["match_loci"]), int(r["match_len"]), chr(int(r["strand"]))
        codes = int(r["codes"]) & ((1 << 36) - 1)
        if g.length(c) == 0 or strand not in "+-" or ln < KLEN or loci + ln > g.length(c):
            out[i] = (codes, 0, BAD, r["low_mm"], 0, 0)
            continue
        status, cur, after, fixed = correct(unpack_codes(codes), window(g, c, loci, ln, strand), int(r["low_mm"]), int(r["max_mms"]))
        out[i] = (pack_codes(after), sum(1 << k for k in fixed), status, cur, len(fixed), 0)
    return out


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTNacgtn", "TGCANtgcan"))


def replay(g, base_recs, rate):
    """PCR5PrimerCorrect(rate) over the aligned records of a SAM written without -6 (helpers.parse_sam) -> ({qname: SEQ as the SAM of the -6
    run shows it}, set of rejected qnames, [reads corrected, bases corrected, reads rejected]).  LowMMCnt is counted from the genome: the
    records are whole-length single-segment alignments, whose count is their Hamming distance to the target"""
    seqs, rejected, counts = {}, set(), [0, 0, 0]
    for r in base_recs:
        seqs[r["qname"]] = r["seq"]
        if r["flag"] & 4:
            continue
        ln = len(r["seq"])
        assert r["cigar"] == f"{ln}M", r["raw"]
        strand = "-" if r["flag"] & 16 else "+"
        read = revcomp(r["seq"]) if strand == "-" else r["seq"]
        c, loci = g.ids[r["rname"]], r["pos"] - 1
        rc = LUT[np.frombuffer(read.encode(), dtype=np.uint8)]
        t = g.codes[c][loci:loci + ln]
        if strand == "-":
            t = np.where(t[::-1] < 4, 3 - t[::-1], t[::-1])
        low_mm = int((rc != t).sum())
        status, _, after, fixed = correct([int(x) for x in rc[:KLEN]], [int(x) for x in t[:KLEN]], low_mm, max_mms(rate, ln))
        if status == CORRECTED:
            read = "".join(LETTERS[x] for x in after) + read[KLEN:]
            seqs[r["qname"]] = revcomp(read) if strand == "-" else read
            counts[0] += 1
            counts[1] += len(fixed)
        elif status == REJECTED:
            rejected.add(r["qname"])
            seqs[r["qname"]] = read                 # (an unaligned record shows the read as loaded)
            counts[2] += 1
    return seqs, rejected, counts
