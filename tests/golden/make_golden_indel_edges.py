#!/usr/bin/env python3
"""Generates tests/golden/indeledge/: edge cases of `biokanga align -a <n>` / `-A <n>` (CSfxArrayV3::LocateInDels, LocateSpliceJuncts and
their Explore* routines), by RUNNING THE REAL REFERENCE executable (oracle/_ref/biokanga, built by oracle/build_ref.sh).  Run in the build
container only; everything written is data.

    python tests/golden/make_golden_indel_edges.py

Genome (seeded), eight sequences, some 154 000 bases in all (below 500 000: the shortest cores, 6 bases):
  eA   3 000   the first sequence: placements at loci 0..20, the start of the concatenation
  eP   8 000   plain random bases: flank limits, length limits, read lengths, mismatch budgets
  eB   4 000   single Ns and one run of three (far below the length at which the indexer rewrites a run)
  eL 108 000   5 000 unique bases, then 5 150 copies of one 16-mer 2..3 bases apart (their first base C or G), then unique bases again:
               introns of up to 100 001 bases span the copies, and the 16-mer is an anchor core of more members than MaxIter (5 000)
  eF  11 300   80 copies of one 25-mer and 150 of another, 4..8 bases apart (first base C or G), and single copies of the three repeated
               cores in unique surroundings, followed by an A (first in suffix-array order among the copies) or a T (last)
  eS  16 000   junction ties: one donor with two acceptors at different distances, with and without GT..AG / CT..AC
  eT   3 000   microInDel ties: a segment present twice, exactly and with one substitution, and a dinucleotide run in which an insertion
               and a deletion of one base score the same
  eE   2 500   the last sequence: placements ending on the last base of the concatenation; 500 bases of eA are repeated in it
reads_repeat.fa.gz holds reads for the tests/golden/repeat genome (loaded from there, not copied): 51-base reads whose 25-base anchor core is
one of that genome's 25-mers of 2 000..6 000 copies, taken at the copies that lie in unique surroundings (chrU); the suffix-array rank of the
true placement among the copies goes into the read's name.

Reads: every planted read is written twice (/a, /b) so that the orphan filters (a junction or microInDel must be seen in two reads) let it
stand.  Names carry the kind (ins / del / jct / none) and the planted placement, start = first base of the first segment
and end = last base of the second in the sequence (-1: nothing planted).  Both survive any sliding of the gap along equal bases.  The
classes and what each is designed for are listed in CLASSES below; cases.json records, per run and class, the reads, those the reference
reported with two segments, and those of them at the planted place.

Every run is made three times: -T1, -T4 and -T4 on the read file in reversed order; the generator stops if a read's records differ.
Classes dropped because the reference's answer was not repeatable: none.

Names are class|case|kind|sequence|start|end|strand|serial/copy.  Two classes hold what is designed to be refused (no read of them is
reported with two segments in any run): beyond_limit (a gap is planted, a limit forbids it) and no_gap (nothing to find); every other
class is found at the planted place in some run.  What the reference does otherwise than first designed, kept and recorded:
  * an insertion is found with 7 bases behind it, a deletion needs 8, and a deletion 8 bases from the read's 5' end is refused (flank);
  * `-A n` places introns of up to n - 41 bases before a 40-base second segment and n - 51 behind a 40-base first one, one base more at
    the price of a mismatch (jlim); gaps of n - 1, n, n + 1 are out of reach for n = 100000, and `-A25` can place nothing at all;
  * the junction score is a UINT32 kept as a UINT16: introns beyond some 80 000 bases under a 100-base read wrap it, and such a junction
    beats every other placement (jlim|A100000_*);
  * a read equally placed in two copies 1 000 bases apart is ambiguous for -a and a junction between the copies for -A (tie|two_copies);
  * no more than two substitutions are accepted beside a gap whatever -s says (mm_*3_*).
"""
import gzip
import json
import os
import struct
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, gz_copy, rand_seq, revcomp, run, write_fasta, write_reads  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
from helpers import read_sfx  # noqa: E402

OUT = os.path.join(HERE, "indeledge")
REPEAT = os.path.join(HERE, "repeat")
LEN_FLAGS = ["-l30", "-L1100"]

# class -> what it is designed for: "found" (at least one read reported with two segments at the planted place in some run), "refused"
# (none with two segments in any run), "any" (whatever the reference does is recorded)
CLASSES = {"flank": "found", "jseg": "found", "ilen": "found", "jgap": "found", "seqstart": "found", "seqend": "found", "catends": "found",
           "jlim": "found", "readlen": "found", "mm": "found", "n": "found", "tie": "found", "big": "found", "rep": "found",
           "beyond_limit": "refused", "no_gap": "refused"}
# cases of the found classes that are never found at the planted place, and why
NEVER_AT_PLANTED = {
    "big|Z_last": "behind the cut at 100 placements", "big|Z_r100": "the first placement behind the cut at 100",
    "mm|i2_b13": "two substitutions in 13 bases: more than one per 7", "rep|K6000": "more copies than MaxIter, all true placements behind the cut",
    "tie|ins_del": "the insertion wins the tie: another end", "tie|len1000": "the nearer acceptor wins", "tie|two_copies": "ambiguous for -a, a junction between the copies for -A",
    "tie|two_seqs": "ambiguous"}
# repeated anchor cores of eF / eL: where among the copies, in suffix-array order, the true placements lie
FAM_LABELS = {"X": (("first", "A"), ("last", "T")), "Y": (("first", "A"), ("last", "T")),
              "Z": (("first", "AA"), ("r98", "AG"), ("r100", "AT"), ("last", "T"))}
# tag -> run
CASES = {
    "a20s3": dict(flags=["-a20", "-s3"]),
    "a3s5": dict(flags=["-a3", "-s5"]),
    "a1s1": dict(flags=["-a1", "-s1"]),
    "a20s0": dict(flags=["-a20", "-s0"]),
    "A100000s3": dict(flags=["-A100000", "-s3"]),
    "A500s5": dict(flags=["-A500", "-s5"]),
    "A25s1": dict(flags=["-A25", "-s1"]),
    "a20A100000s3": dict(flags=["-a20", "-A100000", "-s3"]),
    "r1R5a20s3": dict(flags=["-r1", "-R5", "-a20", "-s3"]),
    "c50a20A5000s3": dict(flags=["-c50", "-a20", "-A5000", "-s3"]),
    "rep_a5A200s3": dict(flags=["-a5", "-A200", "-s3"], genome="repeat"),
    "rep_a5s3Q1": dict(flags=["-a5", "-s3", "-Q1"], genome="repeat"),
    "rep_A200s3Q2": dict(flags=["-A200", "-s3", "-Q2"], genome="repeat"),
}


def other_base(rng, c):
    return "ACGT"[("ACGT".index(c) + int(rng.integers(1, 4))) % 4] if c in "ACGT" else "ACGT"[int(rng.integers(0, 4))]


class Planter:
    def __init__(self, rng, seqs):
        self.rng, self.seqs, self.reads, self.serial = rng, seqs, [], 0

    def build(self, kind, ch, p, a, l, b):
        """target-forward read: a bases from ch:p, a gap of l, b more bases -> (read, last base)"""
        g = self.seqs[ch]
        if kind == "ins":
            x = "".join(other_base(self.rng, g[p + a + i] if p + a + i < len(g) else "A") for i in range(l))
            return g[p:p + a] + x + g[p + a:p + a + b], p + a + b - 1
        return g[p:p + a] + g[p + a + l:p + a + l + b], p + a + l + b - 1

    def explorable(self, s, ch, p, end, a, need):
        """would the ungapped compare from the anchored end show `need` mismatches on the short side, the first one at the gap"""
        g = self.seqs[ch]
        if len(s) - a <= a:                        # short 3' side: anchored at p, explored rightwards
            if p + len(s) > len(g):
                return False
            return s[a] != g[p + a] and sum(1 for i in range(a, len(s)) if s[i] != g[p + i]) >= need
        t = end + 1 - len(s)
        if t < 0:
            return False
        return s[a - 1] != g[t + a - 1] and sum(1 for i in range(a) if s[i] != g[t + i]) >= need

    def emit(self, cls, kind, ch, start, end, strand, s):
        r = revcomp(s) if strand == "-" else s
        for cp in "ab":
            self.reads.append((f"{cls[0]}|{cls[1]}|{kind}|{ch}|{start}|{end}|{strand}|{self.serial}/{cp}", r))
        self.serial += 1

    def plant(self, cls, kind, ch, p, a, l, b, strand, subs=(), n_at=None):
        s, end = self.build(kind, ch, p, a, l, b)
        assert len(s) == a + b + (l if kind == "ins" else 0) and end < len(self.seqs[ch]), (cls, kind, ch, p, a, l, b)
        s = list(s)
        for k in subs:
            s[k] = other_base(self.rng, s[k])
        if n_at is not None:
            s[n_at] = "N"
        self.emit(cls, kind, ch, p, end, strand, "".join(s))

    def sample(self, cls, kind, ch, a, l, b, strand, need, lo, hi, subs=()):
        for _ in range(20000):
            p = int(self.rng.integers(lo, hi))
            s, end = self.build(kind, ch, p, a, l, b)
            if end >= len(self.seqs[ch]) or "N" in self.seqs[ch][p:end + 1]:
                continue
            if self.explorable(s, ch, p, end, a, need):
                s = list(s)
                for k in subs:
                    s[k] = other_base(self.rng, s[k])
                self.emit(cls, kind, ch, p, end, strand, "".join(s))
                return p
        raise SystemExit(f"no place for {cls} {kind} {a} {l} {b}")


def make_genome(rng):
    seqs = {}
    seqs["eA"] = rand_seq(rng, 3000)
    seqs["eP"] = rand_seq(rng, 8000)
    b = list(rand_seq(rng, 4000))
    n_sites = [400 * k for k in range(1, 9)]                    # single Ns
    for q in n_sites:
        b[q] = "N"
    b[3600:3603] = "NNN"
    seqs["eB"] = "".join(b)
    # eL: unique, copies of Z, unique
    z = rand_seq(rng, 16)
    parts = [rand_seq(rng, 5000)]
    for _ in range(5150):
        parts.append(z)
        parts.append("CG"[int(rng.integers(0, 2))] + rand_seq(rng, int(rng.integers(1, 3))))
    el = "".join(parts)
    z_end = len(el)
    el += rand_seq(rng, 108000 - len(el))
    seqs["eL"] = el
    # eF: families X (80 copies) and Y (150), then single copies of X, Y, Z in unique surroundings followed by A / T
    x, y = rand_seq(rng, 25), rand_seq(rng, 25)
    parts = [rand_seq(rng, 300)]
    for fam, k in ((x, 80), (y, 150)):
        for _ in range(k):
            parts.append(fam)
            parts.append("CG"[int(rng.integers(0, 2))] + rand_seq(rng, int(rng.integers(3, 8))))
        parts.append(rand_seq(rng, 200))
    f = "".join(parts)
    # (what follows a copy decides its rank among the copies: the spacers begin with C or G, so the copies followed by an A come first, in
    # the order of what follows that A, and those followed by a T last.  Z: ranks 0, 1 ("AA"), 2..97 (96 further copies, "AC"), 98, 99
    # ("AG"), 100, 101 ("AT") - the walk looks at the number of copies once 100 placements are done)
    fam_sites = {}
    for name, fam in (("X", x), ("Y", y), ("Z", z)):
        for label, nxt in FAM_LABELS[name]:
            for side in "53":
                f += rand_seq(rng, 150)
                fam_sites[(name, label, side)] = len(f)
                f += fam + nxt + ("A" if side == "5" else "T" if len(nxt) == 2 else "") + rand_seq(rng, 100)
    for _ in range(96):
        f += rand_seq(rng, 6) + "T" + z + "AC" + rand_seq(rng, 4)
    f += rand_seq(rng, 300)
    seqs["eF"] = f
    # eS: junction ties.  Each block: E1 (60) donor .. near acceptor E2' .. far acceptor E2; read = E1 + E2 (40)
    s = list(rand_seq(rng, 16000))
    ties = {}

    def no_motif(at):                                # the two bases before `at` are neither AG nor AC
        s[at - 2:at] = "TT"

    def tie_block(name, at, near_gap, far_gap, donor, far_acc, near_sub):
        s[at + 60 + far_gap] = "A"                   # (no donor starts with an A: the gap cannot slide by a base)
        e2 = s[at + 60 + far_gap:at + 60 + far_gap + 40]
        near = list(e2)
        if near_sub:
            near[20] = other_base(rng, near[20])
        s[at + 60 + near_gap:at + 60 + near_gap + 40] = near
        s[at + 60:at + 62] = donor
        no_motif(at + 60 + near_gap)
        if far_acc:
            s[at + 60 + far_gap - 2:at + 60 + far_gap] = far_acc
        else:
            no_motif(at + 60 + far_gap)
        ties[name] = (at, near_gap, far_gap)

    tie_block("bonusGT", 300, 200, 600, "GT", "AG", False)       # the farther acceptor earns the bonus: it wins on either strand
    tie_block("bonusCT", 1500, 200, 600, "CT", "AC", False)
    tie_block("len999", 2700, 500, 999, "TA", None, True)         # nearer: one mismatch (-5); farther: exact and below 1000 bases: it wins
    tie_block("len1000", 4700, 500, 1000, "TA", None, True)       # farther: exact, but 1 x 10 for its length: the nearer one wins
    tie_block("strandGT", 6000, 300, 4500, "GT", "AG", False)     # bonus 50 - 40 on '+' (farther wins), 25 - 40 on '-' (nearer wins)
    tie_block("strandCT", 11000, 300, 4500, "CT", "AC", False)    # and the other way round
    seqs["eS"] = "".join(s)
    # eT: microInDel ties
    t = list(rand_seq(rng, 3000))
    t[1200:1350] = t[200:350]                                     # twice, exactly
    t[1600:1750] = t[600:750]                                     # twice, the second copy with one substitution
    t[1700] = other_base(rng, t[1700])
    t[2200:2350] = t[2000:2150]                                   # twice, the first copy with one substitution
    t[2100] = other_base(rng, t[2100])
    t[2600:2640] = list("AC" * 20)                                # insertion or deletion of one base
    if t[2599] in "AC":
        t[2599] = "G"
    seqs["eT"] = "".join(t)
    e = rand_seq(rng, 2500)
    seqs["eE"] = e[:1200] + seqs["eA"][2000:2500] + e[1700:]      # 500 bases of the first sequence again in the last
    return seqs, dict(n_sites=n_sites, z=z, z_end=z_end, fam_sites=fam_sites, fams=dict(X=x, Y=y, Z=z), ties=ties)


def make_reads(rng, seqs, info):
    P = Planter(rng, seqs)
    plant, sample = P.plant, P.sample

    def cls(name, case, refused=None):
        """(class, case) of the reads that follow; a case designed to be refused goes to one of the two classes of that kind"""
        return (refused, f"{name}_{case}") if refused else (name, str(case))

    # ---- flank limits: the gap d bases from the read's 5' / 3' end.  With fewer than 8 bases the search never tries a gap there
    for d in (5, 6, 7, 8, 9):
        c = cls("flank", d, None if d >= 7 else "beyond_limit")
        for end5 in (True, False):
            for strand in "+-":
                for kind in ("ins", "del"):
                    short_first = end5 == (strand == "+")               # target-forward: is the short flank the first one
                    l = 3
                    a, b = (d, 100 - d - (l if kind == "ins" else 0)) if short_first else (100 - d - (l if kind == "ins" else 0), d)
                    sample(c, kind, "eP", a, l, b, strand, min(d, 7), 50, 7800)
    for d in (9, 10, 11, 12):
        c = cls("jseg", d, None if d >= 11 else "beyond_limit")
        for end5 in (True, False):
            for strand in "+-":
                short_first = end5 == (strand == "+")
                a, b = (d, 100 - d) if short_first else (100 - d, d)
                sample(c, "jct", "eP", a, 200, b, strand, 8, 50, 7600)
    # ---- length limits
    for l in (1, 2, 3, 4, 20, 21):
        c = cls("ilen", l, None if l <= 20 else "beyond_limit")
        for strand in "+-":
            for kind in ("ins", "del"):
                sample(c, kind, "eP", 50, l, 50 - (l if kind == "ins" else 0), strand, 7, 50, 7800)
    for gap in (24, 25, 26, 499, 500, 501, 999, 1000, 1001, 1999, 2000):
        c = cls("jgap", gap, None if gap >= 25 else "beyond_limit")
        for strand in "+-":
            for a in (40, 60):
                sample(c, "jct", "eP", a, gap, 100 - a, strand, 8, 50, 5800)
    for gap in (99999, 100000, 100001):
        c = cls("jgap", gap, "beyond_limit")
        for strand in "+-":
            for a in (40, 60):
                sample(c, "jct", "eL", a, gap, 100 - a, strand, 8, 1000, 3000)
    # the limit itself: ExploreSpliceRight / -Left try gaps below the limit less the moved segment (and less 10 going left), so the longest
    # intron `-A n` can place is n - 41 bases before a 40-base second segment and n - 51 bases behind a 40-base first one
    for big in (500, 100000):
        for a, b, last in ((60, 40, big - 41), (40, 60, big - 51)):
            for gap in (last, last + 1, last + 6):         # (one base further is still reached by moving the gap one mismatch along)
                c = cls("jlim", f"A{big}_{a}_{gap - last}", None if (gap <= last + 1 or big == 500) else "beyond_limit")
                for strand in "+-":
                    if big == 500:
                        sample(c, "jct", "eP", a, gap, b, strand, 8, 50, 7000)
                    else:
                        sample(c, "jct", "eL", a, gap, b, strand, 8, 1000, 3000)
    # ---- sequence and concatenation ends
    for ch in ("eA", "eB"):
        c = cls("seqstart", ch)
        for p in (0, 1, 2, 3, 5, 8, 13, 20):
            kind = ("ins", "del", "jct")[p % 3]
            l = 60 if kind == "jct" else 4
            plant(c, kind, ch, p, 50, l, 50 - (l if kind == "ins" else 0), "+-"[p % 2])
    for ch in ("eA", "eE"):
        c = cls("seqend", ch)
        n = len(seqs[ch])
        for k, kind in enumerate(("ins", "del", "jct", "ins", "del", "jct")):
            l = 80 if kind == "jct" else 5
            span = 100 + (l if kind != "ins" else 0)
            a = 45 + 2 * k
            plant(c, kind, ch, n - span, a, l, 100 - a - (l if kind == "ins" else 0), "+-"[k % 2])
    for ch in ("eA", "eE"):                           # a junction read whose 3' anchor ends on the last base (no 5' anchor: 30 bases): LocateSpliceJuncts
        n = len(seqs[ch])                             # wants one base more behind the placement than LocateInDels; one base earlier it is found
        for strand in "+-":
            plant(cls("seqend", "jct3_last", "beyond_limit"), "jct", ch, n - 180, 30, 80, 70, strand)
            plant(cls("seqend", "jct3_last_but_one"), "jct", ch, n - 181, 30, 80, 70, strand)
    c = cls("cross_entry", "del", "beyond_limit")     # a deletion explored leftwards whose first segment (9 bases) lies in the sequence before
    for prev, ch in (("eA", "eP"), ("eP", "eB")):
        g0, g1, done = seqs[prev], seqs[ch], 0
        for d in range(0, 12):
            for l in range(12, 21):
                # ungapped the read starts d bases into ch; its first 9 bases are the previous sequence's, l bases before
                k0 = len(g0) + 1 + d - l                  # locus in prev of the read's first base (the separator counts as one position)
                if k0 + 9 > len(g0) or done >= 2:
                    continue
                s = g0[k0:k0 + 9] + g1[d + 9:d + 100]
                if s[8] != g1[d + 8] and sum(1 for i in range(9) if s[i] != g1[d + i]) >= 7:
                    for strand in "+-":
                        P.emit(c, "none", ch, -1, -1, strand, s)
                    done += 1
        assert done == 2, (prev, ch)
    c = cls("catends", "jct")                    # junctions whose outer segment lies within 35 bases of either end of the concatenation
    for p in (0, 10, 34):
        for strand in "+-":
            plant(c, "jct", "eA", p, 30, 300, 70, strand)
            n = len(seqs["eE"])
            plant(c, "jct", "eE", n - 400 - p, 70, 300, 30, strand)
    c = cls("del_before_start", "x", "no_gap")            # 3' 60 bases from locus t of the first / a later sequence, 5' 40 bases foreign: the leftward
    for ch in ("eA", "eB"):                            # search tries deletions of up to 20 bases with fewer than that before the read
        for t in (0, 3, 10, 19):
            for strand in "+-":
                P.emit(c, "none", ch, -1, -1, strand, rand_seq(rng, 40) + seqs[ch][t + 40:t + 100])
    c = cls("seg2_beyond_end", "x", "no_gap")             # after a deletion of 5 the second segment would run over the separator into the next sequence
    for ch, nxt in (("eA", "eP"), ("eT", "eE")):
        n = len(seqs[ch])
        for strand in "+-":
            P.emit(c, "none", ch, -1, -1, strand, seqs[ch][n - 60:n - 10] + seqs[ch][n - 5:n] + seqs[nxt][0:45])
            P.emit(c, "none", ch, -1, -1, strand, seqs[ch][n - 60:n - 10] + rand_seq(rng, 50))
    c = cls("separator_gap", "x", "no_gap")                   # fits only with the separator as a deleted base / as part of an intron
    for ch, nxt in (("eA", "eP"), ("eT", "eE")):
        n = len(seqs[ch])
        for strand in "+-":
            P.emit(c, "none", ch, -1, -1, strand, seqs[ch][n - 50:n] + seqs[nxt][0:50])
            P.emit(c, "none", ch, -1, -1, strand, seqs[ch][n - 90:n - 40] + seqs[nxt][0:50])
            P.emit(c, "none", ch, -1, -1, strand, seqs[ch][n - 50:n] + seqs[nxt][40:90])
    # ---- read lengths
    for ln in (30, 31, 50, 51, 64, 65, 128, 129, 150, 250, 500, 1000):
        c = cls("readlen", ln)
        for strand in "+-":
            for kind in ("ins", "del", "jct"):
                l = 150 if kind == "jct" else 2
                a = ln // 2 + (1 if strand == "-" else 0)
                sample(c, kind, "eP", a, l, ln - a - (l if kind == "ins" else 0), strand, 8 if ln >= 50 else 7, 50, 6500)
    # ---- mismatch budget: n substitutions between the 5' anchor core and the gap (side k) or in the b bases behind the gap (side i);
    #      behind the gap the budget is one per 7 bases compared
    for side in "ki":
        for n in (0, 1, 2, 3):
            for b in (13, 20, 22, 38):
                c = cls("mm", f"{side}{n}_b{b}", "beyond_limit" if n > 2 else None)
                for kind in ("ins", "del", "jct"):
                    l = 120 if kind == "jct" else 3
                    a = 100 - b - (l if kind == "ins" else 0)
                    ofs = a + (l if kind == "ins" else 0)
                    if side == "k":
                        subs = [int(q) for q in rng.choice(np.arange(50, a - 1), n, replace=False)]
                    else:
                        subs = [int(q) for q in ofs + 1 + rng.choice(b - 2, n, replace=False)]
                    sample(c, kind, "eP", a, l, b, "+-"[n % 2], 8, 50, 7600, subs=subs)
    # ---- N
    sites = info["n_sites"]
    c = cls("n", "target_flank")                  # a target N ten bases into the second segment (the read holds a base there)
    for k, kind in enumerate(("ins", "del", "jct")):
        q = sites[k]
        l = 100 if kind == "jct" else 3
        for strand in "+-":
            s, end = P.build(kind, "eB", q - 10 - 50 - (l if kind != "ins" else 0), 50, l, 50 - (l if kind == "ins" else 0))
            s = s.replace("N", "ACGT"[int(rng.integers(0, 4))])
            P.emit(c, kind, "eB", q - 10 - 50 - (l if kind != "ins" else 0), end, strand, s)
    c = cls("n", "at_gap")                        # the target N is the first base behind the gap
    for k, kind in enumerate(("ins", "del", "jct")):
        q = sites[3 + k % 2]
        l = 100 if kind == "jct" else 3
        p = q - 50 - (l if kind != "ins" else 0)
        for strand in "+-":
            s, end = P.build(kind, "eB", p, 50, l, 50 - (l if kind == "ins" else 0))
            P.emit(c, kind, "eB", p, end, strand, s.replace("N", "ACGT"[int(rng.integers(0, 4))]))
    c = cls("n", "in_intron")                     # an N (and the run of three) inside the scanned window
    for q in (sites[5], 3600):
        for strand in "+-":
            plant(c, "jct", "eB", q - 100, 50, 200, 50, strand)
            plant(c, "jct", "eB", q - 160, 60, 200, 40, strand)
    c = cls("n", "in_read")                     # one N in the read, in the second segment
    for kind in ("ins", "del", "jct"):
        l = 100 if kind == "jct" else 3
        for strand in "+-":
            s, end = P.build(kind, "eP", 7000, 50, l, 50 - (l if kind == "ins" else 0))
            P.emit(c, kind, "eP", 7000, end, strand, s[:80] + "N" + s[81:])
    # ---- ties and replacement
    c = cls("tie", "two_copies")              # equally good in two copies: ambiguous
    for kind in ("ins", "del"):
        for strand in "+-":
            plant(c, kind, "eT", 220, 50, 3, 50 - (3 if kind == "ins" else 0), strand)
    c = cls("tie", "two_seqs")                  # equally good in two sequences: ambiguous for -a and for -A (no intron leads from one to the other)
    for kind in ("ins", "del", "jct"):
        for strand in "+-":
            l = 150 if kind == "jct" else 3
            plant(c, kind, "eA", 2100, 50, l, 50 - (l if kind == "ins" else 0), strand)
    c = cls("tie", "better_copy")               # exact in one copy, one substitution in the other: whichever comes later in the suffix array
    for p in (620, 2020 + 180):
        for kind in ("ins", "del"):
            for strand in "+-":
                plant(c, kind, "eT", p, 50, 3, 50 - (3 if kind == "ins" else 0), strand)
    c = cls("tie", "same_start")                # both anchor cores lead to the same first segment
    for kind in ("ins", "del", "jct"):
        for strand in "+-":
            sample(c, kind, "eP", 50, 130 if kind == "jct" else 2, 50 - (2 if kind == "ins" else 0), strand, 8, 50, 7600)
    c = cls("tie", "ins_del")                   # 70 unique bases, then the dinucleotide run one base on: insertion and deletion of one base tie
    for strand in "+-":
        P.emit(c, "del", "eT", 2530, 2630, strand, seqs["eT"][2530:2600] + seqs["eT"][2601:2631])
    for name, (at, near_gap, far_gap) in info["ties"].items():
        c = cls("tie", name)
        for strand in "+-":
            s = seqs["eS"][at:at + 60] + seqs["eS"][at + 60 + far_gap:at + 100 + far_gap]
            P.emit(c, "jct", "eS", at, at + 99 + far_gap, strand, s)
    # ---- large anchor intervals: the repeated core at the read's 5' (phase 0) or 3' end (phase 1) of the matched strand
    f = seqs["eF"]
    for fam, core in info["fams"].items():
        ln = 2 * len(core) + 1
        for label, _ in FAM_LABELS[fam]:
            # (Z_r100 and Z_last lie behind the cut at 100 placements: never found at the planted place, but a 33-base read may be placed
            # by chance at one of the 100 copies that are looked at, so they stay in this class)
            c = cls("big", f"{fam}_{label}")
            for side in "53":
                q = info["fam_sites"][(fam, label, side)]
                for kind in ("ins", "del", "jct"):
                    for strand in "+-":
                        l = 40 if kind == "jct" else 2
                        if side == "5":               # target-forward read starts with the core
                            a = len(core) + 4
                            plant(c, kind, "eF", q, a, l, ln - a - (l if kind == "ins" else 0), strand)
                        else:
                            b = len(core) + 4
                            a = ln - b - (l if kind == "ins" else 0)
                            plant(c, kind, "eF", q + len(core) - (ln + (l if kind != "ins" else 0)) + (l if kind == "ins" else 0), a, l, b, strand)
    # ---- background
    c = cls("plain", "x", "no_gap")
    for k in range(120):
        ch = ("eA", "eP", "eB", "eE", "eT")[k % 5]
        ln = (40, 75, 100, 140)[k % 4]
        p = int(rng.integers(0, len(seqs[ch]) - ln))
        s = list(seqs[ch][p:p + ln].replace("N", "A"))
        for q in rng.choice(ln, k % 5, replace=False):
            s[q] = other_base(rng, s[q])
        P.reads.append((f"{c[0]}|{c[1]}|none|{ch}|-1|-1|{'+-'[k % 2]}|p{k}/a", revcomp("".join(s)) if k % 2 else "".join(s)))
    order = rng.permutation(len(P.reads))
    return [P.reads[i] for i in order]


def make_repeat_reads(rng):
    """51-base reads on the repeat genome: the 25-base anchor core is one of its 25-mers of 2 000..6 000 copies, the rest unique (chrU)"""
    _, sa, _ = read_sfx(os.path.join(REPEAT, "genome.sfx.gz"))
    fa = gzip.open(os.path.join(REPEAT, "genome.fa.gz"), "rt").read().split(">")[1:]
    u = "".join(fa[0].split("\n")[1:])
    assert fa[0].startswith("chrU") and len(u) == 60000
    rank = np.empty(len(sa), dtype=np.int64)
    rank[sa] = np.arange(len(sa))
    reads = []
    serial = 0
    for fi, K in enumerate((2000, 3000, 4000, 6000)):
        core_at = [1000 + fi * 14000 + j * 1100 + 25 for j in range(12)]
        ranks = sorted((int(rank[q]), q) for q in core_at)
        first = ranks[0][0]                           # (the copies of chrR follow in rank order; ranks relative to the lowest chrU copy are
        picks = [ranks[0], ranks[1], ranks[len(ranks) // 2], ranks[-1]]      # only a label)
        for rk, q in picks:
            name = f"rep|K{K}"
            for side in "53":
                for kind in ("ins", "del", "jct"):
                    for strand in "+-":
                        l = 60 if kind == "jct" else 2
                        if side == "5":
                            a = 29
                            b = 51 - a - (l if kind == "ins" else 0)
                            p = q
                        else:
                            b = 29
                            a = 51 - b - (l if kind == "ins" else 0)
                            p = q + 25 - (51 + (l if kind != "ins" else 0)) + (l if kind == "ins" else 0)
                        if kind == "ins":
                            s = u[p:p + a] + "".join(other_base(rng, ch) for ch in u[p + a:p + a + l]) + u[p + a:p + a + b]
                            end = p + a + b - 1
                        else:
                            s = u[p:p + a] + u[p + a + l:p + a + l + b]
                            end = p + a + l + b - 1
                        r = revcomp(s) if strand == "-" else s
                        for cp in "ab":
                            reads.append((f"{name}|{kind}|chrU|{p}|{end}|{strand}|r{rk - first}s{serial}/{cp}", r))
                        serial += 1
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def m0_records(path):
    out = {}
    for line in open(path):
        f = line.rstrip("\n").split(",")
        out.setdefault(f[13].strip('"'), []).append((f[1].strip('"'), f[3].strip('"'), int(f[4]), int(f[5]), int(f[6]), f[7].strip('"'), int(f[11])))
    return out


def m6_records(path):
    out = {}
    for line in open(path):
        if line[0] == "@":
            continue
        t = line.rstrip("\n").split("\t")
        out[t[0]] = (t[1:9], [x for x in t[11:] if x.startswith("YU:Z:")])
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261021)
    seqs, info = make_genome(rng)
    reads = make_reads(rng, seqs, info)
    rep_reads = make_repeat_reads(rng)
    print(f"{len(reads)} reads, {len(rep_reads)} on the repeat genome, {len(CLASSES)} classes")
    with tempfile.TemporaryDirectory() as tmp:
        fa, sfx = os.path.join(tmp, "genome.fa"), os.path.join(tmp, "genome.sfx")
        write_fasta(fa, list(seqs.items()))
        run([REF, "index", "-i", fa, "-o", sfx, "-r", "indeledge", "-T4"], tmp)
        rep_sfx = os.path.join(tmp, "repeat.sfx")
        with gzip.open(os.path.join(REPEAT, "genome.sfx.gz"), "rb") as f, open(rep_sfx, "wb") as g:
            g.write(f.read())
        files = {}
        for key, rs in (("indeledge", reads), ("repeat", rep_reads)):
            fwd, rev = os.path.join(tmp, f"reads_{key}.fa"), os.path.join(tmp, f"reads_{key}_rev.fa")
            write_reads(fwd, rs)
            write_reads(rev, rs[::-1])
            files[key] = (fwd, rev)
        gz_copy(fa, os.path.join(OUT, "genome.fa.gz"))
        gz_copy(sfx, os.path.join(OUT, "genome.sfx.gz"))
        gz_copy(files["indeledge"][0], os.path.join(OUT, "reads.fa.gz"))
        gz_copy(files["repeat"][0], os.path.join(OUT, "reads_repeat.fa.gz"))
        found_anywhere = {c: 0 for c in CLASSES}
        two_anywhere = {c: 0 for c in CLASSES}
        out_cases, case_found = {}, {}
        # every run three times (-T1, -T4, -T4 on the reversed read file), each as CSV and as SAM; the runs do not depend on each other
        jobs = []
        for tag, cs in CASES.items():
            key = cs.get("genome", "indeledge")
            cs["all_flags"] = cs["flags"] + (LEN_FLAGS if key == "indeledge" else ["-l30"])
            for variant, (threads, rd) in enumerate((("-T1", files[key][0]), ("-T4", files[key][0]), ("-T4", files[key][1]))):
                for fmt, ext in (("-M0", "m0.csv"), ("-M6", "m6.sam")):
                    jobs.append([REF, "align", "-i", rd, "-I", rep_sfx if key == "repeat" else sfx, "-o", os.path.join(tmp, f"{tag}.{variant}.{ext}"),
                                 fmt, threads] + cs["all_flags"])
        with ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(lambda cmd: run(cmd, tmp), jobs))
        for tag, cs in CASES.items():
            key = cs.get("genome", "indeledge")
            flags = cs["all_flags"]
            recs = [(m0_records(os.path.join(tmp, f"{tag}.{v}.m0.csv")), m6_records(os.path.join(tmp, f"{tag}.{v}.m6.sam"))) for v in range(3)]
            for v in (1, 2):
                for what in (0, 1):
                    bad = [n for n in recs[0][what] if recs[v][what].get(n) != recs[0][what][n]] + [n for n in recs[v][what] if n not in recs[0][what]]
                    if bad:
                        raise SystemExit(f"{tag}: not repeatable ({'-T4' if v == 1 else 'reversed reads'}, {'CSV' if what == 0 else 'SAM'}): {sorted(set(bad))[:8]}")
            gz_copy(os.path.join(tmp, f"{tag}.1.m0.csv"), os.path.join(OUT, f"{tag}.m0.csv.gz"))
            gz_copy(os.path.join(tmp, f"{tag}.1.m6.sam"), os.path.join(OUT, f"{tag}.m6.sam.gz"))
            counts, case_counts = {}, {}
            for name, _ in (reads if key == "indeledge" else rep_reads):
                c, case, kind, ch, start, end = name.split("|")[:6]
                rows = recs[0][0].get(name, [])
                two = len(rows) == 2
                at = two and rows[0][1] == ch and rows[0][2] == int(start) and rows[1][3] == int(end)
                for n in (counts.setdefault(c, [0, 0, 0]), case_counts.setdefault(f"{c}|{case}", [0, 0, 0])):
                    n[0] += 1
                    n[1] += 1 if two else 0
                    n[2] += 1 if at else 0
            for c, n in counts.items():
                two_anywhere[c] += n[1]
                found_anywhere[c] += n[2]
            for c, n in case_counts.items():
                case_found[c] = case_found.get(c, 0) + n[2]
            out_cases[tag] = dict(flags=flags, genome=key, reads="reads.fa.gz" if key == "indeledge" else "reads_repeat.fa.gz", counts=counts,
                                  case_counts=case_counts)
            print("  ran", tag, "two-segment reads:", sum(n[1] for n in counts.values()))
        for c in sorted(case_found):
            print(f"  {c:32s}", " ".join(f"{t}:{out_cases[t]['case_counts'][c][1]}/{out_cases[t]['case_counts'][c][2]}/{out_cases[t]['case_counts'][c][0]}"
                                         for t in out_cases if c in out_cases[t]["case_counts"] and out_cases[t]["case_counts"][c][1]))
        # per case: the cases of the found classes that are by design never found at the planted place, and no others
        never_case = sorted(c for c, n in case_found.items() if n == 0 and CLASSES[c.split("|")[0]] == "found")
        assert never_case == sorted(NEVER_AT_PLANTED), (never_case, sorted(NEVER_AT_PLANTED))
        wrong = [c for c, d in CLASSES.items() if (d == "found" and found_anywhere[c] == 0) or (d == "refused" and two_anywhere[c] != 0)]
        assert not wrong, ("the reference does otherwise than designed", {c: (CLASSES[c], two_anywhere[c], found_anywhere[c]) for c in wrong})
        never = sorted(c for c in CLASSES if two_anywhere[c] == 0)
        print("classes without any two-segment placement:", never)
        print("cases never found at the planted place:", sorted(c for c, n in case_found.items() if n == 0))
        assert len(never) <= 2, never
        with open(os.path.join(OUT, "cases.json"), "w") as f:
            json.dump({"cases": out_cases, "classes": CLASSES, "no_two_segment": never, "case_found": case_found}, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
