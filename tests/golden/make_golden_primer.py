#!/usr/bin/env python3
"""Generates tests/golden/primer/: `biokanga align -6 <n>` fixtures (5' primer artefact correction, CAligner::PCR5PrimerCorrect), by
RUNNING THE REAL REFERENCE executable (oracle/_ref/biokanga, built by oracle/build_ref.sh).  Run in the build container only; everything
written is data.

    python tests/golden/make_golden_primer.py

Inputs (seeded): a genome of three sequences (30 000 + 20 000 + 12 000 bases) with a lower-case stretch in the first, 20 Ns in the
second - short enough that the indexer leaves the run alone - and one 300-base segment of the first repeated in the third; about 3 000
reads of 50, 60, 75 and 100 bases, among them on purpose, on both strands,
  * 0..7 substitutions all inside the first 12 bases of the read (corrected as far as needed, the later ones stay), all outside
    (rejected once above the rate), split so that the count gets down to MaxMMs at the k-th of several 5' mismatches, and split so
    that it stays one short (rejected),
  * reads at locus 0 and at the last locus of every sequence,
  * reads with an N among their first 12 bases,
  * reads whose first 12 bases lie over the N run's edge and inside the lower-case stretch,
  * reads of 13..15 substitutions for the run whose initial rate is capped at 15,
  * reads already within -s.
Pairs (60 bases, FR, inserts 200..400) with substitutions in either mate, and planted orphans: a mate inside the repeated segment
(no unique alignment of its own) with two substitutions at read offsets 15 and 45.  With -d150 -D1400 the recovery window is longer
than 1 000 bases, so the recovery looks for exact cores - whose length comes from the user's -s, not from the initial rate: cores of 30
(rate 1) are both broken, cores of 20 (rate 4) are not.  The generator runs the reference at `-s1 -6 3` and at `-s4` and asserts that
the planted mates are recovered by the second only.

cases.json: tag -> flags, the reads (se / pe), the outputs written, the tag of the run without -6 at the initial rate (`base`; -x is
left out of it: it runs behind the correction) and the three counts of the reference's "Completed PCR 5' primer correction" line.
"""
import gzip
import json
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, gz_copy, rand_seq, revcomp, run, write_fasta, write_reads  # noqa: E402

OUT = os.path.join(HERE, "primer")
LENS = {"pcA": 30000, "pcB": 20000, "pcC": 12000}
LOWER = (5000, 5400)              # of pcA
N_AT, N_LEN = 8000, 20            # of pcB
DUP_FROM, DUP_TO, DUP_LEN = 21000, 6000, 300     # pcA[21000:21300] again at pcC[6000:6300]
PE_D, PE_DD = 150, 1400
COUNTS = re.compile(r"Completed PCR 5' primer correction, (\d+) reads with (\d+) bases corrected, (\d+) reads with excessive substitutions rejected")


def sub_at(rng, r, positions):
    r = list(r)
    for k in positions:
        r[k] = "ACGT"[("ACGTN".index(r[k].upper()) + int(rng.integers(1, 4))) % 4] if r[k].upper() != "N" else "ACGT"[int(rng.integers(0, 4))]
    return "".join(r)


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261019)
    a, b, c = (rand_seq(rng, n) for n in LENS.values())
    a = a[:LOWER[0]] + a[LOWER[0]:LOWER[1]].lower() + a[LOWER[1]:]
    b = b[:N_AT] + "N" * N_LEN + b[N_AT + N_LEN:]
    c = c[:DUP_TO] + a[DUP_FROM:DUP_FROM + DUP_LEN] + c[DUP_TO + DUP_LEN:]
    seqs = {"pcA": a, "pcB": b, "pcC": c}
    reads = []

    def in_dup(ch, p, ln):
        return (ch == "pcA" and p < DUP_FROM + DUP_LEN and p + ln > DUP_FROM) or (ch == "pcC" and p < DUP_TO + DUP_LEN and p + ln > DUP_TO)

    def add(tag, ch, p, ln, strand, five=0, rest=0, five_pos=None, n_at=None):
        """a read of ln bases from ch:p on `strand` with `five` substitutions among its own first 12 bases and `rest` behind them"""
        s = seqs[ch][p:p + ln].upper()
        assert len(s) == ln and not in_dup(ch, p, ln), (tag, ch, p)
        r = revcomp(s) if strand == "-" else s
        pos5 = sorted(five_pos if five_pos is not None else rng.choice(12, five, replace=False))
        posr = sorted(12 + rng.choice(ln - 12, rest, replace=False))
        r = sub_at(rng, r, list(pos5) + list(posr))
        if n_at is not None:
            r = r[:n_at] + "N" + r[n_at + 1:]
        reads.append((f"{tag}{len(reads)}|{ch}|{p}|{strand}|{len(pos5)}|{rest}", r))

    def place(ln):
        while True:
            ch = ("pcA", "pcB", "pcC")[int(rng.integers(0, 3))]
            p = int(rng.integers(0, LENS[ch] - ln + 1))
            if "N" in seqs[ch][p:p + ln] or in_dup(ch, p, ln):
                continue
            return ch, p

    for _ in range(1500):                          # background: 0..6 substitutions anywhere
        ln = (50, 60, 75, 100)[int(rng.integers(0, 4))]
        ch, p = place(ln)
        k = int(rng.integers(0, 7))
        f = int(rng.integers(0, k + 1))
        add("r", ch, p, ln, "+-"[int(rng.integers(0, 2))], min(f, 8), k - min(f, 8))
    for ln in (50, 60, 75, 100):                   # the planted shapes
        for strand in "+-":
            for five in range(0, 8):               # all inside the first 12
                for _ in range(3):
                    add("in", *place(ln), ln, strand, five, 0)
            for rest in range(0, 8):               # all outside
                for _ in range(2):
                    add("out", *place(ln), ln, strand, 0, rest)
            for five in range(1, 6):               # split: reached at the k-th, exactly, one short, ..
                for rest in range(1, 6):
                    add("sp", *place(ln), ln, strand, five, rest)
            for n_at in (0, 5, 11):                # a read N inside the first 12, alone and beside substitutions
                for five, rest in ((0, 0), (1, 1), (2, 2), (0, 3)):
                    ch, p = place(ln)
                    free = [k for k in range(12) if k != n_at]
                    add("rn", ch, p, ln, strand, five, rest, five_pos=list(rng.choice(free, five, replace=False)), n_at=n_at)
    for ch, n in LENS.items():                     # locus 0 and the last locus of every sequence
        for ln in (50, 100):
            for strand in "+-":
                for five, rest in ((0, 0), (2, 2), (3, 0), (1, 4)):
                    add("e0", ch, 0, ln, strand, five, rest)
                    add("e1", ch, n - ln, ln, strand, five, rest)
    for ln in (60, 100):                           # the first 12 bases over the edge of the N run: 1..3 target Ns under them
        for over in (1, 2, 3):
            for rest in (0, 1, 2, 3):
                # '+': the read starts on the run's last `over` bases; '-': it ends on the run's first `over` bases
                for strand, p in (("+", N_AT + N_LEN - over), ("-", N_AT + over - ln)):
                    s = seqs["pcB"][p:p + ln]
                    r = revcomp(s) if strand == "-" else s
                    r = "".join("ACGT"[int(rng.integers(0, 4))] if ch == "N" else ch for ch in r)
                    r = sub_at(rng, r, sorted(12 + rng.choice(ln - 12, rest, replace=False)))
                    reads.append((f"tn{len(reads)}|pcB|{p}|{strand}|{over}|{rest}", r))
    for k in range(60):                            # inside the lower-case stretch
        ln = (50, 75, 100)[k % 3]
        p = LOWER[0] + int(rng.integers(0, LOWER[1] - LOWER[0] - ln))
        add("lc", "pcA", p, ln, "+-"[k % 2], k % 5, (k // 5) % 4)
    for k in range(20):                            # several reads on one start (-k)
        ln = (60, 100)[k % 2]
        ch, p = place(ln)
        for j in range(3):
            add("dup", ch, p, ln, "+-"[k % 4 < 2], j, (j + k) % 3)
    for k in range(90):                            # 13..15 substitutions (the -s12 -6 5 run: initial rate 15, not 17)
        tot = 13 + k % 3
        five = int(rng.integers(0, 7))
        add("hi", *place(100), 100, "+-"[k % 2], five, tot - five)
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]

    # pairs: FR, inserts 200..400, 60 bases
    L = 60
    pe1, pe2, planted = [], [], []
    for k in range(400):
        ch = ("pcA", "pcB", "pcC")[k % 3]
        ins = int(rng.integers(200, 401))
        p = int(rng.integers(100, LENS[ch] - ins - 100))
        frag = seqs[ch][p:p + ins].upper()
        if "N" in frag or in_dup(ch, p, ins):
            continue
        m1, m2 = frag[:L], revcomp(frag[-L:])
        f1, r1 = int(rng.integers(0, 4)), int(rng.integers(0, 3))
        m1 = sub_at(rng, m1, sorted(list(rng.choice(12, f1, replace=False)) + list(12 + rng.choice(L - 12, r1, replace=False))))
        if k % 3 == 0:
            f2, r2 = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            m2 = sub_at(rng, m2, sorted(list(rng.choice(12, f2, replace=False)) + list(12 + rng.choice(L - 12, r2, replace=False))))
        if k % 4 == 0:
            m1, m2 = m2, m1
        pe1.append((f"p{k}|{ch}|{p}/1", m1))
        pe2.append((f"p{k}|{ch}|{p}/2", m2))
    for k in range(24):                            # orphans: the second mate inside the repeated segment, offsets 15 and 45 substituted
        in_a = k % 2 == 0
        ch, d0 = ("pcA", DUP_FROM) if in_a else ("pcC", DUP_TO)
        q = d0 + 20 + 9 * k                        # the mate's locus, inside the repeat
        ins = 700 + 25 * k                         # anchor 5' of it, on the '+' strand, uniquely placed outside the repeat
        p = q + L - ins
        m1 = seqs[ch][p:p + L].upper()
        m2 = sub_at(rng, revcomp(seqs[ch][q:q + L].upper()), [15, 45])
        assert "N" not in m1 and not in_dup(ch, p, L)
        name = f"orph{k}|{ch}|{p}|{q}"
        planted.append(name + "/2")
        pe1.append((name + "/1", m1))
        pe2.append((name + "/2", m2))

    with tempfile.TemporaryDirectory() as tmp:
        fa, rd, r1, r2 = (os.path.join(tmp, n) for n in ("genome.fa", "reads.fa", "reads_1.fa", "reads_2.fa"))
        write_fasta(fa, [("pcA primer correction test sequence", a), ("pcB", b), ("pcC", c)])
        write_reads(rd, reads)
        write_reads(r1, pe1)
        write_reads(r2, pe2)
        sfx = os.path.join(tmp, "genome.sfx")
        run([REF, "index", "-i", fa, "-o", sfx, "-r", "primer", "-T4"], tmp)
        for src in (fa, rd, r1, r2, sfx):
            gz_copy(src, os.path.join(OUT, os.path.basename(src) + ".gz"))
        pe = ["-d%d" % PE_D, "-D%d" % PE_DD]
        # tag -> flags; outputs beyond the -M6 SAM; base: the run without -6 at the initial rate
        cases = {
            "s2p3": {"flags": ["-s2", "-6", "3"], "base": "b_s5", "more": ["m5bam", "m0", "m3stats"]},
            "s2p5": {"flags": ["-s2", "-6", "5"], "base": "b_s7"},
            "s12p5": {"flags": ["-s12", "-6", "5"], "base": "b_s15"},
            "s0p2": {"flags": ["-s0", "-6", "2"], "base": "b_s2"},
            "s2p3x3": {"flags": ["-s2", "-6", "3", "-x3"], "base": "b_s5"},
            "s2p3k": {"flags": ["-s2", "-6", "3", "-k10"], "base": "b_s5k"},
            "s2p3Q1": {"flags": ["-s2", "-6", "3", "-Q1"], "base": "b_s5Q1"},
            "s2p3snp": {"flags": ["-s2", "-6", "3", "-p5"], "base": "b_s5", "more": ["snp"], "m6": False},
            "U3": {"flags": ["-U3", "-s1", "-6", "3"] + pe, "base": "b_U3s4", "pe": True},
            "U2": {"flags": ["-U2", "-s1", "-6", "3"] + pe, "base": "b_U2s4", "pe": True},
            "r3": {"flags": ["-r3", "-R5", "-s2", "-6", "3"], "base": "b_r3s5"},
        }
        bases = {
            "b_s5": ["-s5"], "b_s7": ["-s7"], "b_s15": ["-s15"], "b_s2": ["-s2"], "b_s5k": ["-s5", "-k10"], "b_s5Q1": ["-s5", "-Q1"],
            "b_U3s4": ["-U3", "-s4"] + pe, "b_U2s4": ["-U2", "-s4"] + pe, "b_r3s5": ["-r3", "-R5", "-s5"],
        }

        def align(tag, flags, is_pe, fmt, ext, extra=()):
            out = os.path.join(tmp, f"{tag}.{ext}")
            cmd = [REF, "align", "-I", sfx, "-o", out, "-T4", fmt] + flags + list(extra)
            cmd += ["-i", r1, "-u", r2] if is_pe else ["-i", rd]
            return out, run(cmd, tmp)

        for tag, flags in bases.items():
            out, _ = align(tag, flags, tag.startswith("b_U"), "-M6", "m6.sam")
            gz_copy(out, os.path.join(OUT, f"{tag}.m6.sam.gz"))
            print("  ran", tag)
        for tag, cs in cases.items():
            is_pe = bool(cs.get("pe"))
            cs["counts"] = None
            if cs.get("m6", True):
                out, log = align(tag, cs["flags"], is_pe, "-M6", "m6.sam")
                gz_copy(out, os.path.join(OUT, f"{tag}.m6.sam.gz"))
                cs["counts"] = [int(x) for x in COUNTS.search(log).groups()]
                assert "correcting PCR 5' artefacts : %s" % cs["flags"][cs["flags"].index("-6") + 1] in log
            for more in cs.get("more", []):
                if more == "m5bam":
                    out, log = align(tag, cs["flags"], is_pe, "-M5", "m5.bam")
                    for e in ("", ".bai"):
                        with open(out + e, "rb") as f, open(os.path.join(OUT, f"{tag}.m5.bam{e}"), "wb") as g:
                            g.write(f.read())
                elif more == "m0":
                    out, log = align(tag, cs["flags"], is_pe, "-M0", "m0.csv")
                    gz_copy(out, os.path.join(OUT, f"{tag}.m0.csv.gz"))
                elif more == "m3stats":
                    st = os.path.join(tmp, f"{tag}.stats.csv")
                    out, log = align(tag, cs["flags"], is_pe, "-M3", "m3.csv", ["-O", st])
                    gz_copy(out, os.path.join(OUT, f"{tag}.m3.csv.gz"))
                    gz_copy(st, os.path.join(OUT, f"{tag}.m3.stats.csv.gz"))
                elif more == "snp":
                    snp = os.path.join(tmp, f"{tag}.snp.csv")
                    out, log = align(tag, cs["flags"], is_pe, "-M5", "m5.sam", ["-S", snp])
                    gz_copy(out, os.path.join(OUT, f"{tag}.m5.sam.gz"))
                    gz_copy(snp, os.path.join(OUT, f"{tag}.snp.csv.gz"))
                    assert len(open(snp).read().splitlines()) > 1, "no SNP called"
                got = [int(x) for x in COUNTS.search(log).groups()]
                assert cs["counts"] in (None, got)
                cs["counts"] = got
            print("  ran", tag, cs["counts"])
            assert cs["counts"][0] > 0 and cs["counts"][2] > 0, tag

        # the planted orphans: recovered at -s4 (cores of 20), left alone at -s1 -6 3 (cores of 30) - and not because the correction
        # pass rejected them (that would read YU:Z:NL)
        def records(path):
            return {t[0]: t for t in (l.rstrip("\n").split("\t") for l in gzip.open(path, "rt") if l[0] != "@")}

        for u in ("U3", "U2"):
            with6, base = records(os.path.join(OUT, f"{u}.m6.sam.gz")), records(os.path.join(OUT, f"b_{u}s4.m6.sam.gz"))
            differ = []
            for n in planted:
                b_rec, s_rec = base[n], with6[n]
                if not int(b_rec[1]) & 4 and int(s_rec[1]) & 4 and "YU:Z:NL" not in s_rec:
                    differ.append(n)
            print(f"  {u}: {len(differ)} of {len(planted)} planted orphans recovered at the initial rate's cores only")
            # (-U2 has no orphan recovery: nothing can differ there)
            assert len(differ) == (len(planted) if u == "U3" else 0), (u, len(differ))
            cases[u]["orphans_differ"] = sorted(differ)
        with open(os.path.join(OUT, "cases.json"), "w") as f:
            json.dump({"cases": cases, "bases": bases}, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
