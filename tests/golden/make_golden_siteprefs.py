#!/usr/bin/env python3
"""Generates tests/golden/siteprefs/: `biokanga align -8 <file> [-9 <ofs>]` fixtures (start-site octamer preferences), by RUNNING THE
REAL REFERENCE executable (oracle/_ref/biokanga, built by oracle/build_ref.sh).  Run in the build container only; everything written is data.

    python tests/golden/make_golden_siteprefs.py

Inputs (seeded): a genome of two sequences (35 000 + 25 000 bases; 20 Ns in the first - short enough that the indexer leaves the run alone,
so the .sfx holds the FASTA's bases) and about 3 000 reads of 60 bases, among them on purpose
  * reads on both strands at the very ends of both sequences (the end clamp),
  * '+' reads at loci 0..3 of the SECOND sequence (with -9 -4 the site wraps: the reference goes on with the buffer the last read of the
    first sequence left),
  * reads whose octamer window overlaps the N run (skipped),
  * several reads sharing one start (NumOccs > NumSites), exact duplicates,
  * a '+' and a '-' read whose sites coincide, next to each other in the sorted order, for each offset the runs use,
  * no '+' read in the first 150 bases of the first sequence, a '-' read at its locus 0: the first visited read of every run is in range.
cases.json lists the runs: tag -> flags / offset / output kind / whose table (prefs) / paired reads; per run its SAM / BED / CSV and, where
the table differs from the default run's, <tag>.siteprefs.csv.gz.
"""
import gzip
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, gz_copy, mutate, rand_seq, revcomp, run, write_fasta, write_reads  # noqa: E402

OUT = os.path.join(HERE, "siteprefs")
L = 60
LEN_A, LEN_B = 35000, 25000
N_AT, N_LEN = 12000, 20
QUIET = (20000, 22000)            # of the second sequence: only the planted coinciding-site reads lie here


def site_of(loci, length, strand, ofs, chrom_len):
    """the reference's UINT32 HitLoci arithmetic (Aligner.cpp:8130-8146)"""
    s = (loci + ofs) if strand == "+" else (loci + length - 1 - ofs - 7)
    s &= 0xffffffff
    if ((s + 8) & 0xffffffff) >= chrom_len:
        s = (chrom_len - 9) & 0xffffffff
    return s


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261018)
    a, b = rand_seq(rng, LEN_A), rand_seq(rng, LEN_B)
    a = a[:N_AT] + "N" * N_LEN + a[N_AT + N_LEN:]
    seqs = {"spA": a, "spB": b}
    reads = []

    def add(tag, c, p, strand, subs=0):
        s = seqs[c][p:p + L]
        assert len(s) == L and "N" not in s, (tag, c, p)
        r = mutate(rng, s, subs) if subs else s
        reads.append((f"{tag}{len(reads)}|{c}|{p}|{strand}", revcomp(r) if strand == "-" else r))

    for _ in range(2500):                         # background
        c = "spA" if rng.integers(0, 7) < 4 else "spB"
        n = len(seqs[c])
        p = int(rng.integers(0, n - L + 1))
        strand = "+-"[int(rng.integers(0, 2))]
        if "N" in seqs[c][p:p + L]:
            continue
        if c == "spA" and p < 150 and strand == "+":
            continue
        if c == "spB" and (p < 8 or QUIET[0] - L <= p < QUIET[1]):
            continue
        add("r", c, p, strand, int(rng.integers(0, 3)))
    for c, n in (("spA", LEN_A), ("spB", LEN_B)):  # the ends of both sequences, both strands
        for d in (0, 1, 2, 5, 9):
            add("end", c, n - L - d, "+")
            add("end", c, n - L - d, "-")
    add("first", "spA", 0, "-")
    add("first", "spA", 5, "-")
    for p in (150, 153):
        add("start", "spA", p, "+")
    for p in (0, 1, 2, 3, 4, 6):                   # loci 0..3 of the second sequence: the wrapped sites
        add("wrap", "spB", p, "+")
    add("wrap", "spB", 2, "-")
    for d in (0, 1, 3):                            # windows over the N run
        add("nwin", "spA", N_AT + N_LEN + d, "+")
        add("nwin", "spA", N_AT - L - d, "-")
        add("nwin", "spA", N_AT + N_LEN + d, "-")
        add("nwin", "spA", N_AT - L - d, "+")
    for k in range(40):                            # several reads sharing one start
        c = "spA" if k % 2 else "spB"
        p = 1000 + 397 * k
        strand = "+-"[k % 3 == 0]
        for j in range(2 + k % 3):
            add("occ", c, p, strand, j % 3)
    for k in range(12):                            # exact duplicates
        p = 3000 + 911 * k
        for j in range(2):
            reads.append((f"dup{len(reads)}|{j}", seqs["spA"][p:p + L]))
    # '+' at q and '-' at q - d share their site under offset ofs when d = L - 8 - 2 * ofs; nothing else lies between them
    for k, ofs in enumerate((-4, 0, 7, -100)):
        d = L - 8 - 2 * ofs
        q = QUIET[0] + 400 * k + 300
        add("co", "spB", q, "+")
        add("co", "spB", q - d, "-")
        add("co", "spB", q - d, "-", 1)
        assert site_of(q, L, "+", ofs, LEN_B) == site_of(q - d, L, "-", ofs, LEN_B)
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    # pairs for the -U3 run: FR, inserts 200..400, away from the sequences' starts
    pe1, pe2 = [], []
    for k in range(300):
        c = "spA" if k % 2 else "spB"
        n = len(seqs[c])
        ins = int(rng.integers(200, 401))
        p = int(rng.integers(200, n - ins))
        frag = seqs[c][p:p + ins]
        if "N" in frag:
            continue
        m1, m2 = mutate(rng, frag[:L], k % 3), revcomp(frag[-L:])
        if k % 4 == 0:
            m1, m2 = m2, m1
        pe1.append((f"p{k}|{c}|{p}/1", m1))
        pe2.append((f"p{k}|{c}|{p}/2", m2))

    with tempfile.TemporaryDirectory() as tmp:
        fa, rd, r1, r2 = (os.path.join(tmp, n) for n in ("genome.fa", "reads.fa", "reads_1.fa", "reads_2.fa"))
        write_fasta(fa, [("spA site preference test sequence", a), ("spB", b)])
        write_reads(rd, reads)
        write_reads(r1, pe1)
        write_reads(r2, pe2)
        sfx = os.path.join(tmp, "genome.sfx")
        run([REF, "index", "-i", fa, "-o", sfx, "-r", "siteprefs", "-T4"], tmp)
        for src in (fa, rd, r1, r2, sfx):
            gz_copy(src, os.path.join(OUT, os.path.basename(src) + ".gz"))
        cases = {
            "dflt": {"flags": ["-s3", "-M5"], "ofs": -4, "out": "sam"},
            "ofs0": {"flags": ["-s3", "-M5", "-9", "0"], "ofs": 0, "out": "sam"},
            "ofs7": {"flags": ["-s3", "-M5", "-9", "7"], "ofs": 7, "out": "sam"},
            "ofsm100": {"flags": ["-s3", "-M5", "-9", "-100"], "ofs": -100, "out": "sam"},
            "m4": {"flags": ["-s3", "-M4"], "ofs": -4, "out": "bed"},
            "m0": {"flags": ["-s3", "-M0"], "ofs": -4, "out": "csv"},
            "x3": {"flags": ["-s3", "-M5", "-x3"], "ofs": -4, "out": "sam"},
            "U3": {"flags": ["-s3", "-M5", "-U3", "-d150", "-D450"], "ofs": -4, "out": "sam", "pe": True},
        }
        lens = {"spA": LEN_A, "spB": LEN_B}
        sams, tables = {}, {}
        for tag, c in cases.items():
            out = os.path.join(tmp, f"{tag}.{c['out']}")
            prefs = os.path.join(tmp, f"{tag}.siteprefs.csv")
            cmd = [REF, "align", "-I", sfx, "-o", out, "-T4", "-8", prefs] + c["flags"]
            cmd += ["-i", r1, "-u", r2] if c.get("pe") else ["-i", rd]
            run(cmd, tmp)
            # the first visited read - the first record written - is in range; 64 octamers and more have hits on either strand
            with open(out) as f:
                for line in f:
                    if line.startswith(("@", "track")):
                        continue
                    if c["out"] == "sam":
                        t = line.split("\t")
                        chrom, loci, strand, length = t[2], int(t[3]) - 1, "-" if int(t[1]) & 16 else "+", len(t[9])
                    elif c["out"] == "bed":
                        t = line.split("\t")
                        chrom, loci, strand, length = t[0], int(t[1]), t[5].strip(), int(t[2]) - int(t[1])
                    else:
                        t = line.split(",")
                        chrom, loci, strand, length = t[3].strip('"'), int(t[4]), t[7].strip('"'), int(t[6])
                    break
            if tag != "x3":                        # (-x moves the written start; the run's reads are the default run's)
                assert site_of(loci, length, strand, c["ofs"], lens[chrom]) < lens[chrom], (tag, chrom, loci, strand)
            rows = open(prefs).read().splitlines()[1:]
            assert len(rows) == 2 * 0xffff
            for s in ('"+"', '"-"'):
                hit = sum(1 for r in rows if r.split(",")[1] == s and int(r.split(",")[3]) > 0)
                assert hit >= 64, (tag, s, hit)
                print(f"  {tag} {s}: {hit} octamers with hits")
            table = open(prefs, "rb").read()
            if tag in ("m4", "m0"):                # the output format changes nothing in the table: the default run's serves
                assert table == tables["dflt"]
                c["prefs"] = "dflt"
            else:
                tables[tag] = table
                c["prefs"] = tag
                with gzip.GzipFile(os.path.join(OUT, f"{tag}.siteprefs.csv.gz"), "wb", 9, mtime=0) as g:
                    g.write(table)
            if c["out"] == "sam" and not c.get("pe") and tag != "x3":
                sams[tag] = open(out, "rb").read()
                if tag != "dflt":                  # -9 changes nothing but the table: one SAM serves the four runs
                    assert sams[tag] == sams["dflt"]
                    continue
            gz_copy(out, os.path.join(OUT, f"{tag}.{c['out']}.gz"))
            print("  ran", tag)
        # the default run's SAM without -8: the option leaves it alone
        out = os.path.join(tmp, "plain.sam")
        run([REF, "align", "-I", sfx, "-o", out, "-T4", "-i", rd, "-s3", "-M5"], tmp)
        assert open(out, "rb").read() == sams["dflt"]
        with open(os.path.join(OUT, "cases.json"), "w") as f:
            json.dump(cases, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
