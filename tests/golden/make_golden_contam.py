#!/usr/bin/env python3
"""Generates tests/golden/contam/: `biokanga align -H <contaminants.fa>` fixtures, by RUNNING THE REAL REFERENCE executable
(oracle/_ref/biokanga, built by oracle/build_ref.sh) over the genome, .sfx and reads of tests/golden/basic (and the mates of tests/golden/pe).
Run in the build container only; everything written is data.

    python tests/golden/make_golden_contam.py

Inputs (seeded): reads of the basic fixture with adaptor ends glued on - whole, partial, with one and with two substitutions, with an N
inside the overlap - beside clean ones, reads that pass -l only before the contaminant cut, reads shorter than the 20 bases the matcher
looks at, 250-base reads for a set of 300 entries of 4..200 bases, a FASTQ copy, tagged mates.  cases.json lists the runs: tag ->
reads / mates / contaminants file / flags; per run <tag>.m6.sam.gz, <tag>.nar.txt and <tag>.contam.txt (the reference's contaminant log lines).
"""
import gzip
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, gz_copy, mutate, nar_summary, rand_seq, revcomp, run  # noqa: E402

OUT = os.path.join(HERE, "contam")


def read_fa(path):
    recs, name, seq = [], None, []
    with gzip.open(path, "rt") as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                if name is not None:
                    recs.append((name, "".join(seq)))
                name, seq = line[1:], []
            else:
                seq.append(line)
    if name is not None:
        recs.append((name, "".join(seq)))
    return recs


def write_fa(path, recs):
    with open(path, "w") as f:
        for name, seq in recs:
            f.write(">" + name + "\n" + seq + "\n")


def tag_read(rng, seq, a5, a3, kind):
    """glue the last k5 bases of a5 in front and the first k3 bases of a3 behind; kind picks what is done to the glued ends"""
    k5 = len(a5) if kind == "whole" else int(rng.integers(3, len(a5) + 1))
    k3 = len(a3) if kind == "whole" else int(rng.integers(3, len(a3) + 1))
    e5, e3 = a5[len(a5) - k5:], a3[:k3]
    if kind == "sub1":
        e5, e3 = mutate(rng, e5, 1), mutate(rng, e3, 1)
    elif kind == "sub2":
        e5, e3 = mutate(rng, e5, 2), mutate(rng, e3, 2)
    elif kind == "n":
        p, q = int(rng.integers(0, k5)), int(rng.integers(0, k3))
        e5, e3 = e5[:p] + "N" + e5[p + 1:], e3[:q] + "N" + e3[q + 1:]
    elif kind == "only5":
        e3 = ""
    elif kind == "only3":
        e5 = ""
    return e5 + seq + e3


def contam_lines(log):
    out = []
    for line in log.splitlines():
        msg = line.split("](biokanga) ", 1)[-1]
        if "contaminate trimmed" in msg or "contaminant trimmed" in msg or msg.startswith("Contaminant sequences file"):
            out.append(msg.strip())
    return "\n".join(out) + "\n"


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261017)
    basic, pe = os.path.join(HERE, "basic"), os.path.join(HERE, "pe")
    A5, A3 = rand_seq(rng, 33), rand_seq(rng, 34)
    B5, B3 = rand_seq(rng, 21), rand_seq(rng, 58)
    kinds = ["whole", "part", "sub1", "sub2", "n", "only5", "only3", "clean", "part", "sub1"]
    src = [(n, s) for n, s in read_fa(os.path.join(basic, "reads.fa.gz")) if len(s) >= 50]
    pick = rng.choice(len(src), 1200, replace=False)
    reads = []
    for j, i in enumerate(sorted(pick)):
        name, seq = src[i]
        kind = kinds[j % len(kinds)]
        reads.append((name.split()[0] + "_" + kind, seq if kind == "clean" else tag_read(rng, seq, A5, A3, kind)))
    # pass -l50 only before the contaminant cut: 40 genome bases + 12 of the adaptor
    for j in range(40):
        reads.append((f"lenedge{j}", A5[-12:] + src[int(rng.integers(0, len(src)))][1][:40 + j % 3]))
    # shorter than 20 bases: loaded with -l15, never matched
    for j in range(40):
        reads.append((f"short{j}", A5[-6:] + src[int(rng.integers(0, len(src)))][1][:9 + j % 5]))
    # .. and exactly 20 / 21: matched
    for j in range(10):
        reads.append((f"twenty{j}", A5[-6:] + src[int(rng.integers(0, len(src)))][1][:14 + j % 2]))
    with tempfile.TemporaryDirectory() as tmp:
        def unz(s, d):
            with gzip.open(s, "rb") as f, open(d, "wb") as g:
                g.write(f.read())
        sfx = os.path.join(tmp, "genome.sfx")
        unz(os.path.join(basic, "genome.sfx.gz"), sfx)
        genome = read_fa(os.path.join(basic, "genome.fa.gz"))
        files = {}

        def put(name, recs, fastq=False):
            p = os.path.join(tmp, name)
            if fastq:
                with open(p, "w") as f:
                    for n, s in recs:
                        f.write("@" + n + "\n" + s + "\n+\n" + "".join(chr(33 + int(q)) for q in rng.integers(2, 41, len(s))) + "\n")
            else:
                write_fa(p, recs)
            gz_copy(p, os.path.join(OUT, name + ".gz"))
            files[name] = p
            return p

        put("reads.fa", reads)
        put("reads.fq", reads[:600], fastq=True)
        # 250-base reads for the large set
        long_reads = []
        for j in range(400):
            g = genome[j % len(genome)][1].upper()
            at = int(rng.integers(0, len(g) - 260))
            seq = g[at:at + 250 - 66]
            if "N" in seq:
                continue
            long_reads.append((f"long{j}_{kinds[j % len(kinds)]}", seq if kinds[j % len(kinds)] == "clean" else tag_read(rng, seq, A5, A3, kinds[j % len(kinds)])))
        put("long.fa", long_reads)
        # mates: the pe fixture's first 800 pairs, PE1 tagged with A5 / A3, PE2 with B5 / B3
        m1, m2 = read_fa(os.path.join(pe, "reads_1.fa.gz"))[:800], read_fa(os.path.join(pe, "reads_2.fa.gz"))[:800]
        t1 = [(n, s if kinds[j % len(kinds)] == "clean" else tag_read(rng, s, A5, A3, kinds[j % len(kinds)])) for j, (n, s) in enumerate(m1)]
        t2 = [(n, s if kinds[(j + 3) % len(kinds)] == "clean" else tag_read(rng, s, B5, B3, kinds[(j + 3) % len(kinds)])) for j, (n, s) in enumerate(m2)]
        put("pe_1.fa", t1)
        put("pe_2.fa", t2)
        # the contaminants files (committed as they are: small)
        def contam(name, recs):
            p = os.path.join(OUT, name)
            write_fa(p, recs)
            return p
        a5n = A5[:20] + "N" + A5[21:27] + "N" + A5[28:]
        a3n = A3[:3] + "N" + A3[4:15] + "n" + A3[16:]
        many = [("A5@1", A5), ("A3@3", A3)]
        seen = {A5, A3}
        for j in range(300):
            s = rand_seq(rng, int(rng.integers(4, 201)))
            if s in seen or revcomp(s) in seen:
                continue
            seen.add(s)
            many.append((f"m{j}@{['1', '3', '13', '24', '57', '1234'][j % 6]}", s))
        cfiles = {
            "ad13.fa": contam("ad13.fa", [("A5@1 five prime", A5), ("A3@3", A3.lower())]),
            "names.fa": contam("names.fa", [("plain", A5), ("ad12", rand_seq(rng, 40)), ("x@19", rand_seq(rng, 25)), ("77", rand_seq(rng, 12)),
                                            ("tail@", rand_seq(rng, 9)), ("t@3", A3)]),
            "rc57.fa": contam("rc57.fa", [("A5rc@57", revcomp(A5)), ("A3rc@7", revcomp(A3))]),
            "nn.fa": contam("nn.fa", [("A5n@1", a5n), ("A3n@3", a3n)]),
            "pe.fa": contam("pe.fa", [("A5@1", A5), ("A3@3", A3), ("B5@2", B5), ("B3@4", B3)]),
            "many.fa": contam("many.fa", many),
        }
        cases = {
            "se13": {"reads": "reads.fa", "contaminants": "ad13.fa", "flags": ["-s3"]},
            "se13y3Y5": {"reads": "reads.fa", "contaminants": "ad13.fa", "flags": ["-s3", "-y3", "-Y5"]},
            "se13l15": {"reads": "reads.fa", "contaminants": "ad13.fa", "flags": ["-s3", "-l15"]},
            "se13n2": {"reads": "reads.fa", "contaminants": "ad13.fa", "flags": ["-s3", "-#2"]},
            "names": {"reads": "reads.fa", "contaminants": "names.fa", "flags": ["-s3"]},
            "rc57": {"reads": "reads.fa", "contaminants": "rc57.fa", "flags": ["-s3"]},
            "nn": {"reads": "reads.fa", "contaminants": "nn.fa", "flags": ["-s3"]},
            "fqg0": {"reads": "reads.fq", "contaminants": "ad13.fa", "flags": ["-s3", "-g0"]},
            "pe24": {"reads": "pe_1.fa", "mates": "pe_2.fa", "contaminants": "pe.fa", "flags": ["-U3", "-d200", "-D400", "-s5"]},
            "many": {"reads": "long.fa", "contaminants": "many.fa", "flags": ["-s3"]},
        }
        for tag, c in cases.items():
            out = os.path.join(tmp, tag + ".sam")
            cmd = [REF, "align", "-i", files[c["reads"]], "-I", sfx, "-o", out, "-M6", "-T4", "-H", cfiles[c["contaminants"]]] + c["flags"]
            if "mates" in c:
                cmd += ["-u", files[c["mates"]]]
            log = run(cmd, tmp)
            gz_copy(out, os.path.join(OUT, tag + ".m6.sam.gz"))
            with open(os.path.join(OUT, tag + ".nar.txt"), "w") as f:
                f.write(nar_summary(log))
            with open(os.path.join(OUT, tag + ".contam.txt"), "w") as f:
                f.write(contam_lines(log).replace(os.path.dirname(cfiles[c["contaminants"]]) + os.sep, ""))
            print("  ran", tag)
        with open(os.path.join(OUT, "cases.json"), "w") as f:
            json.dump(cases, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
