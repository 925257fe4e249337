#!/usr/bin/env python3
"""Generates tests/golden/constraints/: `biokanga align -5 <file>` fixtures (loci base constraints, CAligner::LoadLociConstraints and
IdentifyConstraintViolations), by RUNNING THE REAL REFERENCE executable (oracle/_ref/biokanga, built by oracle/build_ref.sh).  Run in the
build container only; everything written is data.

    python tests/golden/make_golden_constraints.py

Inputs (seeded): a genome of three sequences - lcA (28 000 bases, a lower-case stretch), "lc,B" (18 000 bases, a run of 20 Ns; its name
has to be quoted in a CSV) and lcC (10 000 bases, holding a 300-base copy of a stretch of lcA) - and main.csv, the constraints: a
header line, quoted names, blanks around fields and inside the bases field, point constraints (CT, a, ACGT), R ranges (over the N run's
edges and inside the lower-case stretch among them), nested and overlapping ranges with conflicting masks, two constraints on one
locus, locus 0 and the last locus of a sequence, one constraint inside each copy of the repeated stretch.

Reads of 50 bases tiled over every constrained stretch on both strands (written in that order, not shuffled: the files stay small),
with the target's base, another base or an N at constrained loci, so that both outcomes occur everywhere; background reads; reads with
a 3-base deletion or insertion, reads over a 300-base intron and reads with 15 bases of junk at one end, each placed so that the
constrained locus lies in the second segment / behind the trimmed end (-a, -A, -c); reads inside the repeated stretch (-r3, -r5);
pairs with one end over a constrained stretch (-U).  About 7 700 reads and 1 250 pairs: with two or three times as many the SAM files outgrow the largest file
of tests/golden/primer, which is the limit set for this directory.

cases.json: tag -> flags, reads (se / pe), the outputs written beside the -M6 SAM, and what the generator asserted of the run with the
restatement of tests/constraints_ref.py applied to the run WITHOUT -5 (<tag>.base.m6.sam.gz): the LC records are exactly the
reference's, at least 20 of them, at least 20 records touch a constraint and stay accepted, and for -a / -A / -c at least one record of
either kind is decided by its second segment or by the trim offset.  errors: one file per refusal of the loader with the reference's
messages and exit status.
"""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, gz_copy, mutate, rand_seq, revcomp, run, write_fasta, write_reads  # noqa: E402
import constraints_ref as cr  # noqa: E402
import helpers  # noqa: E402

OUT = os.path.join(HERE, "constraints")
LIMIT = max(os.path.getsize(os.path.join(HERE, "primer", f)) for f in os.listdir(os.path.join(HERE, "primer")))
NAMES = ("lcA", "lc,B", "lcC")
LENS = {"lcA": 28000, "lc,B": 18000, "lcC": 10000}
LOWER = (5000, 5400)              # of lcA
N_AT, N_LEN = 8000, 20            # of lc,B
DUP_FROM, DUP_TO, DUP_LEN = 21000, 6000, 300     # lcA[21000:21300] again at lcC[6000:6300]
L = 50
MAIN_CSV = '''"Sequence","Start","End","Bases"
# point constraints
lcA,0,0,AC
lcA,1000,1000,CT
lcA,1500,1500,a
lcA,2000,2000,ACGT
lcA,2500,2507,R
"lcA", 5100 , 5139 , r

lcA,21100,21100,G
LCA,27999,27999,"R g"
"lc,B",3000,3040,R
"lc,B",3010,3020,"A C"
"lc,B",3015,3015,T
"lc,B",3030,3060,ACG
"lc,B",7990,8030,R
"lc,B",12000,12000,CT,a fifth field
"lc,B",17999,17999,R
lcC,0,3,R
lcC,4000,4000,G
lcC,4000,4000,R
lcC,6100,6100,AT
lcC,9999,9999,	C T
'''
ERRORS = {                                           # tag -> (text, index)
    "e_fields": ("lcA,5,5,A\nlcA,6,6\n", "genome"),
    "e_name": ("Sequence,Start,End,Bases\nlcA,5,5,A\nnochr,5,5,A\n", "genome"),
    "e_neg": ("lcA,-1,5,A\n", "genome"),
    "e_order": ("lcA,5,5,A\n\nlcA,9,5,A\n", "genome"),
    "e_end": ("lcA,5,28000,A\n", "genome"),
    "e_base": ("lcA,5,5,AX\n", "genome"),
    "e_empty": ('lcA,5,5," "\n', "genome"),
    "e_loci": ("".join(f"lcA,{k},{k},A\n" for k in range(cr.MAX_LOCI + 1)), "genome"),
    "e_chroms": ("".join(f"m{k:02d},5,5,A\n" for k in range(cr.MAX_CHROMS + 1)), "many"),
}


def strip_log(log):
    return [re.sub(r"^\[[^\]]*\]\(biokanga\) ", "", ln) for ln in log.splitlines()]


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261020)
    a, b, c = (rand_seq(rng, LENS[n]) for n in NAMES)
    a = a[:LOWER[0]] + a[LOWER[0]:LOWER[1]].lower() + a[LOWER[1]:]
    b = b[:N_AT] + "N" * N_LEN + b[N_AT + N_LEN:]
    c = c[:DUP_TO] + a[DUP_FROM:DUP_FROM + DUP_LEN] + c[DUP_TO + DUP_LEN:]
    seqs = dict(zip(NAMES, (a, b, c)))
    reads = []

    def in_dup(ch, p, ln):
        return (ch == "lcA" and p < DUP_FROM + DUP_LEN and p + ln > DUP_FROM) or (ch == "lcC" and p < DUP_TO + DUP_LEN and p + ln > DUP_TO)

    def alleles(s, ch, p, sites, how):
        """the target stretch with the bases at constrained loci left alone, replaced by another base, or (one of them) by N"""
        s = list(s.upper())
        inside = [k for k in sites if p <= k < p + len(s)]
        if how == "ref" or not inside:
            return "".join(s)
        for k in (inside if len(inside) == 1 else rng.choice(inside, int(rng.integers(1, 3)), replace=False)):
            s[k - p] = "ACGT"[int(rng.integers(0, 4))]
        if how == "n":
            s[int(rng.choice(inside)) - p] = "N"
        return "".join(s)

    def emit(tag, s, strand):
        reads.append((f"{tag}{len(reads)}", revcomp(s) if strand == "-" else s))

    name_of = {n.lower(): n for n in NAMES}
    table = []
    for fields, _ in cr.csv_lines(MAIN_CSV)[1:]:
        table.append((name_of[fields[0][0].lower()], cr.atoi(fields[1][0]), cr.atoi(fields[2][0])))
    sites_of = {n: sorted({k for ch, s, e in table if ch == n for k in range(s, e + 1)}) for n in NAMES}
    stretches = sorted({(ch, min(s for c2, s, e in table if c2 == ch and s <= e0 + 60 and e >= s0 - 60),
                         max(e for c2, s, e in table if c2 == ch and s <= e0 + 60 and e >= s0 - 60)) for ch, s0, e0 in table})
    for ch, s0, e0 in stretches:                     # tiled over every constrained stretch, its edges first
        n = LENS[ch]
        starts = [s0 - L, s0 - L + 1, e0, e0 + 1] + [int(x) for x in rng.integers(s0 - L - 3, e0 + 4, 450)]
        for k, p in enumerate(sorted(starts)):
            p = max(0, min(n - L, p))
            s = seqs[ch][p:p + L]
            if in_dup(ch, p, L) or s.count("N") > 3:
                continue
            how = ("ref", "alt", "alt", "n")[k % 4]
            s = alleles(s, ch, p, sites_of[ch], how)
            if s.count("N") > 1:                     # over the N run's edge: a read may hold one N (-n1)
                s = _one_n(rng, s, int(rng.integers(0, s.count("N") + 1)))
            emit("t", s, "+-"[k % 2])
    for k in range(900):                             # background
        ch = NAMES[k % 3]
        p = int(rng.integers(0, LENS[ch] - L + 1))
        s = seqs[ch][p:p + L].upper()
        if "N" in s or in_dup(ch, p, L):
            continue
        emit("b", mutate(rng, s, int(rng.integers(0, 4))), "+-"[k % 2])
    points = [("lcA", 1000), ("lcA", 1500), ("lc,B", 12000), ("lcC", 4000), ("lcA", 2503), ("lc,B", 3015)]
    for k in range(360):                             # second segments (-a: 3 bases deleted / inserted; -A: a 300-base intron)
        ch, site = points[k % len(points)]
        kind = ("del", "ins", "jct")[k % 3]
        d = int(rng.integers(2, 22))                 # the site's offset inside the second segment (first, every fourth)
        gap = {"del": 3, "ins": 0, "jct": 300}[kind]
        half = 25 if kind != "ins" else 22
        if k % 4 == 3:
            p = site - int(rng.integers(2, 22))      # .. inside the first one
        else:
            p = site - d - gap - 25
        first, second = seqs[ch][p:p + 25], seqs[ch][p + 25 + gap:p + 25 + gap + half]
        second = alleles(second, ch, p + 25 + gap, sites_of[ch], ("ref", "alt")[k // 3 % 2])
        first = alleles(first, ch, p, sites_of[ch], ("ref", "alt")[k // 3 % 2])
        s = first.upper() + ("ACG" if kind == "ins" else "") + second
        assert len(s) == L
        emit(kind[0], s, "+-"[k // 6 % 2])
    for k in range(240):                             # chimeric (-c50): 15 bases of junk at one end
        ch, site = points[k % len(points)]
        p = site - int(rng.integers(1, 34))
        s = alleles(seqs[ch][p:p + 35], ch, p, sites_of[ch], ("ref", "alt")[k // 2 % 2])
        junk = rand_seq(rng, 15)
        s = junk + s if k % 2 else s + junk          # (in target order: which of the read's ends that is depends on the strand)
        emit("c", s, "+-"[k // 4 % 2])
    for k in range(200):                             # inside the repeated stretch (-r3 / -r5)
        p = int(rng.integers(60, 100)) + k % 3
        s = alleles(seqs["lcA"][DUP_FROM + p - L + 10:DUP_FROM + p + 10], "lcA", DUP_FROM + p - L + 10, sites_of["lcA"], ("ref", "alt")[k % 2])
        emit("m", s, "+-"[k // 2 % 2])

    pe1, pe2 = [], []
    for k in range(1500):                            # pairs: FR, inserts 150..300; the first end over a constrained stretch
        ch, s0, e0 = stretches[k % len(stretches)]
        ins = int(rng.integers(150, 301))
        p = int(rng.integers(s0 - L + 1, e0 + 1))
        if k % 2:
            p -= ins - L                             # .. or the second
        p = max(0, min(LENS[ch] - ins, p))
        frag = alleles(seqs[ch][p:p + ins], ch, p, sites_of[ch], ("ref", "alt", "alt")[k % 3])
        if "N" in frag[:L] + frag[-L:] or in_dup(ch, p, ins):
            continue
        m1, m2 = frag[:L], revcomp(frag[-L:])
        if k % 4 >= 2:
            m1, m2 = m2, m1
        pe1.append((f"p{k}/1", m1))
        pe2.append((f"p{k}/2", m2))

    with tempfile.TemporaryDirectory() as tmp:
        fa, rd, r1, r2 = (os.path.join(tmp, n) for n in ("genome.fa", "reads.fa", "reads_1.fa", "reads_2.fa"))
        write_fasta(fa, [("lcA loci constraints test sequence", a), ("lc,B", b), ("lcC", c)])
        write_reads(rd, reads)
        write_reads(r1, pe1)
        write_reads(r2, pe2)
        many = os.path.join(tmp, "many.fa")
        write_fasta(many, [(f"m{k:02d}", rand_seq(rng, 120)) for k in range(cr.MAX_CHROMS + 2)])
        sfx, many_sfx = os.path.join(tmp, "genome.sfx"), os.path.join(tmp, "many.sfx")
        run([REF, "index", "-i", fa, "-o", sfx, "-r", "constraints", "-T4"], tmp)
        run([REF, "index", "-i", many, "-o", many_sfx, "-r", "many", "-T4"], tmp)
        with open(os.path.join(tmp, "main.csv"), "w") as f:
            f.write(MAIN_CSV)
        for src in (fa, rd, r1, r2, sfx, many_sfx, os.path.join(tmp, "main.csv")):
            gz_copy(src, os.path.join(OUT, os.path.basename(src) + ".gz"))
        print(f"  {len(reads)} reads, {len(pe1)} pairs")

        g = cr.Genome(os.path.join(OUT, "genome.fa.gz"))
        tab = cr.load_constraints(os.path.join(tmp, "main.csv"), list(NAMES), [LENS[n] for n in NAMES])
        pe = ["-d100", "-D400"]
        cases = {
            "s3": {"flags": ["-s3"], "more": ["m5bam", "m0"]},
            "c50": {"flags": ["-s3", "-c50"], "decides": "trim"},
            "a5": {"flags": ["-s3", "-a5"], "decides": "seg"},
            # (-A forces the flank trimmer, which runs behind the pass: its clips are put back, and the reads it removed - unaligned in the run
            # without -5 - are left out of the comparison)
            "A1000": {"flags": ["-s3", "-A1000"], "decides": "seg", "untrim": True},
            "r3": {"flags": ["-s3", "-r3", "-R5"]},
            # (-T1: the reference numbers -r5's records as its threads make them, and equal records come out in that order)
            "r5": {"flags": ["-s3", "-r5", "-R5", "-T1"]},
            "U3": {"flags": ["-U3", "-s3"] + pe, "pe": True},
            "U2": {"flags": ["-U2", "-s3"] + pe, "pe": True},
            # (-k, -6, -x and -Z's filter run behind the constraint pass and turn records of the run without -5 into unaligned ones, which
            # say nothing of where they lay: the pass of these runs sees the records of s3's, and is replayed from them)
            "k": {"flags": ["-s3", "-k10"], "replay": "s3"},
            "p6": {"flags": ["-s1", "-6", "2"], "replay": "s3"},
            "x3": {"flags": ["-s3", "-x3"], "replay": "s3"},
            "Z": {"flags": ["-s3", "-Z", "lcC"], "replay": "s3"},
            # (the reference takes -p with -M0 .. -M5 only: the -M5 SAM and the SNP file, the latter also from the run without -5)
            "snp": {"flags": ["-s3", "-p5"], "more": ["snp"], "m6": False, "replay": "s3"},
        }

        def align(tag, flags, is_pe, fmt, ext, extra=(), with5=True):
            out = os.path.join(tmp, f"{tag}.{ext}")
            cmd = [REF, "align", "-I", sfx, "-o", out, fmt] + ([] if "-T1" in flags else ["-T4"]) + flags + list(extra) + (["-5", "main.csv"] if with5 else [])
            cmd += ["-i", r1, "-u", r2] if is_pe else ["-i", rd]
            return out, run(cmd, tmp)

        def put(src, name):
            dst = os.path.join(OUT, name)
            if name.endswith(".gz"):
                gz_copy(src, dst)
            else:
                with open(src, "rb") as f, open(dst, "wb") as h:
                    h.write(f.read())
            assert os.path.getsize(dst) <= LIMIT, (name, os.path.getsize(dst), LIMIT)

        for tag, cs in cases.items():
            is_pe = bool(cs.get("pe"))
            if not cs.get("m6", True):
                snp0, snp = os.path.join(tmp, f"{tag}.base.snp.csv"), os.path.join(tmp, f"{tag}.snp.csv")
                align(tag + ".base", cs["flags"], is_pe, "-M5", "m5.sam", ["-S", snp0], with5=False)
                o, log = align(tag, cs["flags"], is_pe, "-M5", "m5.sam", ["-S", snp])
                put(snp0, f"{tag}.base.snp.csv.gz")
                put(o, f"{tag}.m5.sam.gz")
                put(snp, f"{tag}.snp.csv.gz")
                assert len(open(snp).read().splitlines()) > 1, "no SNP called"
                assert open(snp).read() != open(snp0).read(), "the constraints do not reach the SNP caller"
                # its records are the aligned ones of the replayed run's -M6 SAM
                _, mine = helpers.parse_sam(o)
                _, full = helpers.parse_sam(os.path.join(OUT, cs["replay"] + ".m6.sam.gz"))
                assert sorted(r["qname"] for r in mine) == sorted(r["qname"] for r in full if not r["flag"] & 4)
                cs["identified"] = int(next(re.match(r"Identified (\d+) ", ln).group(1) for ln in strip_log(log) if ln.startswith("Identified ")))
                assert cs["identified"] == cases[cs["replay"]]["identified"]
                print("  ran", tag, cs["identified"])
                continue
            out0, _ = align(tag + ".base", cs["flags"], is_pe, "-M6", "m6.sam", with5=False)
            put(out0, f"{tag}.base.m6.sam.gz")
            out, log = align(tag, cs["flags"], is_pe, "-M6", "m6.sam")
            put(out, f"{tag}.m6.sam.gz")
            lines = strip_log(log)
            assert "Loci base constraints file: 'main.csv'" in log
            assert f"Identifying {'PE' if is_pe else 'SE'} loci base constraint violations ..." in lines
            cs["identified"] = int(next(re.match(r"Identified (\d+) ", ln).group(1) for ln in lines if ln.startswith("Identified ")))
            for more in cs.get("more", []):
                if more == "m5bam":
                    o, _ = align(tag, cs["flags"], is_pe, "-M5", "m5.bam")
                    put(o, f"{tag}.m5.bam")
                    put(o + ".bai", f"{tag}.m5.bam.bai")
                elif more == "m0":
                    o, _ = align(tag, cs["flags"], is_pe, "-M0", "m0.csv")
                    put(o, f"{tag}.m0.csv.gz")
            # the restatement over the run without -5 against what the reference made of it
            _, base = helpers.parse_sam(os.path.join(OUT, cs.get("replay", tag) + ".base.m6.sam.gz"))
            _, with5 = helpers.parse_sam(out)
            lc, stay = cr.replay(g, tab, base, is_pe, untrim=bool(cs.get("untrim")))
            ref_lc = cr.lc_records(with5, base if cs.get("untrim") else None)
            assert lc == ref_lc, (tag, len(lc), len(ref_lc), sorted(set(lc) ^ set(ref_lc))[:10])
            cs["lc"], cs["stay"] = len(lc), len(stay)
            assert cs["lc"] >= 20 and cs["stay"] >= 20, (tag, cs["lc"], cs["stay"])
            if cs.get("decides"):
                # .. and how many of either kind the second segment / the trim offset decides: -a, -A: violated by the second segment alone;
                # accepted with only the second segment over a constraint.  -c: the other outcome when the read is indexed without the offset
                n_lc = n_stay = 0
                for r in base:
                    if r["flag"] & 4:
                        continue
                    segs = cr.sam_segments(r, bool(cs.get("untrim")))
                    other = segs[:1] if cs["decides"] == "seg" else [(s, n, 0) for s, n, _ in segs]
                    if other == segs:
                        continue
                    codes = cr.LUT[np.frombuffer(r["seq"].encode(), dtype=np.uint8)]
                    ok, touched = cr.accept_segments(g, tab, g.ids[r["rname"]], "+", codes, segs)
                    ok2, touched2 = cr.accept_segments(g, tab, g.ids[r["rname"]], "+", codes, other)
                    if cs["decides"] == "seg":
                        n_lc += not ok and ok2
                        n_stay += ok and touched and not touched2
                    elif ok != ok2:
                        n_lc += not ok
                        n_stay += ok
                cs["decided_lc"], cs["decided_stay"] = n_lc, n_stay
                assert n_lc >= 1 and n_stay >= 1, (tag, n_lc, n_stay)
            print("  ran", tag, {k: v for k, v in cs.items() if k not in ("flags", "more")})

        errors = {}
        for tag, (text, index) in ERRORS.items():
            with open(os.path.join(tmp, tag + ".csv"), "w") as f:
                f.write(text)
            gz_copy(os.path.join(tmp, tag + ".csv"), os.path.join(OUT, tag + ".csv.gz"))
            errors[tag] = {"index": index, "file": tag + ".csv"}
        errors["e_missing"] = {"index": "genome", "file": "missing.csv"}
        for tag, e in errors.items():
            r = subprocess.run([REF, "align", "-I", sfx if e["index"] == "genome" else many_sfx, "-o", os.path.join(tmp, "e.sam"), "-T4", "-M6", "-s3", "-i", rd, "-5", e["file"]],
                               cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            lines = strip_log(r.stdout)
            at = next(i for i, ln in enumerate(lines) if ln.startswith("Loading loci base constraints"))
            e["messages"] = [ln for ln in lines[at + 1:] if ln and not ln.startswith("Exit code") and not ln.startswith("[")]
            e["exit"] = r.returncode
            assert e["messages"][-1] == "Unable to load loci constraints" and r.returncode != 0, (tag, lines[-6:])
            # the loader's restatement refuses the file with the same words
            names, lens = (list(NAMES), [LENS[n] for n in NAMES]) if e["index"] == "genome" else ([f"m{k:02d}" for k in range(cr.MAX_CHROMS + 2)], [120] * (cr.MAX_CHROMS + 2))
            try:
                cwd = os.getcwd()
                os.chdir(tmp)
                cr.load_constraints(e["file"], names, lens)
                raise SystemExit(f"{tag}: the restatement accepts the file")
            except cr.LoadError as err:
                assert str(err) == e["messages"][-2], (tag, str(err), e["messages"])
            finally:
                os.chdir(cwd)
            print("  refused", tag, e["messages"][-2])
        with open(os.path.join(OUT, "cases.json"), "w") as f:
            json.dump({"cases": cases, "errors": errors}, f, indent=1, sort_keys=True)
            f.write("\n")


def _one_n(rng, s, keep):
    """the Ns of a stretch over the run's edge replaced by bases, the keep-th (1..) left in; keep 0: none left"""
    out, i = [], 0
    for ch in s:
        if ch == "N":
            i += 1
            out.append("N" if i == keep else "ACGT"[int(rng.integers(0, 4))])
        else:
            out.append(ch)
    return "".join(out)


if __name__ == "__main__":
    main()
