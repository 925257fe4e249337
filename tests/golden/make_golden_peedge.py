#!/usr/bin/env python3
"""Generates tests/golden/peedge/: paired-end pair rules and orphan recovery at their edges (CAligner::ProcessPairedEnds, AcceptProvPE,
PEInsertSize, CSfxArrayV3::AlignPairedRead), by RUNNING THE REAL REFERENCE executable (oracle/_ref/biokanga, built by
oracle/build_ref.sh).  Run in the build container only; everything written is data.

    python tests/golden/make_golden_peedge.py

Genome (seeded): peA 7000, peB 6500, peC 6000 bases.  The first and the last 150 bases of every sequence ("end blocks") are present
twice more, on the two other sequences and well inside them: once exactly, once with the base at block offset 75 substituted.  A mate of
100 bases read from an end block therefore has two exact placements (ML); the same mate read from the substituted copy has one exact
placement and two one substitution away, and the reference accepts it as unique ("nc": beside near copies).  It does so at -e2 as well,
so no MH partner comes out of this genome.

Pairs of 2 x 100 bases, the kind in the read name:
  ins<n>fr / ins<n>rf   proper pairs with inserts exactly d-1, d, d+1, D-1, D, D+1 for (d, D) = (200, 400) and 149..151, 1149..1151 for
                        the wide runs: read 1 on '+' to the left and read 1 on '-' to the right;  ins<n>ff / ins<n>rr the same fragments
                        with both mates on one strand (proper under -E), ins<n>out with the mates facing outwards
  o<R|L><route><1|2>[s] orphan candidates: one mate unique, placed every 5 (6) bases over the 185 (270) bases before an end block (R) or
                        behind one (L) - the range over which AlignPairedRead's give-up tests and its clamp of the window at locus 0 change
                        their answer - the other inside the end block.  <1|2>: the unique mate is read 1 / read 2.  s: both mates on the
                        strand that -E pairs.  route ml: the partner from the block with 0..2 substitutions; nl: random bases; en: three
                        Ns; nc: read from the substituted copy (aligns uniquely)
  xchr / same           mates on different sequences, and on one strand, near sequence ends and inside

Runs, each -M6 with the log's NAR summary: -U1..4 at -d200 -D400 -s5; -U3 -E; -U3 -d150 -D1149 (the widest offset scan) and -D1150
(core lookups; over the pairs of core_safe() only, see RUNS); for each -U mode -Z peA and -z peA.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, gz_copy, mutate, nar_summary, rand_seq, revcomp, run, write_fasta, write_reads  # noqa: E402

OUT = os.path.join(HERE, "peedge")
LENS = {"peA": 7000, "peB": 6500, "peC": 6000}
L, BLK, NEAR_AT = 100, 150, 75
COPY_AT = ((1800, 2600), (2200, 3000))        # [first / last block][exact, substituted] copy loci on the next / next but one sequence
RUNS = [("U1", ["-U1", "-d200", "-D400", "-s5"]), ("U2", ["-U2", "-d200", "-D400", "-s5"]), ("U3", ["-U3", "-d200", "-D400", "-s5"]),
        ("U4", ["-U4", "-d200", "-D400", "-s5"]), ("U3E", ["-U3", "-d200", "-D400", "-s5", "-E"]),
        ("U3D1149", ["-U3", "-d150", "-D1149", "-s5"]), ("U3D1150", ["-U3", "-d150", "-D1150", "-s5"])]
# U3D1150 runs over the pairs of core_safe() only.  With a window of 1000 loci or more AlignPairedRead looks cores of the partner up in the
# suffix array, and where a core's hit implies a placement that ends on the last base of its sequence or beyond
# (PutHitLoci + ReadLen - PutCoreOfs >= TargSeqLen, SfxArrayV2.cpp:8361-8362) it `continue`s without advancing PutHitIdx: IterateExactsRange
# returns that hit again, for ever.  A partner planted at exactly len - 100 of its sequence is such a hit, so those pairs stay out of that run.
RUNS += [(f"U{u}ZpeA", [f"-U{u}", "-d200", "-D400", "-s5", "-Z", "peA"]) for u in (1, 2, 3, 4)]
RUNS += [(f"U{u}zpeA", [f"-U{u}", "-d200", "-D400", "-s5", "-z", "peA"]) for u in (1, 2, 3, 4)]


def core_safe(name):
    """whether the pair of this read name is part of the U3D1150 run: every pair but the orphan candidates whose partner ends on the last
    base of its sequence"""
    t = name.split("/")[0].split("_")
    return not (t[1].startswith("oR") and int(t[4]) == LENS[t[2]] - L)


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261020)
    names = list(LENS)
    seqs = {n: rand_seq(rng, ln) for n, ln in LENS.items()}
    near = {}                                       # (sequence, R|L) -> the block as its substituted copy has it
    for k, n in enumerate(names):
        for e, lo in enumerate((0, LENS[n] - BLK)):
            blk = seqs[n][lo:lo + BLK]
            nb = mutate(rng, blk, 1, [NEAR_AT])
            near[(n, "LR"[e])] = nb
            for which, (dst, txt) in enumerate(((names[(k + 1) % 3], blk), (names[(k + 2) % 3], nb))):
                at = COPY_AT[e][which]
                seqs[dst] = seqs[dst][:at] + txt + seqs[dst][at + BLK:]
    for n in names:                                 # the copies left the end blocks alone
        assert len(seqs[n]) == LENS[n]
    r1, r2, unsafe = [], [], set()

    def emit(tag, a, b):
        i = len(r1)
        r1.append((f"p{i}_{tag}/1", a))
        r2.append((f"p{i}_{tag}/2", b))

    def piece(ch, p, strand, subs=0, avoid=None):
        s = seqs[ch][p:p + L]
        assert len(s) == L and p >= 0, (ch, p)
        if subs:
            pos = [int(x) for x in rng.permutation(L) if x != avoid][:subs]
            s = mutate(rng, s, subs, pos)
        return revcomp(s) if strand == "-" else s

    # proper pairs at the exact limits, in the copy-free middle of every sequence
    for ch in names:
        for ins in (199, 200, 201, 399, 400, 401, 149, 150, 151, 1149, 1150, 1151):
            for rep in range(3 if ins in (199, 200, 201, 399, 400, 401) else 1):
                p = int(rng.integers(3300, LENS[ch] - 500 - ins))
                q = p + ins - L
                e1, e2 = int(rng.integers(0, 3)), int(rng.integers(0, 3))
                emit(f"ins{ins}fr", piece(ch, p, "+", e1), piece(ch, q, "-", e2))
                emit(f"ins{ins}rf", piece(ch, q, "-", e1), piece(ch, p, "+", e2))
                if rep == 0:
                    emit(f"ins{ins}ff", piece(ch, p, "+"), piece(ch, q, "+"))
                    emit(f"ins{ins}rr", piece(ch, q, "-"), piece(ch, p, "-"))
                    emit(f"ins{ins}out", piece(ch, p, "-"), piece(ch, q, "+"))

    # orphan candidates around the end blocks
    def orphan(ch, end, a_start, p, anchor_first, route, same):
        n = LENS[ch]
        if same:                                    # the strand of both mates that -E pairs with the anchor where it is
            s_a = s_p = ("+" if anchor_first else "-") if end == "R" else ("-" if anchor_first else "+")
        else:
            s_a, s_p = ("+", "-") if end == "R" else ("-", "+")
        anchor = piece(ch, a_start, s_a)
        blk_lo = n - BLK if end == "R" else 0
        if route == "ml":
            partner = piece(ch, p, s_p, int(rng.integers(0, 3)), avoid=NEAR_AT - (p - blk_lo))
        elif route == "nl":
            partner = rand_seq(rng, L)
        elif route == "en":
            fwd = list(seqs[ch][p:p + L])
            for k in rng.choice(L, 3, replace=False):
                fwd[k] = "N"
            fwd = "".join(fwd)
            partner = revcomp(fwd) if s_p == "-" else fwd
        else:                                       # nc
            fwd = near[(ch, end)][p - blk_lo:p - blk_lo + L]
            assert len(fwd) == L
            partner = revcomp(fwd) if s_p == "-" else fwd
        tag = f"o{end}{route}{1 if anchor_first else 2}{'s' if same else ''}_{ch}_{a_start}_{p}"
        if end == "R" and p == n - L:
            unsafe.add(len(r1))
        if anchor_first:
            emit(tag, anchor, partner)
        else:
            emit(tag, partner, anchor)

    for ch in names:
        n = LENS[ch]
        grid = [("R", a) for a in range(n - 360, n - 174, 5)] + [("L", a) for a in range(75, 346, 6)]
        for k, (end, a) in enumerate(grid):
            if end == "R":
                lo = a + 200
                p = n - BLK + int(rng.integers(0, 51)) if lo > n - L - 1 else min(n - L, max(n - BLK, lo) + int(rng.integers(0, 12)))
            else:
                hi = a + L - 1 - 200
                p = int(rng.integers(0, 51)) if hi < 0 else min(50, max(0, hi - int(rng.integers(0, 12))))
            for first in (True, False):
                orphan(ch, end, a, p, first, "ml", False)
                if k % 3 == 0:
                    orphan(ch, end, a, p, first, "ml", True)
                if k % 4 == 1:
                    for route in ("nl", "en", "nc"):
                        orphan(ch, end, a, p, first, route, False)

    # mates on different sequences and on one strand, near ends as well
    for k in range(36):
        c1, c2 = names[k % 3], names[(k + 1 + k // 18) % 3]
        p1 = 160 + 3 * k if k % 2 else int(rng.integers(3300, LENS[c1] - 700))
        p2 = LENS[c2] - BLK - L - 10 - 2 * k if k % 4 < 2 else int(rng.integers(3300, LENS[c2] - 700))
        emit("xchr", piece(c1, p1, "+-"[k % 2]), piece(c2, p2, "-+"[(k // 2) % 2]))
    for k in range(36):
        ch = names[k % 3]
        p = (160 + 4 * k, LENS[ch] - BLK - L - 260 - 3 * k, int(rng.integers(3300, LENS[ch] - 900)))[k % 3 if k < 24 else 2]
        s = "+-"[(k // 3) % 2]
        emit("same", piece(ch, p, s), piece(ch, p + 150 + 5 * k, s))
    assert len(r1) <= 1500, len(r1)

    with tempfile.TemporaryDirectory() as tmp:
        fa, f1, f2 = (os.path.join(tmp, n) for n in ("genome.fa", "reads_1.fa", "reads_2.fa"))
        write_fasta(fa, [(n, seqs[n]) for n in names])
        write_reads(f1, r1)
        write_reads(f2, r2)
        s1, s2 = os.path.join(tmp, "safe_1.fa"), os.path.join(tmp, "safe_2.fa")
        write_reads(s1, [r for i, r in enumerate(r1) if i not in unsafe])
        write_reads(s2, [r for i, r in enumerate(r2) if i not in unsafe])
        assert 0 < len(unsafe) < 200 and all(core_safe(r[0]) == (i not in unsafe) for i, r in enumerate(r1))
        sfx = os.path.join(tmp, "genome.sfx")
        run([REF, "index", "-i", fa, "-o", sfx, "-r", "peedge", "-T4"], tmp)
        for src in (fa, f1, f2, sfx):
            gz_copy(src, os.path.join(OUT, os.path.basename(src) + ".gz"))
        seen = {}
        for tag, flags in RUNS:
            out = os.path.join(tmp, f"{tag}.sam")
            i1, i2 = (s1, s2) if tag == "U3D1150" else (f1, f2)
            log = run(["timeout", "300", REF, "align", "-i", i1, "-u", i2, "-I", sfx, "-o", out, "-M6", "-T4"] + flags, tmp)
            gz_copy(out, os.path.join(OUT, f"{tag}.m6.sam.gz"))
            summ = nar_summary(log)
            with open(os.path.join(OUT, f"{tag}.nar.txt"), "w") as f:
                f.write(summ)
            cnt = {t.split()[1].strip("()"): int(t.split()[0]) for t in summ.splitlines()}
            seen[tag] = cnt
            print("  ran", tag, " ".join(f"{k}={v}" for k, v in cnt.items() if v))
        # the partner routes are what they were planted as, and every PE reason occurs somewhere
        for t in ("ML", "NL", "EN"):
            assert seen["U4"][t] > 0, t
        assert seen["U3D1150"]["AA"] > seen["U4"]["AA"] - 2 * len(unsafe)
        for t in ("FC", "UI", "OI", "UP", "IS", "IT", "NP"):
            assert any(c[t] > 0 for c in seen.values()), t
        # recoveries: -U3 accepts more than -U4 does, the wide window more still, and the scan / core branches are both in use
        assert seen["U3"]["AA"] > seen["U4"]["AA"] + 100, (seen["U3"]["AA"], seen["U4"]["AA"])
        assert seen["U3D1149"]["AA"] > seen["U4"]["AA"] + 100
        print(f"  {len(r1)} pairs")


if __name__ == "__main__":
    main()
