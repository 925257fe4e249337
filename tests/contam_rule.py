"""A plain Python statement of `align -H`'s contaminant rule (what CContaminants::LoadContaminantsFile / MatchContaminants and the loader of
CAligner::LoadRawReads come to), for the tests: the contaminants file's entries, the cut of a read end, the loader's acceptance."""
import gzip
import json
import os

import helpers

CONTAM = os.path.join(helpers.GOLDEN, "contam")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def cases():
    return json.load(open(os.path.join(CONTAM, "cases.json")))


def norm(seq):
    """bases as the matcher sees them: a,c,g,t in either case, everything else N"""
    return "".join(c if c in "ACGT" else "N" for c in seq.upper())


def revcomp(s):
    return "".join(COMP.get(c, "N") for c in reversed(s))


def read_fasta(path):
    recs, name, seq = [], None, []
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rt") as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                if name is not None:
                    recs.append((name, "".join(seq)))
                name, seq = line[1:], []
            else:
                seq.append(line.strip())
    if name is not None:
        recs.append((name, "".join(seq)))
    return recs


def read_fastq(path):
    lines = gzip.open(path, "rt").read().split("\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def name_codes(descr):
    """(name, codes) of a record: the scan of Contaminants.cpp:280-292; codes None = a vector ('&') record"""
    tok = descr.split()
    if not tok:
        return None, {1, 2, 5, 6}
    name = tok[0]
    p = len(name) - 1
    idx = len(name)
    while idx > 1:
        if name[p] in "@&" or not ("1" <= name[p] <= "8"):
            break
        idx -= 1
        p -= 1
    if name[p] == "&":
        return name, None
    if name[p] == "@" and p + 1 < len(name):
        return name[:p], {int(c) for c in name[p + 1:] if "1" <= c <= "8"}
    return name, {1, 2, 5, 6}


def entries(path):
    """[(use 1..4, sequence)] in the reference's order; ValueError for what the reference (or this project) refuses"""
    out, names = [], []
    for descr, seq in read_fasta(path):
        name, codes = name_codes(descr)
        if codes is None:
            raise ValueError("vector contaminant")
        if name == "":
            raise ValueError("no name")
        seq = norm(seq)
        if not 4 <= len(seq) <= 200:
            raise ValueError("length")
        for u in (1, 2, 3, 4):
            if u in codes:
                out.append((u, seq))
                names.append(name.lower())
        for u in (1, 2, 3, 4):
            if u + 4 in codes:
                out.append((u, revcomp(seq)))
                names.append(name.lower() + "xrc")
    for k, (u, s) in enumerate(out):
        if any(u == v and (s == t or names[k] == names[j]) for j, (v, t) in enumerate(out[:k])):
            raise ValueError("duplicate")
    if len(out) > 1600:
        raise ValueError("too many")
    return out


def mismatches(read_part, contam_part, stop=2):
    n = 0
    for r, c in zip(read_part, contam_part):
        if r == "N" or (c != "N" and c != r):
            n += 1
            if n >= stop:
                break
    return n


def overlap(read, ents, use, trim):
    """the cut beyond the fixed trim of one read end: the rule of the issue, word for word"""
    n = len(read)
    seqs = [s for u, s in ents if u == use]
    if not seqs or n < 20 or n > 2000:
        return 0
    five = use in (1, 2)
    for L in range(min(n, max(len(s) for s in seqs)), trim, -1):
        part = read[:L] if five else read[n - L:]
        for s in seqs:
            if len(s) >= L and mismatches(part, s[len(s) - L:] if five else s[:L]) <= 1:
                return L - trim
    return 0


def cuts(read, ents, pe2=False, trim5=0, trim3=0):
    read = norm(read)
    return overlap(read, ents, 2 if pe2 else 1, trim5), overlap(read, ents, 4 if pe2 else 3, trim3)


def flag_value(flags, opt, dflt):
    for f in flags:
        if f.startswith(opt) and f[len(opt):].isdigit():
            return int(f[len(opt):])
    return dflt


def expected_store(case):
    """what the loader keeps of a case's reads: [(name, trimmed text, trimmed scores or None, mate 0|1)], and the four trimmed counts"""
    ents = entries(os.path.join(CONTAM, case["contaminants"]))
    fl = case["flags"]
    t5, t3, mn, mx = flag_value(fl, "-y", 0), flag_value(fl, "-Y", 0), flag_value(fl, "-l", 50), flag_value(fl, "-L", 500)

    def load(fn):
        p = os.path.join(CONTAM, fn + ".gz")
        return read_fastq(p) if fn.endswith(".fq") else [(n, s, None) for n, s in read_fasta(p)]
    files = [load(case["reads"])] + ([load(case["mates"])] if "mates" in case else [])
    kept, counts = [], [0, 0, 0, 0]
    nth = flag_value(fl, "-#", 1)                       # every nth raw read (or pair), starting with the first
    for recs in list(zip(*files))[::nth]:
        cs = [cuts(s, ents, e == 1, t5, t3) for e, (_, s, _) in enumerate(recs)]
        if any(t5 + t3 + c5 + c3 + mn > len(s) or t5 + t3 + c5 + c3 + mx < len(s) for (c5, c3), (_, s, _) in zip(cs, recs)):
            continue
        for e, ((c5, c3), (n, s, q)) in enumerate(zip(cs, recs)):
            a, b = t5 + c5, len(s) - t3 - c3
            kept.append((n.split()[0], s[a:b], None if q is None else q[a:b], e))
            counts[2 * e] += c5 > 0
            counts[2 * e + 1] += c3 > 0
    return kept, counts
