"""The numpy statement of the --coverage rule (tests/coverage_ref.py) against a per-base brute-force count, and its text against lines
written by hand - CPU only."""
import numpy as np

import coverage_ref as cr

LENGTHS = {1: 50, 2: 37, 3: 20}
NAMES = {1: "one", 2: "two", 3: "three"}


def brute(reqs, lengths):
    """depth per base, counted base by base; (runs, flagged) by one walk over it"""
    d = {c: [0] * n for c, n in lengths.items()}
    n_flagged = 0
    for q in reqs:
        c, pos, m, m2, gap = (int(q[f]) for f in ("chrom_id", "pos", "m", "m2", "gap"))
        spans = [(pos, pos + m)] + ([(pos + m + gap, pos + m + gap + m2)] if m2 else [])
        if c not in lengths or m == 0 or gap < 0 or any(b > lengths[c] for _, b in spans):
            n_flagged += 1
            continue
        for a, b in spans:
            for p in range(a, b):
                d[c][p] += 1
    runs = []
    for c in sorted(lengths):
        p = 0
        while p < lengths[c]:
            if d[c][p] == 0:
                p += 1
                continue
            z = p
            while z < lengths[c] and d[c][z] == d[c][p]:
                z += 1
            runs.append((c, p, z, d[c][p]))
            p = z
    return d, runs, n_flagged


def random_reqs(rng, n):
    rows = []
    for _ in range(n):
        c = int(rng.integers(0, 5))                           # 0 and 4 do not exist
        ln = LENGTHS.get(c, 30)
        kind = int(rng.integers(0, 10))
        pos, m = int(rng.integers(0, ln)), int(rng.integers(0 if kind == 0 else 1, 12))
        if kind < 5:
            rows.append((c, pos, m))
        else:
            rows.append((c, pos, m, int(rng.integers(0, 8)), int(rng.integers(-1 if kind == 5 else 0, 9))))
    return cr.make_reqs(rows)


def test_reference_against_brute_force():
    rng = np.random.default_rng(11)
    for trial in range(6):
        reqs = random_reqs(rng, 300)
        d, runs, n_flagged = brute(reqs, LENGTHS)
        assert 0 < n_flagged < len(reqs)
        got = cr.depth(reqs, LENGTHS)
        for c in LENGTHS:
            assert got[c].tolist() == d[c]
        r, tot = cr.runs_of(reqs, LENGTHS)
        assert [tuple(int(x) for x in row) for row in r.tolist()] == runs
        assert tot == dict(runs=len(runs), covered=sum(v != 0 for c in d for v in d[c]), depth_sum=sum(sum(v) for v in d.values()),
                           max_depth=max(max(v) for v in d.values()), flagged=n_flagged)
        assert cr.flagged(reqs, LENGTHS).sum() == n_flagged


def test_text_against_hand_written_lines():
    reqs = cr.make_reqs([(1, 0, 10), (1, 5, 10), (1, 15, 5),              # staggered, then abutting the second: [0,5) 1, [5,10) 2, [10,20) 1
                         (1, 49, 1),                                      # the last base of the first sequence ..
                         (2, 0, 3),                                       # .. and the first of the next, the same depth: two runs
                         (2, 10, 4, 4, 6),                                # 4M 6N|D 4M: the gap is not counted
                         (2, 30, 3, 4, 0),                                # 3M xI 4M: one unbroken run
                         (3, 0, 20), (3, 0, 20),                          # a whole sequence, twice
                         (3, 19, 2), (4, 0, 1), (1, 3, 0), (2, 0, 2, 2, -1), (2, 20, 4, 4, 10)])      # flagged: five ways
    runs, tot = cr.runs_of(reqs, LENGTHS)
    assert cr.text_of(runs, NAMES) == (b"one\t0\t5\t1\n" b"one\t5\t10\t2\n" b"one\t10\t20\t1\n" b"one\t49\t50\t1\n"
                                       b"two\t0\t3\t1\n" b"two\t10\t14\t1\n" b"two\t20\t24\t1\n" b"two\t30\t37\t1\n"
                                       b"three\t0\t20\t2\n")
    assert tot == dict(runs=9, covered=5 + 5 + 10 + 1 + 3 + 8 + 7 + 20, depth_sum=10 + 10 + 5 + 1 + 3 + 8 + 7 + 40, max_depth=2, flagged=5)


def test_requests_of_sam_lines():
    recs = [dict(flag=0, rname="one", pos=3, cigar="2S8M"), dict(flag=16, rname="two", pos=1, cigar="5M2S3N4M"), dict(flag=4, rname="*", pos=0, cigar="*"),
            dict(flag=0, rname="two", pos=11, cigar="4M2I6M"), dict(flag=0, rname="three", pos=2, cigar="1S3M1S2D5M")]
    reqs = cr.requests_of_sam(recs, {v: k for k, v in NAMES.items()})
    assert reqs.tolist() == [(1, 2, 8, 0, 0), (2, 0, 5, 4, 3), (2, 10, 4, 6, 0), (3, 1, 3, 5, 2)]
