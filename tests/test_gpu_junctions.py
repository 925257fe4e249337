"""GPU tests of --junctions / --splice-strand (intron motifs read on the device): bk_junctions on crafted requests over a small index of
its own, bk_sam_job.xs on the records of the splice golden file, and the command line on tests/golden/splice.  The reference throughout is
the plain-Python statement of the rule in tests/junction_ref.py against the sequence as indexed: tables, strands and totals must be equal."""
import ctypes
import gzip
import os
import struct

import numpy as np
import pytest

import biokanga_amd as bk
from biokanga_amd.binding import BkError, JUNCTION_DTYPE, JUNCTION_REQ_DTYPE, SAMTAG_MD, SAMTAG_NM
import helpers
import junction_ref as jr
import samtags_ref as sr
from test_gpu_cli import golden_bytes, run
from test_gpu_samtags import bam_records, records_of

pytestmark = pytest.mark.gpu

NAMES, LENS = ("jctA", "jctB", "jctC"), (3000, 2600, 2300)
JCT_WAVE, JCT_BLOCK = 64, 256            # lanes of a wave, threads of a block (kJctBlock) of the kernels of bk_junctions.hip
INTRON = 60
MOTIF_AT = {m: 100 + 40 * m for m in range(1, 7)}          # motif m: donor pair at MOTIF_AT[m], acceptor pair ending INTRON further on
NONCANON_AT, N_DONOR_AT, N_ACCEPTOR_AT = 60, 1500, 1600    # AA..AA; an n as the donor's first base; an n as the acceptor's last base
DONORS, ACCEPTORS = (400, 501), (900, 1001)                # GTGT.. / AGAG.. runs of 34 bases, one from an even and one from an odd position
GTAG_AT, GTAA_AT = 1200, 1210


def plant(text, at, letters):
    text[at:at + len(letters)] = letters


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """three random sequences with the same things planted in each -> (.sfx, samtags_ref.Genome of it)"""
    d = tmp_path_factory.mktemp("junctions")
    rng = np.random.default_rng(20261020)
    seqs = {}
    for nm, n in zip(NAMES, LENS):
        t = list("ACGT"[c] for c in rng.integers(0, 4, n))
        for m, (don, acc) in jr.MOTIFS.items():
            plant(t, MOTIF_AT[m], don)
            plant(t, MOTIF_AT[m] + INTRON - 2, acc)
        plant(t, NONCANON_AT, "AA")
        plant(t, NONCANON_AT + INTRON - 2, "AA")
        plant(t, N_DONOR_AT, "NT")
        plant(t, N_DONOR_AT + INTRON - 2, "AG")
        plant(t, N_ACCEPTOR_AT, "GT")
        plant(t, N_ACCEPTOR_AT + INTRON - 2, "AN")
        for at in DONORS:
            plant(t, at, "GT" * 17)
        for at in ACCEPTORS:
            plant(t, at, "AG" * 17)
        plant(t, GTAG_AT, "GTAG")
        plant(t, GTAA_AT, "GTAA")
        seqs[nm] = "".join(t)
    fa, sfx = str(d / "jct3.fa"), str(d / "jct3.sfx")
    with open(fa, "w") as f:
        for nm, text in seqs.items():
            f.write(f">{nm}\n")
            for k in range(0, len(text), 70):
                f.write(text[k:k + 70] + "\n")
    run(["index", "-i", fa, "-o", sfx, "-r", "jct3"], str(d))
    g = sr.Genome(sfx)
    assert [g.names[i] for i in (1, 2, 3)] == list(NAMES)
    for i in (1, 2, 3):                                   # (nothing mutated: the index holds the file's letters, the two n included)
        assert "".join(sr.LETTERS[c] for c in g.codes[i]) == seqs[NAMES[i - 1]]
    return sfx, g


@pytest.fixture(scope="module")
def al(genome):
    with bk.Aligner(genome[0], bk.AlignParams(max_subs=3)) as a:
        assert a.tune("junction_buf_bytes", 0) == 0       # no call yet: nothing allocated
        yield a


def check(al, g, reqs):
    reqs = np.ascontiguousarray(reqs, dtype=JUNCTION_REQ_DTYPE)
    exp_table, exp_strands, exp_tot = jr.junctions(reqs, g)
    table, strands, tot = al.junctions(reqs)
    print("totals", tot, "expected", exp_tot)
    assert tot == exp_tot
    assert table.dtype == exp_table.dtype and table.tolist() == exp_table.tolist()
    assert np.array_equal(strands, exp_strands)
    return table, strands, tot


def tuned(al, **knobs):
    class T:
        def __enter__(self):
            self.old = {k: al.tune(k, v) for k, v in knobs.items()}

        def __exit__(self, *a):
            for k, v in self.old.items():
                al.tune(k, v)
    return T()


# ---- 1. the library ---------------------------------------------------------------------------------------------------
def test_nothing_held_before_the_first_call_and_empty_call(al, genome):
    table, strands, tot = al.junctions(np.zeros(0, dtype=JUNCTION_REQ_DTYPE))
    assert len(table) == 0 and len(strands) == 0 and tot == dict(requests=0, junctions=0, flagged=0, max_reads=0, by_motif=[0] * 7)
    assert al.tune("junction_buf_bytes", 0) == 0
    table, strands, _ = check(al, genome[1], jr.make_reqs([(2, MOTIF_AT[1], MOTIF_AT[1] + INTRON, 17)]))      # one request
    assert table.tolist() == [(2, MOTIF_AT[1], MOTIF_AT[1] + INTRON, 1, 17, 1, ord("+"))] and bytes(strands) == b"+"
    assert al.tune("junction_buf_bytes", 0) >= 1024 * 16 + 16 + 1 + 20
    assert al.tune("junction_table_slots", 0) == 0


def call(al, reqs, n, strands, out, cap, nj, tot, ctx=True):
    p = lambda a: None if a is None else a.ctypes.data
    return al.lib.bk_junctions(al.h if ctx else None, p(reqs), n, p(strands), p(out), cap, None if nj is None else ctypes.byref(nj), None if tot is None else ctypes.byref(tot))


def test_bad_arguments(al):
    one = jr.make_reqs([(1, MOTIF_AT[2], MOTIF_AT[2] + INTRON, 5)])
    strands, out = np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=JUNCTION_DTYPE)
    nj, tot = ctypes.c_uint64(99), (ctypes.c_uint64 * 11)()
    assert call(al, None, 1, strands, out, 1, nj, tot) == -100
    assert call(al, one, (1 << 32) - 1, strands, out, 1, nj, tot) == -100
    assert call(al, one, 1, strands, out, 1, nj, tot, ctx=False) == -100
    assert call(al, one, 1, strands, None, 1, nj, tot) == -100             # room promised, none given
    assert nj.value == 99
    assert call(al, one, 1, None, out, 1, None, None) == 0 and out.tolist() == [(1, MOTIF_AT[2], MOTIF_AT[2] + INTRON, 1, 5, 2, ord("-"))]
    with pytest.raises(BkError):
        al.tune("junction_table_slots", -1)
    two = jr.make_reqs([(1, 10, 20, 5), (1, 10, 30, 5)])
    for slots in (1000, 3, 1536, 1):
        with tuned(al, junction_table_slots=slots):
            with pytest.raises(BkError) as e:
                al.junctions(two)
            assert e.value.rc == -100


def test_room_too_small_says_what_it_takes_and_writes_nothing_else(al, genome):
    reqs = jr.make_reqs([(1, MOTIF_AT[1], MOTIF_AT[1] + INTRON, 9), (2, MOTIF_AT[2], MOTIF_AT[2] + INTRON, 9), (1, MOTIF_AT[1], MOTIF_AT[1] + INTRON, 12),
                         (3, MOTIF_AT[3], MOTIF_AT[3] + INTRON, 9)])
    exp_table, exp_strands, exp_tot = jr.junctions(reqs, genome[1])
    assert len(exp_table) == 3
    for cap in (0, 2):
        strands, out = np.full(4, 0xEE, dtype=np.uint8), np.frombuffer(b"\xEE" * 60, dtype=JUNCTION_DTYPE).copy()
        nj, tot = ctypes.c_uint64(99), (ctypes.c_uint64 * 11)(*([77] * 11))
        assert call(al, reqs, 4, strands, out, cap, nj, tot) == -95
        assert nj.value == 3 and (strands == 0xEE).all() and out.tobytes() == b"\xEE" * 60 and list(tot) == [77] * 11
    assert call(al, reqs, 4, strands, out, 3, nj, tot) == 0
    assert out.tolist() == exp_table.tolist() and np.array_equal(strands, exp_strands) and list(tot)[:4] == [4, 3, 0, 2]
    # strands and totals alone
    strands[:] = 0xEE
    nj.value = 99
    assert call(al, reqs, 4, strands, None, 0, nj, tot) == 0 and nj.value == 3 and np.array_equal(strands, exp_strands)
    assert list(tot) == [4, 3, 0, 2] + exp_tot["by_motif"]


def test_every_motif_on_every_sequence(al, genome):
    rows = []
    for chrom in (1, 2, 3):
        rows += [(chrom, MOTIF_AT[m], MOTIF_AT[m] + INTRON, 10 + m) for m in range(1, 7)]
        rows += [(chrom, NONCANON_AT, NONCANON_AT + INTRON, 3), (chrom, N_DONOR_AT, N_DONOR_AT + INTRON, 3), (chrom, N_ACCEPTOR_AT, N_ACCEPTOR_AT + INTRON, 3)]
    table, strands, tot = check(al, genome[1], jr.make_reqs(rows))
    assert bytes(strands) == b"+-+-+-\0\0\0" * 3                         # by hand: odd motifs '+', even '-', the three others none
    assert tot["by_motif"] == [9, 3, 3, 3, 3, 3, 3]
    assert sorted(table["motif"][table["chrom_id"] == 3].tolist()) == [0, 0, 0, 1, 2, 3, 4, 5, 6]
    starts = {int(e["entry_id"]): int(e["start_ofs"]) for e in al.entries()}
    assert len(set(starts.values())) == 3 and sorted(starts.values())[1] > 0      # (sequences that do not start at 0 of the target)


def test_every_position_of_a_target_word_at_both_ends(al, genome):
    """start swept over 32 consecutive positions of a GTGT.. run and end over 32 of an AGAG.. run, runs from an even and from an odd
    position: the donor pair and the acceptor pair each lie at every position of a 64-bit word of the 4-bit target - the last one,
    where the pair's second base is the next word's first, included - and are a motif's at every one of them"""
    g = genome[1]
    starts = {int(e["entry_id"]): int(e["start_ofs"]) for e in al.entries()}
    rows, donor_hit, acceptor_hit = [], set(), set()
    for chrom in (1, 2, 3):
        for d0 in DONORS:
            rows += [(chrom, d0 + k, ACCEPTORS[0] + 2, 20) for k in range(32)]
        for a0 in ACCEPTORS:
            rows += [(chrom, DONORS[0], a0 + 2 + k, 20) for k in range(32)]
    reqs = jr.make_reqs(rows)
    table, strands, tot = check(al, g, reqs)
    for q, s in zip(reqs, strands):
        if s == ord("+"):
            donor_hit.add((starts[int(q["chrom_id"])] + int(q["start"])) % 16)
            acceptor_hit.add((starts[int(q["chrom_id"])] + int(q["end"]) - 2) % 16)
    assert donor_hit == set(range(16)) and acceptor_hit == set(range(16))
    assert tot["by_motif"][1] == 3 * (16 * 2 + 16 * 2 - 1) and tot["by_motif"][0] == tot["junctions"] - tot["by_motif"][1]      # ((DONORS[0], ACCEPTORS[0] + 2) is in both sweeps)


def test_short_gaps(al, genome):
    rows = [(2, GTAG_AT, GTAG_AT + k, 8) for k in (1, 2, 3, 4)] + [(2, GTAA_AT, GTAA_AT + 4, 8), (2, DONORS[0], DONORS[0] + 3, 8), (2, ACCEPTORS[0] - 1, ACCEPTORS[0] + 2, 8)]
    table, strands, _ = check(al, genome[1], jr.make_reqs(rows))
    assert bytes(strands) == b"\0\0\0+\0\0\0"                            # gaps of 1, 2, 3: no motif; a gap of 4: its four bases decide
    assert table["motif"].tolist() == [0, 0, 0, 0, 0, 1, 0]


def test_keys_that_share_a_start_or_an_end_or_lie_on_another_sequence_stay_apart(al, genome):
    s, e = MOTIF_AT[1], MOTIF_AT[1] + INTRON
    rows = [(1, s, e, 5)] * 3 + [(1, s, e + 40, 6)] * 2 + [(1, s - 40, e, 7)] + [(2, s, e, 8)] * 4 + [(3, s, e, 9)] * 5 + [(1, s, e, 30)]
    table, _, tot = check(al, genome[1], jr.make_reqs(rows))
    assert [(int(j["chrom_id"]), int(j["start"]), int(j["end"]), int(j["reads"]), int(j["max_overhang"])) for j in table] == \
        [(1, s - 40, e, 1, 7), (1, s, e, 4, 30), (1, s, e + 40, 2, 6), (2, s, e, 4, 8), (3, s, e, 5, 9)]
    assert tot["max_reads"] == 5


def test_five_thousand_requests_on_one_key(al, genome):
    reqs = jr.make_reqs([(3, MOTIF_AT[6], MOTIF_AT[6] + INTRON, 40)] * 5000)
    reqs["overhang"][3777] = 71
    table, strands, tot = check(al, genome[1], reqs)
    assert table.tolist() == [(3, MOTIF_AT[6], MOTIF_AT[6] + INTRON, 5000, 71, 6, ord("-"))] and (strands == ord("-")).all() and tot["max_reads"] == 5000


def test_flagged_requests_among_good_ones_change_nothing(al, genome):
    g = genome[1]
    s, e = MOTIF_AT[2], MOTIF_AT[2] + INTRON
    good = jr.make_reqs([(1 + k % 3, (s, MOTIF_AT[3], 700 + k % 7)[k % 3], (e, MOTIF_AT[3] + INTRON, 990)[k % 3], 1 + k % 50) for k in range(300)])
    bad = jr.make_reqs([(0, s, e, 9), (4, s, e, 9), (0xFFFFFFFF, s, e, 9), (1, 0, e, 9), (1, e, e, 9), (1, e + 1, e, 9), (1, s, LENS[0], 9), (3, s, LENS[2], 9),
                        (3, s, LENS[0], 9), (2, s, 0xFFFFFFFF, 9), (1, s, e, 0), (1, 0xFFFFFFFF, 5, 9)])
    assert all(jr.is_flagged(q, g) for q in bad) and not any(jr.is_flagged(q, g) for q in good)
    mixed = np.concatenate([good[:100], bad[:5], good[100:200], bad[5:], good[200:]])
    table, strands, tot = check(al, g, mixed)
    alone = check(al, g, good)
    assert table.tolist() == alone[0].tolist() and tot["flagged"] == len(bad) and tot["junctions"] == alone[2]["junctions"] > 5
    assert {k: v for k, v in tot.items() if k not in ("requests", "flagged")} == {k: v for k, v in alone[2].items() if k not in ("requests", "flagged")}
    assert not strands[100:105].any() and not strands[205:205 + len(bad) - 5].any()
    _, strands, tot = check(al, g, bad)                                  # nothing but flagged requests: no junction at all
    assert tot["junctions"] == 0 and not strands.any()
    check(al, g, jr.make_reqs([(1, s, LENS[0] - 1, 9), (3, 1, LENS[2] - 1, 9)]))      # the last intron that is none: end = length - 1


def random_requests(n, seed):
    """requests over about 400 junctions: the planted ones on every sequence, and random spans"""
    rng = np.random.default_rng(seed)
    keys = [(c, MOTIF_AT[m], MOTIF_AT[m] + INTRON) for c in (1, 2, 3) for m in range(1, 7)] + [(c, d0 + 2 * k, ACCEPTORS[1] + 2 + 2 * k) for c in (1, 2, 3) for d0 in DONORS for k in range(8)]
    while len(keys) < 400:
        c = int(rng.integers(1, 4))
        s = int(rng.integers(1, LENS[c - 1] - 200))
        keys.append((c, s, s + int(rng.integers(1, 150))))
    pick = rng.integers(0, len(keys), n)
    q = np.zeros(n, dtype=JUNCTION_REQ_DTYPE)
    q["chrom_id"], q["start"], q["end"] = np.array(keys, dtype=np.uint32)[pick].T
    q["overhang"] = rng.integers(1, 101, n)
    return q


@pytest.fixture(scope="module")
def twenty_thousand(genome):
    reqs = random_requests(20000, 5)
    return reqs, jr.junctions(reqs, genome[1])


def test_twenty_thousand_random_requests_and_the_same_shuffled(al, twenty_thousand):
    reqs, (exp_table, exp_strands, exp_tot) = twenty_thousand
    table, strands, tot = al.junctions(reqs)
    print("totals", tot)
    assert tot == exp_tot and table.tolist() == exp_table.tolist() and np.array_equal(strands, exp_strands)
    assert 300 < tot["junctions"] <= 400 and tot["max_reads"] > 50 and tot["flagged"] == 0 and tot["by_motif"][1] > 10 and min(tot["by_motif"][1:]) >= 3
    held = al.tune("junction_buf_bytes", 0)
    perm = np.random.default_rng(9).permutation(20000)
    table2, strands2, tot2 = al.junctions(reqs[perm])
    assert tot2 == exp_tot and table2.tobytes() == table.tobytes() and np.array_equal(strands2, exp_strands[perm])
    assert al.tune("junction_buf_bytes", 0) == held                     # a second call of the same size reuses the buffers


def test_twenty_thousand_random_requests_in_the_smallest_table(al, genome, twenty_thousand):
    """20 000 requests in 32 768 slots of which only the junctions' few hundred are ever taken - and, in a table of exactly as many slots
    as requests, long probe runs that wrap"""
    reqs, (exp_table, exp_strands, exp_tot) = twenty_thousand
    with tuned(al, junction_table_slots=32768):
        table, strands, tot = al.junctions(reqs)
    assert tot == exp_tot and table.tolist() == exp_table.tolist() and np.array_equal(strands, exp_strands)
    distinct = jr.make_reqs([(1 + k % 3, 1 + k // 3, 2000, 1 + k % 9) for k in range(1024)])
    with tuned(al, junction_table_slots=1024):
        table, strands, tot = al.junctions(distinct)                    # every slot taken
        exp = jr.junctions(distinct, genome[1])
        assert tot == exp[2] and tot["junctions"] == 1024 and table.tolist() == exp[0].tolist() and np.array_equal(strands, exp[1])
        with pytest.raises(BkError) as e:
            al.junctions(np.concatenate([distinct, distinct[:1]]))
        assert e.value.rc == -100


@pytest.mark.parametrize("n", [1, JCT_WAVE - 1, JCT_WAVE, JCT_WAVE + 1, JCT_BLOCK, JCT_BLOCK + 1])
def test_wave_and_block_edges(al, genome, n):
    gt = [d0 + 2 * i for d0 in DONORS for i in range(16)]              # where a GT starts, where an AG ends: 32 of each on every sequence
    ag = [a0 + 2 + 2 * i for a0 in ACCEPTORS for i in range(16)]
    reqs = jr.make_reqs([(1 + k % 3, gt[k // 3 % 32], ag[k // 96], 1 + k % 90) for k in range(n)])      # all GT..AG, all distinct
    if n > 1:
        reqs[n - 1] = reqs[0]                          # the last lane's request belongs to the first lane's junction ..
        reqs["overhang"][n - 1] = 99                   # .. and brings its largest overhang
    table, strands, tot = check(al, genome[1], reqs)
    assert (strands == ord("+")).all() and tot["junctions"] == max(n - 1, 1) and tot["by_motif"][1] == tot["junctions"]
    if n > 1:
        assert tot["max_reads"] == 2 and (int(table[0]["reads"]), int(table[0]["max_overhang"])) == (2, 99)


# ---- 2. the formatter: bk_sam_job.xs ------------------------------------------------------------------------------------
def with_xs(text, xs):
    """the body `text` with \\tXS:A:<c> at the end of the lines whose entry of xs is '+' / '-'"""
    lines = [ln for ln in text.split(b"\n") if ln]
    assert len(lines) == len(xs)
    return b"".join(ln + (b"\tXS:A:" + c.encode() if c else b"") + b"\n" for ln, c in zip(lines, xs))


def test_formatter_writes_xs_at_the_end_of_the_lines_it_is_given_for(golden_tmp):
    sfx = os.path.join(golden_tmp["splice"], "genome.sfx")
    g = sr.Genome(sfx)
    golden = b"".join(ln + b"\n" for ln in golden_bytes("splice", "A5000.m6.sam.gz").split(b"\n") if ln and not ln.startswith(b"@"))
    recs = [dict(flag=int(t[1]), rname=t[2], pos=int(t[3]), cigar=t[5]) for t in (ln.split("\t") for ln in golden.decode().split("\n") if ln)]
    exp = jr.expected_xs(recs, g)
    assert sum(1 for c in exp if c == "+") >= 10 and sum(1 for c in exp if c == "-") >= 10
    xs = np.array([ord(c) if c else 0 for c in exp], dtype=np.uint8)
    unaccepted = np.array([bool(r["flag"] & 4) for r in recs])
    assert unaccepted.sum() >= 10
    xs[unaccepted] = ord("+")                              # an unaccepted -M6 line never carries the tag
    plain_acc = np.flatnonzero(~unaccepted & (xs == 0))
    xs[plain_acc[::3]] = 1                                 # neither '+' nor '-': nothing
    xs[plain_acc[1::3]] = ord(".")
    with bk.Aligner(sfx, bk.AlignParams(max_subs=3)) as al:
        ids = {e["name"].decode(): int(e["entry_id"]) for e in al.entries()}
        job, kw = records_of(golden, ids)
        assert al.sam_format(*job, **kw) == golden
        assert al.sam_format(*job, xs=np.zeros(len(recs), dtype=np.uint8), **kw) == golden
        want = with_xs(golden, exp)
        assert want != golden
        for packed in (False, True):
            assert al.sam_format(*job, xs=xs, packed=packed, **kw) == want
            for mask in (SAMTAG_NM | SAMTAG_MD, SAMTAG_NM, SAMTAG_MD):
                tagged = al.sam_format(*job, tags=mask, packed=packed, **kw)
                got = al.sam_format(*job, tags=mask, xs=xs, packed=packed, **kw)
                assert got == with_xs(tagged, exp)
        got = al.sam_format(*job, tags=SAMTAG_NM | SAMTAG_MD, xs=xs, **kw)
        both = [ln.split(b"\t") for ln in got.split(b"\n") if ln.endswith((b"XS:A:+", b"XS:A:-"))]
        assert len(both) == sum(1 for c in exp if c) and all([f[:5] for f in t[11:]] == [b"NM:i:", b"MD:Z:", b"XS:A:"] for t in both)      # order NM, MD, XS
        with pytest.raises(BkError) as e:
            al.sam_format(*job, tags=4, xs=xs, **kw)       # the tag mask has two bits, XS is none of them
        assert e.value.rc == -100


# ---- 3. the command line ---------------------------------------------------------------------------------------------
SETS = [("A5000", ["-A5000", "-s3"]), ("A500s5", ["-A500", "-s5"])]
DEVICE, HOST = {"BK_SAM_DEVICE_MIN": "1"}, {"BK_SAM_DEVICE_MIN": str(1 << 40)}


def cli(golden_tmp, out, flags, fmt="-M6"):
    d = golden_tmp["splice"]
    return ["align", "-i", os.path.join(d, "reads.fa"), "-I", os.path.join(d, "genome.sfx"), "-o", out, fmt] + flags


@pytest.fixture(scope="module")
def splice_genome(golden_tmp):
    return sr.Genome(os.path.join(golden_tmp["splice"], "genome.sfx"))


def reference_of_sam(path, g):
    """the reference's table text, log line and per-line XS over a SAM file"""
    _, recs = helpers.parse_sam(path)
    reqs, _ = jr.requests_of_sam(recs, g.ids)
    table, _, tot = jr.junctions(reqs, g)
    return jr.table_text(table, g), jr.log_line(tot), jr.expected_xs(recs, g), tot, recs


def body_with_xs(golden, exp):
    """the golden file (header included) with the tag on the lines the reference names"""
    out, k = [], 0
    for ln in golden.split(b"\n"):
        if ln and not ln.startswith(b"@"):
            if exp[k]:
                ln += b"\tXS:A:" + exp[k].encode()
            k += 1
        out.append(ln)
    assert k == len(exp)
    return b"\n".join(out)


@pytest.mark.parametrize("tag,flags", SETS, ids=[s[0] for s in SETS])
def test_cli_junction_table(golden_tmp, tmp_path, splice_genome, tag, flags):
    out, sj = str(tmp_path / "o.sam"), str(tmp_path / "sj.tab")
    log = run(cli(golden_tmp, out, flags + ["--junctions", sj]), str(tmp_path))
    assert open(out, "rb").read() == golden_bytes("splice", f"{tag}.m6.sam.gz")
    assert open(out + ".jct", "rb").read() == golden_bytes("splice", f"{tag}.m6.sam.jct.gz")
    text, line, _, tot, _ = reference_of_sam(out, splice_genome)
    assert open(sj).read() == text
    assert line in log, log[-2000:]
    assert tot["junctions"] >= 50 and tot["max_reads"] > 1 and tot["flagged"] == 0
    rows = [ln.split("\t") for ln in text.split("\n") if ln]
    assert all(len(r) == 9 and r[5] == "0" and r[7] == "0" for r in rows) and {r[3] for r in rows} == {"0", "1", "2"}


@pytest.mark.parametrize("formatter", ["device", "host"])
@pytest.mark.parametrize("tag,flags", SETS, ids=[s[0] for s in SETS])
def test_cli_splice_strand(golden_tmp, tmp_path, splice_genome, tag, flags, formatter):
    out = str(tmp_path / "o.sam")
    log = run(cli(golden_tmp, out, flags + ["--splice-strand"]), str(tmp_path), env=dict(DEVICE if formatter == "device" else HOST, BK_TIMING="1"))
    assert ("SAM formatted on the device" in log) == (formatter == "device"), log[-1500:]
    golden = golden_bytes("splice", f"{tag}.m6.sam.gz")
    gold_path = str(tmp_path / "golden.sam")
    open(gold_path, "wb").write(golden)
    _, line, exp, tot, recs = reference_of_sam(gold_path, splice_genome)
    assert open(out, "rb").read() == body_with_xs(golden, exp)
    assert line in log
    assert not os.path.exists(str(tmp_path / "sj.tab"))
    spliced = [k for k, r in enumerate(recs) if "N" in r["cigar"] and not r["flag"] & 4]
    assert min(sum(1 for k in spliced if exp[k] == "+"), sum(1 for k in spliced if exp[k] == "-"), sum(1 for k in spliced if exp[k] is None)) >= 10
    assert {bool(recs[k]["flag"] & 16) for k in spliced if exp[k]} == {False, True}       # tagged records on both read strands


@pytest.mark.parametrize("formatter", ["device", "host"])
@pytest.mark.parametrize("tag,flags", SETS, ids=[s[0] for s in SETS])
def test_cli_splice_strand_with_sam_tags(golden_tmp, tmp_path, splice_genome, tag, flags, formatter):
    env = DEVICE if formatter == "device" else HOST
    tagged, both = str(tmp_path / "t.sam"), str(tmp_path / "b.sam")
    run(cli(golden_tmp, tagged, flags + ["--sam-tags", "NM,MD"]), str(tmp_path), env=env)
    run(cli(golden_tmp, both, flags + ["--sam-tags", "NM,MD", "--splice-strand"]), str(tmp_path), env=env)
    bare, _ = sr.strip_body(open(tagged, "rb").read())
    assert bare == golden_bytes("splice", f"{tag}.m6.sam.gz")
    _, _, exp, _, _ = reference_of_sam(tagged, splice_genome)
    assert open(both, "rb").read() == body_with_xs(open(tagged, "rb").read(), exp)
    assert sum(1 for c in exp if c) >= 50


def bam_aux_xs(rec):
    """the aux fields of a BAM record (as bam_records returns it) -> {tag: value} for the types the writer uses"""
    l_qn, n_cig, l_seq = rec[8], struct.unpack_from("<H", rec, 12)[0], struct.unpack_from("<I", rec, 16)[0]
    at = 32 + l_qn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    out = {}
    while at < len(rec):
        t, typ = rec[at:at + 2].decode(), chr(rec[at + 2])
        at += 3
        if typ == "A":
            out[t], at = chr(rec[at]), at + 1
        else:
            assert typ == "Z", typ
            end = rec.index(b"\0", at)
            out[t], at = rec[at:end].decode(), end + 1
    return out


@pytest.mark.parametrize("tag,flags", SETS, ids=[s[0] for s in SETS])
def test_cli_gzip_and_bam_carry_the_same_strands_and_every_form_the_same_table(golden_tmp, tmp_path, splice_genome, tag, flags):
    golden = golden_bytes("splice", f"{tag}.m6.sam.gz")
    gold_path = str(tmp_path / "golden.sam")
    open(gold_path, "wb").write(golden)
    text, _, exp, _, recs = reference_of_sam(gold_path, splice_genome)
    gz, bam, bam0 = (str(tmp_path / n) for n in ("x.sam.gz", "x.bam", "x0.bam"))
    run(cli(golden_tmp, gz, flags + ["--splice-strand", "--junctions", gz + ".tab"]), str(tmp_path))
    assert gzip.open(gz, "rb").read() == body_with_xs(golden, exp)
    run(cli(golden_tmp, bam, flags + ["--splice-strand", "--junctions", bam + ".tab"]), str(tmp_path))
    run(cli(golden_tmp, bam0, flags), str(tmp_path))
    head, brecs = bam_records(bam)
    head0, brecs0 = bam_records(bam0)
    assert head == head0 and len(brecs) == len(brecs0) == len(recs)
    for r, r0, c, line in zip(brecs, brecs0, exp, recs):
        assert r0[32:32 + r0[8]] == line["qname"].encode() + b"\0"     # (the BAM's records are in the SAM file's order)
        assert r[:len(r0)] == r0 and r[len(r0):] == (b"XSA" + c.encode() if c else b"")
        assert bam_aux_xs(r).get("XS") == c
    # the table: whatever the output format, and with two contexts on one device
    forms = [(str(tmp_path / "m0.csv"), "-M0", []), (str(tmp_path / "m5.sam"), "-M5", []), (str(tmp_path / "d.sam"), "-M6", ["--devices", "0,0"])]
    for out, fmt, extra in forms:
        run(cli(golden_tmp, out, flags + extra + ["--junctions", out + ".tab"], fmt=fmt), str(tmp_path))
    for out in [gz, bam] + [f[0] for f in forms]:
        assert open(out + ".tab").read() == text, out
    assert open(forms[2][0], "rb").read() == golden


@pytest.mark.parametrize("tag,flags", SETS, ids=[s[0] for s in SETS])
def test_cli_without_the_options_nothing_changes(golden_tmp, tmp_path, tag, flags):
    out = str(tmp_path / "o.sam")
    log = run(cli(golden_tmp, out, flags), str(tmp_path), env={"BK_TIMING": "1"})
    assert open(out, "rb").read() == golden_bytes("splice", f"{tag}.m6.sam.gz")
    assert sorted(os.listdir(str(tmp_path))) == ["o.sam", "o.sam.jct"]
    assert "Junctions" not in log and "junctions:" not in log


def test_cli_best_matches_find_no_junctions(golden_tmp, tmp_path):
    """-N sends the reads through the best-matches search, which has no splice branch: -A is accepted, the table is empty, no line is tagged"""
    out, sj = str(tmp_path / "o.sam"), str(tmp_path / "sj.tab")
    log = run(cli(golden_tmp, out, ["-A5000", "-s3", "-r2", "-R5", "-N", "--junctions", sj, "--splice-strand"]), str(tmp_path))
    assert open(sj, "rb").read() == b""
    assert b"XS:A:" not in open(out, "rb").read() and b"N" not in b"".join(ln.split(b"\t")[5] for ln in open(out, "rb").read().split(b"\n") if ln and not ln.startswith(b"@"))
    assert "Junctions: 0 spliced records, 0 junctions (0 GT/AG, 0 other canonical, 0 non-canonical), most reads at one junction 0" in log
