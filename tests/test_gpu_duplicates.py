"""GPU tests of --mark-duplicates (FLAG 0x400 set by a device grouping pass): bk_mark_duplicates on crafted requests over a small index
of its own, and the command line on reads cut from that index's sequences.  The reference throughout is the plain-Python statement of
the rule in tests/dup_ref.py: answers and totals must be equal, and the FLAGs of the written lines those the rule gives for them."""
import gzip
import os
import struct

import numpy as np
import pytest

import biokanga_amd as bk
from biokanga_amd.binding import BkError, DUP_REQ_DTYPE
import dup_ref as dr
import helpers
from test_gpu_cli import run

pytestmark = pytest.mark.gpu

NAMES, LENS = ("dupA", "dupB", "dupC"), (3000, 2600, 2300)
CHROMS = {1, 2, 3}
DUP_WAVE, DUP_BLOCK = 64, 256            # lanes of a wave, threads of a block (kDupBlock) of the kernels of bk_dups.hip


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """three random sequences and their index -> (directory, .sfx, {name: text})"""
    d = tmp_path_factory.mktemp("dups")
    rng = np.random.default_rng(20261020)
    seqs = {nm: "".join("ACGT"[c] for c in rng.integers(0, 4, n)) for nm, n in zip(NAMES, LENS)}
    fa, sfx = str(d / "dup3.fa"), str(d / "dup3.sfx")
    with open(fa, "w") as f:
        for nm, text in seqs.items():
            f.write(f">{nm}\n")
            for k in range(0, len(text), 70):
                f.write(text[k:k + 70] + "\n")
    run(["index", "-i", fa, "-o", sfx, "-r", "dup3"], str(d))
    return str(d), sfx, seqs


@pytest.fixture(scope="module")
def al(genome):
    with bk.Aligner(genome[1], bk.AlignParams(max_subs=3)) as a:
        assert a.tune("dup_buf_bytes", 0) == 0            # no call yet: nothing allocated
        yield a


def check(al, reqs, want=None):
    reqs = np.ascontiguousarray(reqs, dtype=DUP_REQ_DTYPE)
    exp, exp_tot = dr.mark(reqs, CHROMS)
    if want is not None:
        assert exp.tolist() == want
    out, tot = al.mark_duplicates(reqs)
    print("totals", tot, "expected", exp_tot)
    assert tot == exp_tot
    assert np.array_equal(out, exp)
    return out, tot


def tuned(al, **knobs):
    class T:
        def __enter__(self):
            self.old = {k: al.tune(k, v) for k, v in knobs.items()}

        def __exit__(self, *a):
            for k, v in self.old.items():
                al.tune(k, v)
    return T()


# ---- 1. the library ---------------------------------------------------------------------------------------------------
def test_nothing_held_before_the_first_call_and_empty_call(al):
    out, tot = al.mark_duplicates(np.zeros(0, dtype=DUP_REQ_DTYPE))
    assert len(out) == 0 and tot == dict(templates=0, groups=0, duplicates=0, max_group=0, flagged=0)
    assert al.tune("dup_buf_bytes", 0) == 0
    check(al, dr.make_reqs([(2, 17, "+", 100)]), want=[0])                                   # one request
    assert al.tune("dup_buf_bytes", 0) >= 1024 * 16 + 17
    assert al.tune("dup_table_slots", 0) == 0


def test_bad_arguments(al):
    import ctypes
    one = dr.make_reqs([(1, 0, "+", 5)])
    out = np.zeros(1, dtype=np.uint8)
    tot = (ctypes.c_uint64 * 5)()
    assert al.lib.bk_mark_duplicates(al.h, None, 1, out.ctypes.data, ctypes.byref(tot)) == -100
    assert al.lib.bk_mark_duplicates(al.h, one.ctypes.data, 1, None, ctypes.byref(tot)) == -100
    assert al.lib.bk_mark_duplicates(al.h, one.ctypes.data, (1 << 32) - 1, out.ctypes.data, ctypes.byref(tot)) == -100
    assert al.lib.bk_mark_duplicates(None, one.ctypes.data, 1, out.ctypes.data, ctypes.byref(tot)) == -100
    assert al.lib.bk_mark_duplicates(al.h, one.ctypes.data, 1, out.ctypes.data, None) == 0 and out[0] == 0
    with pytest.raises(BkError):
        al.tune("dup_table_slots", -1)


def test_two_equal_keys_both_score_orders_and_a_tie(al):
    check(al, dr.make_reqs([(1, 500, "+", 90), (1, 500, "+", 100)]), want=[1, 0])
    check(al, dr.make_reqs([(1, 500, "+", 100), (1, 500, "+", 90)]), want=[0, 1])
    check(al, dr.make_reqs([(1, 500, "+", 100), (1, 500, "+", 100)]), want=[0, 1])
    check(al, dr.make_reqs([(1, 500, "+", 100), (1, 500, "-", 100), (2, 500, "+", 100), (1, -500, "+", 100), (1, -500, "+", 100)]), want=[0, 0, 0, 0, 1])


def test_pairs_mirrored_pairs_and_fragments_at_their_ends(al):
    check(al, dr.make_reqs([(1, 100, "+", 200, 400, "-"), (1, 400, "-", 200, 100, "+"), (1, 400, "+", 200, 100, "-"), (1, 100, "+", 100), (1, 400, "-", 100),
                            (1, 100, "+", 200, 0, "+"), (1, 100, "+", 201, 400, "-"), (1, 7, "-", 1, 7, "+"), (1, 7, "+", 1, 7, "-"), (1, 100, "+", 100, 12345, 0)]),
          want=[1, 1, 0, 0, 0, 0, 0, 0, 1, 1])


def test_five_thousand_requests_on_one_key(al):
    reqs = dr.make_reqs([(3, 1234, "-", 77)] * 5000)
    out, tot = check(al, reqs)
    assert out[0] == 0 and (out[1:] == 1).all() and tot["max_group"] == 5000 and tot["groups"] == 1
    reqs["score"][3777] = 78                   # one better one in the crowd
    out, tot = check(al, reqs)
    assert (out == 0).sum() == 1 and out[3777] == 0


def random_templates(n, seed):
    """fragments and pairs mixed over 3 sequences x 200 positions x 2 strands, scores from 90..100"""
    rng = np.random.default_rng(seed)
    q = np.zeros(n, dtype=DUP_REQ_DTYPE)
    q["chrom_id"] = rng.integers(1, 4, n)
    q["pos5"] = rng.integers(0, 200, n) - 20
    q["strand"] = rng.choice([dr.PLUS, dr.MINUS], n)
    q["score"] = rng.integers(90, 101, n)
    pair = rng.random(n) < 0.4
    q["pos5_mate"] = np.where(pair, q["pos5"] + rng.integers(0, 4, n) * 50, rng.integers(-5, 5, n))       # (a fragment's is not looked at)
    q["strand_mate"] = np.where(pair, rng.choice([dr.PLUS, dr.MINUS], n), 0)
    return q


@pytest.fixture(scope="module")
def twenty_thousand():
    reqs = random_templates(20000, 5)
    return reqs, dr.mark(reqs, CHROMS)


def test_twenty_thousand_random_templates(al, twenty_thousand):
    reqs, (exp, exp_tot) = twenty_thousand
    out, tot = al.mark_duplicates(reqs)
    print("totals", tot)
    assert tot == exp_tot and np.array_equal(out, exp)
    assert tot["groups"] > 1000 and tot["duplicates"] > 1000 and tot["max_group"] > 5 and tot["flagged"] == 0
    # the same requests twice give the same answer (the table is cleared per call), and so does a table of the smallest size allowed
    out2, tot2 = al.mark_duplicates(reqs)
    assert tot2 == exp_tot and np.array_equal(out2, exp)
    with tuned(al, dup_table_slots=32768):
        out3, tot3 = al.mark_duplicates(reqs)
    assert tot3 == exp_tot and np.array_equal(out3, exp)


def test_twenty_thousand_random_templates_shuffled(al, twenty_thousand):
    """the tie-break is by request index: the reference is applied to the same order"""
    reqs = twenty_thousand[0][np.random.default_rng(9).permutation(20000)]
    _, tot = check(al, reqs)
    assert tot["groups"] == twenty_thousand[1][1]["groups"] and tot["max_group"] == twenty_thousand[1][1]["max_group"]


def distinct_keys(n):
    return dr.make_reqs([(1 + k % 3, k // 3, "+-"[(k // 7) % 2], 100) for k in range(n)])


def test_full_table_and_table_sizes_that_are_refused(al):
    reqs = distinct_keys(1025)
    assert len({dr.key_of(q) for q in reqs}) == 1025
    with tuned(al, dup_table_slots=1024):
        out, tot = check(al, reqs[:1024])              # every slot taken: probes wrap past the mask
        assert tot["groups"] == 1024 and not out.any()
        check(al, np.concatenate([reqs[:512], reqs[:512]]))
        with pytest.raises(BkError) as e:
            al.mark_duplicates(reqs)
        assert e.value.rc == -100
    for slots in (1000, 3, 1536):
        with tuned(al, dup_table_slots=slots):
            with pytest.raises(BkError) as e:
                al.mark_duplicates(reqs[:2])
            assert e.value.rc == -100
    with tuned(al, dup_table_slots=2):
        check(al, reqs[:2])
        check(al, reqs[[0, 0]])
    check(al, reqs)                                    # derived again


@pytest.mark.parametrize("n", [DUP_WAVE - 1, DUP_WAVE, DUP_WAVE + 1, DUP_BLOCK - 1, DUP_BLOCK, DUP_BLOCK + 1])
def test_wave_and_block_edges(al, n):
    reqs = distinct_keys(n)
    reqs[n - 1] = reqs[0]                              # the last lane's request belongs to the first lane's group ..
    reqs["score"][n - 1] = 101                         # .. and is its keeper
    out, tot = check(al, reqs)
    assert out[0] == 1 and out[n - 1] == 0 and tot["groups"] == n - 1 and tot["max_group"] == 2


def test_flagged_requests_in_the_middle_of_a_group_do_not_disturb_it(al):
    good = dr.make_reqs([(2, 40, "-", 90 + k % 5) for k in range(300)])
    bad = dr.make_reqs([(0, 40, "-", 100), (4, 40, "-", 100), (0xFFFFFFFF, 40, "-", 100), (2, 40, "?", 100), (2, 40, 0, 100), (2, 40, "-", 100, 40, "x"),
                        (2, 40, "-", 100, 40, 1)])
    assert (dr.mark(bad, CHROMS)[0] == dr.FLAGGED).all()
    mixed = np.concatenate([good[:100], bad[:3], good[100:200], bad[3:], good[200:]])
    out, tot = check(al, mixed)
    assert tot == dict(templates=307, groups=1, duplicates=299, max_group=300, flagged=7)
    assert (out == 0).sum() == 1 and out[4] == 0       # the first request that scores 94
    check(al, bad)                                     # nothing but flagged requests: no group at all


# ---- 2. the command line ---------------------------------------------------------------------------------------------
COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def mutate(s, at):
    return s[:at] + "ACGT"[("ACGT".index(s[at]) + 1) % 4] + s[at + 1:]


def write_reads(path, reads):
    with open(path, "w") as f:
        for name, text in reads:
            f.write(f">{name}\n{text}\n")
    return {name: k for k, (name, _) in enumerate(reads)}


@pytest.fixture(scope="module")
def se_reads(genome):
    """reads of 100 bases cut from the sequences; of some: exact copies under other names, copies on the other strand, copies whose
    second or last-but-one base differs - which -x5 trims to 2S98M / 98M2S, the unclipped 5' end unmoved and two M bases fewer"""
    d, sfx, seqs = genome
    rng = np.random.default_rng(11)
    starts = {nm: rng.choice(len(seqs[nm]) - 100, size=20, replace=False) for nm in NAMES}           # no two reads share a start
    reads = []
    for k in range(60):
        nm = NAMES[k % 3]
        at = int(starts[nm][k // 3])
        a = seqs[nm][at:at + 100]
        kind = k % 6
        if kind == 0:
            reads += [(f"r{k}", a)]
        elif kind == 1:
            reads += [(f"r{k}", a), (f"r{k}copy", a), (f"r{k}again", a)]
        elif kind == 2:
            reads += [(f"r{k}", a), (f"r{k}rc", revcomp(a)), (f"r{k}rc2", revcomp(a))]
        elif kind == 3:
            reads += [(f"r{k}trim", mutate(a, 1)), (f"r{k}", a), (f"r{k}trim3", mutate(a, 98))]           # the trimmed copy is loaded first and still loses
        elif kind == 4:
            reads += [(f"r{k}rctrim", mutate(revcomp(a), 1)), (f"r{k}rc", revcomp(a)), (f"r{k}", a)]
        else:
            reads += [(f"r{k}trim", mutate(a, 1)), (f"r{k}trimtoo", mutate(a, 1))]                        # equal scores: the first stays
    path = os.path.join(d, "se_reads.fa")
    return path, write_reads(path, reads)


def flags_by_name(path):
    _, recs = helpers.parse_sam(path)
    return recs, {r["qname"]: r["flag"] for r in recs}


def strip_dup_bit(raw):
    out = []
    for ln in raw.split(b"\n"):
        if ln and not ln.startswith(b"@"):
            t = ln.split(b"\t")
            t[1] = str(int(t[1]) & ~0x400).encode()
            ln = b"\t".join(t)
        out.append(ln)
    return b"\n".join(out)


def marked(flags):
    return {n for n, f in flags.items() if f & 0x400}


@pytest.mark.parametrize("formatter", ["host", "device"])
def test_cli_single_ends(genome, se_reads, tmp_path, formatter):
    d, sfx, _ = genome
    path, load = se_reads
    env = {"BK_SAM_DEVICE_MIN": "1"} if formatter == "device" else None
    base = ["align", "-i", path, "-I", sfx, "-M5", "-s3", "-x5"]
    plain, dups = str(tmp_path / "plain.sam"), str(tmp_path / "dups.sam")
    run(base + ["-o", plain], str(tmp_path), env=env)
    log = run(base + ["-o", dups, "--mark-duplicates"], str(tmp_path), env=env)
    recs, flags = flags_by_name(dups)
    assert len(recs) == len(load)                                   # every read was accepted
    exp = dr.expected_flags(recs, load)
    assert [r["flag"] for r in recs] == exp
    assert strip_dup_bit(open(dups, "rb").read()) == open(plain, "rb").read()
    assert not marked(flags_by_name(plain)[1])
    m = marked(flags)
    print(sorted(m))
    # by hand: of every group the untrimmed read loaded first stays
    assert {"r1copy", "r1again", "r2rc2", "r3trim", "r3trim3", "r4rctrim", "r5trimtoo"} <= m
    assert not {"r0", "r1", "r2", "r2rc", "r3", "r4rc", "r4", "r5trim"} & m
    assert len(m) == 10 * (2 + 1 + 2 + 1 + 1)
    assert sum(1 for r in recs if "S" in r["cigar"]) == 10 * (2 + 1 + 2)
    reqs, _ = dr.requests_of_sam(recs, load)
    tot = dr.mark(reqs)[1]
    assert f"Duplicates: {tot['templates']} templates ({tot['templates']} fragments, 0 pairs) in {tot['groups']} groups, {tot['duplicates']} templates ({len(m)} records) marked as duplicates, largest group {tot['max_group']}" in log


def bam_flags(path):
    raw = gzip.decompress(open(path, "rb").read())
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, at)
    at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, at)
        at += 4 + l_name + 4
    flags = {}
    while at < len(raw):
        block, = struct.unpack_from("<i", raw, at)
        l_qn = raw[at + 12]
        flag_nc, = struct.unpack_from("<I", raw, at + 16)
        flags[raw[at + 36:at + 36 + l_qn - 1].decode()] = flag_nc >> 16
        at += 4 + block
    return flags


def test_cli_every_output_form_marks_the_same_reads(genome, se_reads, tmp_path):
    d, sfx, _ = genome
    path, load = se_reads
    base = ["align", "-i", path, "-I", sfx, "-s3", "-x5", "--mark-duplicates"]
    got = {}
    for tag, out, extra, env in (("sam", "o.sam", ["-M5"], None), ("gz", "o.sam.gz", ["-M5"], None), ("bam", "o.bam", ["-M5"], None), ("m6", "o6.sam", ["-M6"], None),
                                 ("tags", "ot.sam", ["-M5", "--sam-tags", "NM,MD"], {"BK_SAM_DEVICE_MIN": "1"}), ("tagsgz", "ot.sam.gz", ["-M6", "--sam-tags", "NM,MD"], None)):
        run(base + extra + ["-o", str(tmp_path / out)], str(tmp_path), env=env)
        got[tag] = bam_flags(str(tmp_path / out)) if tag == "bam" else flags_by_name(str(tmp_path / out))[1]
    assert len(marked(got["sam"])) == 70
    for tag in got:
        assert got[tag] == got["sam"], tag
    recs, _ = flags_by_name(str(tmp_path / "ot.sam"))
    assert all(len(r["tags"]) == 2 for r in recs)                   # duplicates keep their tags


@pytest.fixture(scope="module")
def pe_reads(genome):
    """pairs cut from fragments of 300 bases (PE1 the first 100 bases, PE2 the last 100 reverse complemented): exact copies, a mirrored
    pair (PE1 and PE2 swapped), orphans - a mate of random bases - alone and at a pair's end, and a read that aligns nowhere at all"""
    d, sfx, seqs = genome
    rng = np.random.default_rng(12)
    starts = {nm: rng.choice(len(seqs[nm]) - 300, size=8, replace=False) for nm in NAMES}            # no two fragments share a start
    r1, r2 = [], []

    def add(name, a, b):
        r1.append((name + "/1", a))
        r2.append((name + "/2", b))
    junk = lambda: "".join("ACGT"[c] for c in rng.integers(0, 4, 100))
    for k in range(24):
        nm = NAMES[k % 3]
        at = int(starts[nm][k // 3])
        frag = seqs[nm][at:at + 300]
        a, b = frag[:100], revcomp(frag[-100:])
        kind = k % 4
        add(f"p{k}", a, b)
        if kind == 1:
            add(f"p{k}copy", a, b)
            add(f"p{k}again", a, mutate(b, 50))
        elif kind == 2:
            add(f"p{k}mirror", b, a)
        elif kind == 3:
            add(f"p{k}orphan", a, junk())
            add(f"p{k}orphantoo", a, junk())
    add("nowhere", junk(), junk())
    p1, p2 = os.path.join(d, "pe_1.fa"), os.path.join(d, "pe_2.fa")
    write_reads(p1, r1)
    write_reads(p2, r2)
    load = {}
    for k, ((n1, _), (n2, _)) in enumerate(zip(r1, r2)):
        load[n1], load[n2] = 2 * k, 2 * k + 1
    return p1, p2, load


@pytest.mark.parametrize("formatter", ["host", "device"])
def test_cli_paired_ends(genome, pe_reads, tmp_path, formatter):
    d, sfx, _ = genome
    p1, p2, load = pe_reads
    env = {"BK_SAM_DEVICE_MIN": "1"} if formatter == "device" else None
    base = ["align", "-i", p1, "-u", p2, "-I", sfx, "-M6", "-s3", "-U3", "-d200", "-D400"]
    plain, dups = str(tmp_path / "plain.sam"), str(tmp_path / "dups.sam")
    run(base + ["-o", plain], str(tmp_path), env=env)
    log = run(base + ["-o", dups, "--mark-duplicates"], str(tmp_path), env=env)
    recs, flags = flags_by_name(dups)
    assert len(recs) == len(load)                                   # -M6: a line per read
    assert [r["flag"] for r in recs] == dr.expected_flags(recs, load)
    assert strip_dup_bit(open(dups, "rb").read()) == open(plain, "rb").read()
    m = marked(flags)
    print(sorted(m))
    reqs, members = dr.requests_of_sam(recs, load)
    n_pairs = int((reqs["strand_mate"] != 0).sum())
    assert n_pairs >= 24 + 6 and len(reqs) - n_pairs >= 12         # the pairs and their exact copies at least; the orphans' aligned ends
    # both mates of an exact copy, and of the copy with one mismatch (M bases count, mismatches do not: the first loaded stays)
    assert {"p1copy/1", "p1copy/2", "p1again/1", "p1again/2", "p3orphantoo/1"} <= m
    assert not {"p0/1", "p0/2", "p1/1", "p1/2", "p3/1", "p3/2", "p3orphan/1", "nowhere/1", "nowhere/2"} & m
    assert all(not (r["flag"] & 0x400) for r in recs if r["flag"] & 4)         # lines of unaccepted reads never carry the bit
    by_name = {r["qname"]: r for r in recs}
    assert not by_name["p2mirror/1"]["flag"] & 0x8                   # written as a pair: F2R1 at p2's ends is p2's molecule
    assert {"p2mirror/1", "p2mirror/2"} <= m
    tot = dr.mark(reqs)[1]
    assert f"Duplicates: {tot['templates']} templates ({tot['templates'] - n_pairs} fragments, {n_pairs} pairs) in {tot['groups']} groups, {tot['duplicates']} templates ({len(m)} records) marked as duplicates, largest group {tot['max_group']}" in log
