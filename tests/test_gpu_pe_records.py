"""The paired-end pass of bk_rescue.hip (k_pe_classify, pe_finish, pe_adj_loci, pe_insert_size, k_pe_orphan, launch_pe) on BUILT hit
records: the pair-rule table as a product of its inputs, and the geometry of the orphan recovery around sequence ends, the expected
records always taken from the oracle (helpers.oracle_process_pe) on a copy of the same input and compared exactly, field by field.  The
records keep to what the aligner can emit: existing sequence ids, placements inside their sequence, trims below the read length,
unaligned records without a locus.  Plus the reference's own runs on the edge fixture (tests/golden/peedge) through align + pair, and
k_count_seqs beyond its LDS histogram."""
import itertools

import numpy as np
import pytest

import helpers
from test_oracle_pe import check_pe_hits_against_sam, filt_by_chroms
from test_oracle_pe_edges import CHROMS, RUNS as EDGE_RUNS, check_nar_summary, files, oracle_run, reads, run_reads, se_hits  # noqa: F401

pytestmark = pytest.mark.gpu

L = 100
SEQ_LENS = (4000, 4000, 2500)
HIT_FIELDS = ("chrom_id", "match_loci", "match_len", "low_hit_instances", "rslt", "nar", "strand", "low_mm", "nxt_low_mm", "num_hits", "mismatches")
SEG2_FIELDS = ("match_loci", "match_len", "read_ofs", "mismatches", "flags", "score")
PLUS, MINUS = ord("+"), ord("-")


def _bk():
    import biokanga_amd
    return biokanga_amd


class Index:
    """a numpy index on the device and in the oracle: sequences of the given lengths, each followed by a separator"""

    def __init__(self, lens, seed, seqs=None):
        """seqs: the sequences themselves; otherwise random ones of the given lengths"""
        import torch
        bk = _bk()
        rng = np.random.default_rng(seed)
        self.seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in lens] if seqs is None else list(seqs)
        lens = [len(q) for q in self.seqs]
        self.lens = tuple(lens)
        self.concat = np.concatenate([np.concatenate([s, [7]]) for s in self.seqs]).astype(np.uint8)
        n = len(self.concat)
        self.entries, ofs = [], 0
        for i, ln in enumerate(lens):
            self.entries.append((i + 1, ln, ofs, ofs + ln - 1))
            ofs += ln + 1
        dev = torch.device("cuda:0")
        self.d_seq = torch.from_numpy(self.concat).to(dev)
        self.d_sa = torch.empty(n, dtype=torch.int32, device=dev)
        bk.build_sa_device(self.d_seq.data_ptr(), n, self.d_sa.data_ptr(), 4, 0)
        self.sa = self.d_sa.cpu().numpy().view(np.uint32)
        self.ora = helpers.OracleSfx(seq=self.concat, sa=self.sa, el_size=4, entries=self.entries)
        self.ent = np.zeros(len(lens), dtype=bk.ENTRY_DTYPE)
        for i, (eid, slen, so, eo) in enumerate(self.entries):
            self.ent[i] = (eid, slen, so, eo, f"s{eid}".encode(), b"")

    def aligner(self, **kw):
        bk = _bk()
        return bk.Aligner(None, bk.AlignParams(**kw), d_seq=self.d_seq.data_ptr(), concat_len=len(self.concat), d_sa=self.d_sa.data_ptr(), el_size=4,
                          entries=self.ent)


@pytest.fixture(scope="module")
def index():
    ix = Index(SEQ_LENS, 20261020)
    yield ix
    ix.ora.close()


def assert_same(got, exp, what, gseg=None, eseg=None):
    """every field of the hit records, FlgPEAligned and - where given - every field of seg2, the first differing pair printed"""
    bad = np.zeros(len(exp), dtype=bool)
    for f in HIT_FIELDS:
        bad |= got[f] != exp[f]
    bad |= (got["flags"] & 0x80) != (exp["flags"] & 0x80)
    if eseg is not None:
        for f in SEG2_FIELDS:
            bad |= gseg[f] != eseg[f]
    if bad.any():
        i = int(np.nonzero(bad)[0][0]) // 2
        msg = f"{what}: {int(bad.sum())} records differ, first in pair {i}:\n got {got[2 * i]} {got[2 * i + 1]}\n exp {exp[2 * i]} {exp[2 * i + 1]}"
        if eseg is not None:
            msg += f"\n got seg2 {gseg[2 * i]} {gseg[2 * i + 1]}\n exp seg2 {eseg[2 * i]} {eseg[2 * i + 1]}"
        raise AssertionError(msg)


def both(ix, al, subs, mode, d, D, E, bases, offs, lens, recs, seg2=None, accept=None, min_chim=0):
    """-> (device records, oracle records[, device seg2, oracle seg2]) of one call on copies of recs"""
    bk = _bk()
    p = helpers.make_params(max_subs=subs, min_chimeric_len=min_chim)
    exp = recs.copy()
    eseg = None if seg2 is None else seg2.copy()
    helpers.oracle_process_pe(ix.ora, p, mode, d, D, E, bases, offs, lens, exp, eseg, accept=accept)
    al.set_chrom_filter(accept)
    if seg2 is None:
        got = al.pair(bases, offs, lens, recs.copy(), bk.PEParams(mode, d, D, E))
        return got, exp
    got, gseg = al.pair(bases, offs, lens, recs.copy(), bk.PEParams(mode, d, D, E), seg2=seg2.copy())
    return got, exp, gseg, eseg


def accepted(rec, chrom, loci, strand, mm=0):
    rec["chrom_id"], rec["match_loci"], rec["match_len"], rec["strand"] = chrom, loci, L, strand
    rec["nar"], rec["num_hits"], rec["low_hit_instances"], rec["rslt"] = 1, 1, 1, 1
    rec["low_mm"], rec["nxt_low_mm"], rec["mismatches"] = mm, -1, mm


def n_try_orphan(recs, mode):
    """a lower bound of the pairs k_pe_classify hands to k_pe_orphan: one end accepted and unique, the other MH or ML, i.e. neither accepted
    nor unaligned in the sense of its rule - such a pair is never paired or stopped before the try_orphan test and passes it"""
    if mode not in (1, 3):
        return 0
    f, r = recs[0::2], recs[1::2]

    def mh_ml(h):
        return (h["nar"] == 4) | (h["nar"] == 5)
    one = ((f["nar"] == 1) & mh_ml(r)) | ((r["nar"] == 1) & mh_ml(f))
    return int(one.sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the pair-rule table
TD, TDD = 200, 230
END_STATES = [(nar, nh) for nar in range(6) for nh in (1, 2) if not (nar == 1 and nh == 2)]
SEQ_PAIRS = ((1, 1), (1, 2), (2, 1), (3, 3))
STRANDS = ((PLUS, PLUS), (PLUS, MINUS), (MINUS, PLUS), (MINUS, MINUS))
INSERTS = (-50, TD - 1, TD, (TD + TDD) // 2, TDD, TDD + 1, 1100)


def build_table(seed=7):
    """-> (bases, offs, lens, recs) of the product, pairs in a seeded random order so that every prefix is a mixture"""
    bk = _bk()
    rows = []                                              # (state1, state2, seqs, strands, start1, start2)
    for s1, s2 in itertools.product(END_STATES, END_STATES):
        one_sided = (s1[0] == 1) != (s2[0] == 1) and (s2 if s1[0] == 1 else s1)[0] in (4, 5)
        for sq, st, ins, first_up in itertools.product(SEQ_PAIRS, STRANDS, INSERTS, (True, False)):
            # one end accepted, the other MH / ML: these reach the recovery - six base loci each, for more than 8192 of them in a call
            for x in ((1200, 1213, 1226, 1239, 1252, 1265) if one_sided else (1200,)):
                lo, up = x, x + ins - L
                rows.append((s1, s2, sq, st, lo if first_up else up, up if first_up else lo))
    # accepted pairs: every insert in range on both strands of the fragment, in the orientation each -E setting pairs
    for ch in (1, 2, 3):
        for ins in range(TD, TDD + 1):
            for st, first_up in (((PLUS, MINUS), True), ((MINUS, PLUS), False), ((PLUS, PLUS), True), ((MINUS, MINUS), False)):
                lo, up = 700 + ins, 700 + ins + ins - L
                rows.append(((1, 1), (1, 1), (ch, ch), st, lo if first_up else up, up if first_up else lo))
    order = np.random.default_rng(seed).permutation(len(rows))
    recs = np.zeros(2 * len(rows), dtype=bk.HIT_DTYPE)
    for k, j in enumerate(order):
        s1, s2, sq, st, p1, p2 = rows[j]
        for e, (state, ch, strand, p) in enumerate(((s1, sq[0], st[0], p1), (s2, sq[1], st[1], p2))):
            rec = recs[2 * k + e:2 * k + e + 1]
            if state[0] == 1:
                accepted(rec, ch, p, strand)
            else:                                          # unaligned: no locus
                rec["nar"], rec["num_hits"], rec["low_hit_instances"] = state[0], state[1], state[1]
    n = len(recs)
    bases = np.random.default_rng(seed + 1).integers(0, 4, n * L).astype(np.uint8)
    lens = np.full(n, L, dtype=np.uint32)
    offs = (np.arange(n, dtype=np.uint64) * L).astype(np.uint64)
    return bases, offs, lens, recs


@pytest.fixture(scope="module")
def table():
    t = build_table()
    t[3].setflags(write=False)
    return t


def filter_tables():
    return {"none": None, "first out": np.array([1, 0, 1, 1], np.uint8), "second out": np.array([1, 1, 0, 1], np.uint8),
            "only first": np.array([1, 1, 0, 0], np.uint8), "short": np.array([1, 0], np.uint8)}      # short: ids 2 and 3 lie beyond it and pass


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_pair_rule_table(index, table, mode):
    bases, offs, lens, recs = table
    assert n_try_orphan(recs, 3) > 8192
    seen = np.zeros(20, dtype=np.int64)
    n_pe = 0
    with index.aligner(max_subs=5) as al:
        for E in (False, True):
            for name, accept in filter_tables().items():
                got, exp = both(index, al, 5, mode, TD, TDD, E, bases, offs, lens, recs, accept=accept)
                seen += np.bincount(exp["nar"], minlength=20)
                n_pe += int(((exp["flags"] & 0x80) != 0).sum())
                if name == "none" and not E:
                    assert int(((exp["flags"][0::2] & 0x80) != 0).sum()) >= 100          # accepted pairs in the plain run
                    # random reads: nothing is recovered, the result is the table alone
                    both_in = np.repeat((recs["nar"][0::2] == 1) & (recs["nar"][1::2] == 1), 2)
                    assert not np.any(((exp["flags"] & 0x80) != 0) & ~both_in)
                assert_same(got, exp, f"-U{mode} E={E} filter {name}")
    print(f"-U{mode}: oracle NAR counts over 10 runs {dict((helpers.NAR_TAGS[k], int(v)) for k, v in enumerate(seen) if v)}, PE-aligned records {n_pe}")
    assert n_pe >= 10
    # (-U3 / -U4 accept what aligned uniquely as single-ended at the end, which overwrites the pair reasons 13, 14, 16 and 17)
    need = {1: (11, 13, 14, 15, 16, 17), 2: (11, 13, 14, 15, 16, 17), 3: (11, 18), 4: (11, 18)}[mode]
    for nar in need:
        assert seen[nar] >= 10, (mode, helpers.NAR_TAGS[nar], int(seen[nar]))


def test_pair_rule_table_every_reason_occurs(index, table):
    """NAR 11, 13 .. 18 and FlgPEAligned each in at least 10 records of the oracle's output over the runs (15 NP needs -U1 / -U2, 18 UP -U3 / -U4)"""
    bases, offs, lens, recs = table
    seen = np.zeros(20, dtype=np.int64)
    p = helpers.make_params(max_subs=5)
    for mode, accept in ((1, None), (1, filter_tables()["first out"]), (3, filter_tables()["first out"])):
        exp = recs.copy()
        helpers.oracle_process_pe(index.ora, p, mode, TD, TDD, False, bases, offs, lens, exp, accept=accept)
        seen += np.bincount(exp["nar"], minlength=20)
        assert ((exp["flags"] & 0x80) != 0).sum() >= 10
    for nar in (11, 13, 14, 15, 16, 17, 18):
        assert seen[nar] >= 10, (helpers.NAR_TAGS[nar], int(seen[nar]))


@pytest.mark.parametrize("n_pairs", [1, 255, 256, 257])
def test_pair_rule_table_block_edges(index, table, n_pairs):
    bases, offs, lens, recs = table
    n = 2 * n_pairs
    with index.aligner(max_subs=5) as al:
        for mode in (1, 2, 3, 4):
            got, exp = both(index, al, 5, mode, TD, TDD, False, bases, offs[:n], lens[:n], recs[:n].copy())
            assert_same(got, exp, f"{n_pairs} pairs -U{mode}")


def test_pair_rule_table_on_device_buffers(index, table):
    import torch
    bk = _bk()
    bases, offs, lens, recs = table
    pe = bk.PEParams(3, TD, TDD, False)
    dev = torch.device("cuda", 0)
    with index.aligner(max_subs=5) as al:
        exp = al.pair(bases, offs, lens, recs.copy(), pe)
        d_b = torch.from_numpy(np.ascontiguousarray(bases)).to(dev)
        d_o = torch.from_numpy(offs.astype(np.int64)).to(dev)
        d_l = torch.from_numpy(lens.astype(np.int32)).to(dev)
        d_h = torch.from_numpy(recs.copy().view(np.uint8)).to(dev)
        al.pair_device(d_b.data_ptr(), d_o.data_ptr(), d_l.data_ptr(), len(lens) // 2, d_h.data_ptr(), pe)
        got = d_h.cpu().numpy().view(bk.HIT_DTYPE)
    assert got.tobytes() == exp.tobytes()


def test_pair_rules_on_trimmed_loci(index, table):
    """pe_adj_loci: on a -c context the pair rules look at the end-trimmed loci of chimeric placements (seg2 flags bit 3).  The table
    once more with seg2, and pairs whose trims carry the insert across -d or -D, on both strands"""
    bk = _bk()
    bases, offs, lens, recs = table
    rng = np.random.default_rng(11)
    rows = []
    for ch in (1, 2, 3):
        for ins in list(range(TD, TD + 10)) + list(range(TDD + 1, TDD + 11)):
            for st, first_up in (((PLUS, MINUS), True), ((MINUS, PLUS), False), ((PLUS, PLUS), True), ((MINUS, MINUS), False)):
                for rep in range(4):
                    lo = 600 + 3 * ins + rep
                    rows.append((ch, st, lo if first_up else lo + ins - L, lo + ins - L if first_up else lo))
    xr = np.zeros(2 * len(rows), dtype=bk.HIT_DTYPE)
    xs = np.zeros(len(xr), dtype=bk.SEG2_DTYPE)
    for k, (ch, st, p1, p2) in enumerate(rows):
        accepted(xr[2 * k:2 * k + 1], ch, p1, st[0])
        accepted(xr[2 * k + 1:2 * k + 2], ch, p2, st[1])
    chim = rng.random(len(xr)) < 0.6
    xs["flags"][chim] = 8
    xs["match_len"][chim] = rng.integers(0, 7, int(chim.sum()))            # TrimLeft
    xs["read_ofs"][chim] = rng.integers(0, 7, int(chim.sum()))             # TrimRight
    # trims on records that are not chimeric placements must be ignored
    xs["match_len"][~chim] = rng.integers(0, 7, int((~chim).sum()))
    allr = np.concatenate([recs, xr])
    seg = np.concatenate([np.zeros(len(recs), dtype=bk.SEG2_DTYPE), xs])
    tseg = rng.random(len(recs)) < 0.3
    tseg &= recs["nar"] == 1
    seg["flags"][:len(recs)][tseg] = 8
    seg["match_len"][:len(recs)][tseg] = rng.integers(0, 40, int(tseg.sum()))
    seg["read_ofs"][:len(recs)][tseg] = rng.integers(0, 40, int(tseg.sum()))
    n = len(allr)
    ab = np.concatenate([bases, np.random.default_rng(12).integers(0, 4, len(xr) * L).astype(np.uint8)])
    al_lens = np.full(n, L, dtype=np.uint32)
    al_offs = (np.arange(n, dtype=np.uint64) * L).astype(np.uint64)
    p = helpers.make_params(max_subs=5, min_chimeric_len=50)
    with index.aligner(max_subs=5, min_chimeric_len=50) as al:
        for mode, E in ((3, False), (3, True), (1, False), (2, True), (4, False)):
            got, exp, gseg, eseg = both(index, al, 5, mode, TD, TDD, E, ab, al_offs, al_lens, allr, seg2=seg, min_chim=50)
            plain = allr.copy()
            helpers.oracle_process_pe(index.ora, p, mode, TD, TDD, E, ab, al_offs, al_lens, plain, np.zeros(n, dtype=bk.SEG2_DTYPE))
            x0 = len(recs)
            for s0 in (PLUS, MINUS):                       # the trims changed the verdict, in both directions, with either strand first
                first = exp["strand"][x0::2] == s0
                was, now = (plain["flags"][x0::2] & 0x80) != 0, (exp["flags"][x0::2] & 0x80) != 0
                if mode == 3:
                    assert int((first & was & ~now).sum()) >= 20 and int((first & ~was & now).sum()) >= 20, (mode, E, chr(s0))
            assert_same(got, exp, f"-c -U{mode} E={E}", gseg, eseg)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the geometry of the orphan recovery
def geometry(anchor_first, strand, E):
    """(b3prime, antisense) of AlignPairedRead's call for this anchor (Aligner.cpp:3224-3260,3323-3358)"""
    b3 = strand == PLUS
    if anchor_first:
        return b3, ((strand != PLUS) if E else (strand == PLUS))
    anti = strand == PLUS
    return (not b3, not anti) if E else (b3, anti)


def build_geometry(ix, d, D, E, seed, cap=None):
    bk = _bk()
    rng = np.random.default_rng(seed)
    rows = []
    for ci, n in enumerate(ix.lens):
        loci = set(range(0, 61)) | set(range(n - L - 60, n - L + 1))
        for c in (D, D + L, n - D - L, n - d - L, D - L, d - L):
            loci |= set(range(c - 30, c + 31))
        for a in sorted(x for x in loci if 0 <= x <= n - L):
            for strand in (PLUS, MINUS):
                for first in (True, False):
                    rows.append((ci, a, strand, first))
    if cap is not None and len(rows) > cap:
        rows = [rows[i] for i in sorted(rng.choice(len(rows), cap, replace=False))]
    recs = np.zeros(2 * len(rows), dtype=bk.HIT_DTYPE)
    reads = rng.integers(0, 4, (2 * len(rows), L)).astype(np.uint8)
    stats = dict(give1=0, give2=0, give3=0, clamp=0, past_seq=0, past_concat=0)
    concat_len = len(ix.concat)
    for k, (ci, a, strand, first) in enumerate(rows):
        n = ix.lens[ci]
        ai, oi = (2 * k, 2 * k + 1) if first else (2 * k + 1, 2 * k)
        accepted(recs[ai:ai + 1], ci + 1, a, strand)
        recs["nar"][oi], recs["num_hits"][oi], recs["low_hit_instances"][oi] = 5, 2, 2
        b3, anti = geometry(first, strand, E)
        a_end = a + L - 1
        ins = (d, (d + D) // 2, D)[k % 3]
        p = a + ins - L if b3 else a_end - ins + 1
        if 0 <= p <= n - L:
            r = ix.seqs[ci][p:p + L].copy()
            for q in rng.choice(L, k % 4, replace=False):
                r[q] = (r[q] + 1 + rng.integers(0, 3)) & 3
            reads[oi] = (3 - r)[::-1] if anti else r
        # the branch this anchor takes, by the arithmetic of AlignPairedRead (SfxArrayV2.cpp:8296-8345)
        if b3:
            if a + d > n:
                stats["give1"] += 1
            elif a + d + L >= n:
                stats["give2"] += 1
            elif ix.entries[ci][2] + a + D + L > concat_len:
                stats["past_concat"] += 1
            elif a + D + L > n and ci < len(ix.lens) - 1:
                stats["past_seq"] += 1
        else:
            if a_end < d:
                stats["give3"] += 1
            elif a_end < D:
                stats["clamp"] += 1
    n2 = len(recs)
    return reads.reshape(-1), (np.arange(n2, dtype=np.uint64) * L).astype(np.uint64), np.full(n2, L, dtype=np.uint32), recs, stats


@pytest.mark.parametrize("mode", [3, 1])
@pytest.mark.parametrize("E", [False, True])
@pytest.mark.parametrize("d,D", [(200, 400), (150, 1149), (150, 1150)])
def test_orphan_geometry(index, d, D, E, mode):
    bases, offs, lens, recs, st = build_geometry(index, d, D, E, 1000 + D + int(E), cap=3000 if D - d == 999 else None)
    print(f"d={d} D={D} E={E} -U{mode}: {len(recs) // 2} pairs, {st}")
    for k in ("give1", "give2", "give3"):
        assert st[k] >= 50, (k, st)
    assert st["clamp"] >= 20 and st["past_seq"] >= 20 and st["past_concat"] >= 20, st
    with index.aligner(max_subs=5) as al:
        got, exp = both(index, al, 5, mode, d, D, E, bases, offs, lens, recs)
    rec = int(((exp["nar"] == 1) & (recs["nar"] == 5)).sum())
    print(f"   recovered by the oracle: {rec}")
    assert rec >= 500
    assert_same(got, exp, f"geometry d={d} D={D} E={E} -U{mode}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's runs on the edge fixture, through align + pair
@pytest.mark.parametrize("tag", sorted(EDGE_RUNS))
def test_pe_edges_match_reference_and_oracle(files, reads, se_hits, tag):  # noqa: F811
    bk = _bk()
    cfg = EDGE_RUNS[tag]
    names, bases, offs, lens = run_reads(reads, cfg)
    accept = None
    if "Z" in cfg or "z" in cfg:
        accept = helpers.chrom_accept_table(CHROMS, exclude=cfg.get("Z", ()), include=cfg.get("z", ()))
    with bk.Aligner(files["genome.sfx"], bk.AlignParams(max_subs=5)) as al:
        se = al.align(bases, offs, lens)
        for f in HIT_FIELDS:
            assert np.array_equal(se[f], se_hits[bool(cfg.get("safe"))][f]), f
        al.set_chrom_filter(accept)
        hits = al.pair(bases, offs, lens, se.copy(), bk.PEParams(cfg["pe"], cfg.get("d", 200), cfg.get("D", 400), cfg.get("E", False)))
    exp, _ = oracle_run(files["genome.sfx"], reads, se_hits, cfg)
    assert_same(hits, exp, tag)
    final = hits.copy()
    if accept is not None:
        filt_by_chroms(final, CHROMS, cfg.get("Z", ()), cfg.get("z", ()))
    check_pe_hits_against_sam(names, final, tag, CHROMS, "peedge")
    check_nar_summary(final, tag)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_seq_counts_beyond_the_lds_histogram():
    """k_count_seqs counts entries 0..4095 in LDS and the rest with global atomics: 4300 sequences, reads on all of them, the last included"""
    n_seq, sl, rl = 4300, 120, 50
    ix = Index([sl] * n_seq, 4300)
    rng = np.random.default_rng(4301)
    which = np.concatenate([np.arange(n_seq), np.arange(n_seq - 40, n_seq), rng.integers(0, n_seq, 2000)])
    reads = []
    for i, s in enumerate(which):
        p = int(rng.integers(0, sl - rl + 1))
        r = ix.seqs[s][p:p + rl].copy()
        if i % 3 == 0:
            r[int(rng.integers(0, rl))] ^= 1
        reads.append((3 - r)[::-1] if i % 2 else r)
    bases = np.concatenate(reads).astype(np.uint8)
    lens = np.full(len(reads), rl, dtype=np.uint32)
    offs = (np.arange(len(reads), dtype=np.uint64) * rl).astype(np.uint64)
    exp, _ = ix.ora.align(bases, offs, lens, helpers.make_params(max_subs=3), nthreads=8)
    ix.ora.close()
    with ix.aligner(max_subs=3) as al:
        got = al.align(bases, offs, lens)
        counts = al.seq_counts()
    for f in HIT_FIELDS:
        assert np.array_equal(got[f], exp[f]), f
    want = np.bincount(exp["chrom_id"][exp["nar"] == 1], minlength=n_seq + 1)[1:]
    assert want[4096:].sum() > 200 and want[-1] > 0 and want[:4096].sum() > 4000
    assert np.array_equal(counts.astype(np.int64), want.astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) several acceptable windows in one scan: the reference raises MinPutLen after every placement it takes, the kernel scans once with the
# initial limit and keeps the smallest key (bk_dev_trim.h, above pe_window_key).  -c contexts: the 8-word mismatch map for reads of 100
# bases, the 32-word one (long_reads) for reads of 600
WS = 5                                                     # -s of these contexts
# copies of the partner per layout: (percent of the read replaced at its start, at its end, substitutions), planted a read length and more
# apart, i.e. in different 64-lane groups of the offset scan
LAYOUTS = {"longest first": [(0, 0, 1), (10, 10, 0), (20, 20, 0)], "longest middle": [(10, 10, 0), (0, 0, 1), (20, 20, 0)],
           "longest last": [(20, 20, 0), (10, 10, 0), (0, 0, 1)], "more mismatches first": [(10, 10, 2), (10, 10, 0)],
           "fewer mismatches first": [(10, 10, 0), (10, 10, 2)], "equal": [(10, 10, 1), (10, 10, 1)], "uneven ends": [(25, 0, 1), (0, 25, 1), (12, 13, 0)],
           "whole, equal": [(0, 0, 1), (0, 0, 1)], "whole, more first": [(0, 0, 2), (0, 0, 0), (0, 0, 1)], "whole, fewer first": [(0, 0, 0), (0, 0, 2)],
           "four": [(20, 20, 0), (0, 0, 2), (0, 0, 1), (10, 10, 0)], "trimmed, uneven": [(5, 15, 0), (15, 5, 1)]}
# reads of 600 bases: -D admits a second window at most 399 loci behind the first, so the two copies keep different parts of the read - the
# first its leading c1 bases, the second its trailing c2: (c1, c2, substitutions in either, loci between the windows)
LONG_LAYOUTS = {"longer first": (340, 310, 0, 0, 150), "longer last": (310, 340, 0, 0, 150), "equal": (320, 320, 0, 0, 150),
                "more mismatches first": (320, 320, 2, 0, 150), "fewer mismatches first": (320, 320, 0, 2, 150), "equal, one each": (320, 320, 1, 1, 150),
                "longer first, -c70 too": (440, 430, 0, 0, 300), "longer last, -c70 too": (430, 440, 1, 0, 300), "equal, -c70 too": (430, 430, 1, 1, 300),
                "one group, longer last": (300, 330, 0, 0, 40), "one group, equal": (310, 310, 0, 0, 33), "one group, fewer first": (310, 310, 0, 1, 50),
                "first longer, fewer": (450, 420, 0, 1, 300), "last longer, more": (420, 450, 0, 2, 300), "one group, more first": (330, 300, 2, 0, 30),
                "one group, longer first": (325, 315, 0, 0, 50), "whole last": (330, 600, 0, 2, 350), "whole first": (600, 330, 1, 0, 350),
                # a whole-length stretch with more than -s mismatches behind an acceptable shorter one: it passes AdaptiveTrim's rate only on a
                # long read, is taken for its length, and the pair is then dropped (mm > max_allowed after the scan)
                "displaced": (340, 600, 0, 12, 350)}
# windows fewer than 64 loci apart, inside one group of the scan (asserted from start_put): the partner is periodic, so the windows 30 loci
# apart match alike; a substitution in the first 30 bases of the run lies in the first window only, one behind the read length in the second
PERIODIC = {"tie": (), "first worse": (10,), "second worse": (-20,), "both, tie": (10, -20)}
# .. and (reads of 100 bases) two 60-base cores side by side, the windows around them 60 loci apart; a substitution in either core
CORES = {"tie": (), "first worse": (1,), "second worse": (2,)}


def trim_of(read_fwd, targ, min_put):
    """AdaptiveTrim as AlignPairedRead calls it -> (trimmed length or 0, mismatches)"""
    import ctypes
    mm, t5, t3 = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    a, b = np.ascontiguousarray(read_fwd), np.ascontiguousarray(targ)
    r = helpers.oracle_lib().ora_adaptive_trim(len(a), a.ctypes.data, b.ctypes.data, min_put, WS, 3, ctypes.byref(mm), ctypes.byref(t5), ctypes.byref(t3))
    return max(int(r), 0), int(mm.value)


def build_windows(seed, rl, d):
    """-> (sequence, bases, offs, lens, recs, cases): one region per pair, the anchor unique on '+' as read 1, the partner ML and altered
    copies of it planted in its window.  cases: (kind, name, partner in target direction, loci of the planted windows)"""
    bk = _bk()
    rng = np.random.default_rng(seed)
    far = {n: c for n, c in LAYOUTS.items() if n != "displaced"}
    kinds = ([("far", n) for n in far] if rl <= 512 else [("long", n) for n in LONG_LAYOUTS]) + [("periodic", n) for n in PERIODIC] + \
            ([("cores", n) for n in CORES] if rl == 100 else [])
    region = d + 1000 + 2 * rl + 300
    assert region * len(kinds) + 1500 < 100000
    seq = rng.integers(0, 4, region * len(kinds) + 1500).astype(np.uint8)
    recs = np.zeros(2 * len(kinds), dtype=bk.HIT_DTYPE)
    reads = np.zeros((2 * len(kinds), rl), dtype=np.uint8)
    cases = []
    for k, (kind, name) in enumerate(kinds):
        a = k * region + 50
        sp = a + d                                         # start_put
        if kind == "far":
            part = rng.integers(0, 4, rl).astype(np.uint8)
            los = []
            for j, (k5, k3, subs) in enumerate(far[name]):
                lo = sp + 7 + j * (rl + 19 + 64 * (k % 2))
                assert lo - sp < 990
                c = part.copy()
                k5, k3 = k5 * rl // 100, k3 * rl // 100
                c[:k5] = 3 - c[:k5]                        # foreign ends: every base differs
                c[rl - k3:] = 3 - c[rl - k3:]
                for q in range(subs):
                    at = rl * (40 + 12 * q) // 100 if subs <= 3 else 60 + 40 * q
                    c[at] = (c[at] + 1 + (j + q) % 3) & 3
                seq[lo:lo + rl] = c
                los.append(lo)
        elif kind == "long":
            c1, c2, s1, s2, gap = LONG_LAYOUTS[name]
            part = rng.integers(0, 4, rl).astype(np.uint8)
            lo1, lo2 = sp + 7, sp + 7 + gap
            assert gap >= c1 + c2 - rl and lo2 + rl - 1 - a + 1 <= d + 999        # the kept stretches apart, the second within -D
            seq[lo1:lo2 + rl] = 3                                                  # then every base outside the kept stretches differs
            seq[lo1:lo1 + rl] = 3 - part
            seq[lo2 + (lo1 + rl - lo2):lo2 + rl] = (3 - part)[lo1 + rl - lo2:]
            one, two = part[:c1].copy(), part[rl - c2:].copy()
            for q in range(s1):
                one[40 + 25 * q] = (one[40 + 25 * q] + 1) & 3
            for q in range(s2):
                two[50 + 35 * q] = (two[50 + 35 * q] + 2) & 3
            seq[lo1:lo1 + c1] = one
            seq[lo2 + rl - c2:lo2 + rl] = two
            los = [lo1, lo2]
        elif kind == "periodic":
            run = np.tile(rng.integers(0, 4, 30).astype(np.uint8), rl // 30 + 3)[:rl + 30]
            part = run[:rl].copy()
            lo = sp + 64 + 1                               # windows at 1 and 31 of the second group (and the shorter ones 30 beside them)
            for q in PERIODIC[name]:
                at = q if q >= 0 else rl + 30 + q - 10     # 10: first window only; rl: second window only
                run[at] = (run[at] + 1) & 3
            seq[lo - 1] = 3 - part[29]                     # the run does not go on to either side
            seq[lo + rl + 30] = 3 - part[(rl + 30) % 30]
            seq[lo:lo + rl + 30] = run
            los = [lo, lo + 30]
        else:
            while True:
                part = rng.integers(0, 4, rl).astype(np.uint8)
                if part[20] != part[80] and part[19] != part[79]:
                    break
            lo = sp + 128 + 2                              # windows at 2 and 62 of the third group
            both_cores = np.concatenate([part[20:80], part[20:80]])
            for q in CORES[name]:
                at = 30 + 60 * (q - 1)
                both_cores[at] = (both_cores[at] + 1) & 3
            seq[lo + 20:lo + 140] = both_cores
            seq[lo + 19], seq[lo + 140] = 3 - part[19], 3 - part[80]      # neither core goes on beyond its 60 bases
            los = [lo, lo + 60]
        reads[2 * k] = seq[a:a + rl]
        reads[2 * k + 1] = (3 - part)[::-1]                # the partner as sequenced: on '-'
        accepted(recs[2 * k:2 * k + 1], 1, a, PLUS)
        recs["match_len"][2 * k] = rl
        recs["nar"][2 * k + 1], recs["num_hits"][2 * k + 1], recs["low_hit_instances"][2 * k + 1] = 5, 2, 2
        cases.append((kind, name, part, los))
    n2 = len(recs)
    return seq, reads.reshape(-1), (np.arange(n2, dtype=np.uint64) * rl).astype(np.uint64), np.full(n2, rl, dtype=np.uint32), recs, cases


@pytest.mark.parametrize("span", [999, 1000])
@pytest.mark.parametrize("rl", [100, 600])
def test_scan_with_several_acceptable_windows(rl, span):
    bk = _bk()
    d = 150 if rl == 100 else 700
    D = d + span
    seq, bases, offs, lens, recs, cases = build_windows(77 + rl, rl, d)
    ix = Index(None, 0, seqs=[seq])
    # what was planted, by AdaptiveTrim with the initial limit of the -c50 contexts on every planted window
    n_same_group = n_tie = 0
    for k, (kind, name, part, los) in enumerate(cases):
        sp = int(recs["match_loci"][2 * k]) + d
        tr = [trim_of(part, seq[lo:lo + rl], rl // 2) for lo in los]
        if kind in ("periodic", "cores") or name.startswith("one group"):
            assert (los[0] - sp) // 64 == (los[1] - sp) // 64 and tr[0][0] > 0 and tr[1][0] > 0, (kind, name, los, sp, tr)
            n_same_group += 1
            if name.endswith("tie"):
                assert tr[0] == tr[1], (kind, name, tr)
                n_tie += 1
        elif name == "displaced":
            assert 0 < tr[0][0] < tr[1][0] and tr[0][1] <= WS < tr[1][1], tr
    assert n_same_group >= 4 and n_tie >= 2
    n_rec = n_chim = n_later = n_displaced = 0
    for min_chim in (0, 50, 70):
        with ix.aligner(max_subs=WS, min_chimeric_len=min_chim) as al:
            if min_chim:
                seg = np.zeros(len(recs), dtype=bk.SEG2_DTYPE)
                got, exp, gseg, eseg = both(ix, al, WS, 3, d, D, False, bases, offs, lens, recs, seg2=seg, min_chim=min_chim)
                n_chim += int(((eseg["flags"][1::2] & 8) != 0).sum())
            else:
                got, exp = both(ix, al, WS, 3, d, D, False, bases, offs, lens, recs)
                gseg = eseg = None
        for k, (kind, name, part, los) in enumerate(cases):
            h = exp[2 * k + 1]
            if h["nar"] == 1:
                n_rec += 1
                n_later += int(h["match_loci"]) != los[0]
                if name.endswith("tie") and kind in ("periodic", "cores"):  # equal in length and mismatches inside one group: the first in scan order
                    assert int(h["match_loci"]) == los[0] or span == 1000, (kind, name, min_chim, h, los)
            elif name == "displaced" and min_chim == 50:
                n_displaced += 1
        assert_same(got, exp, f"windows of {rl}-base reads, D-d={span} -c{min_chim}", gseg, eseg)
    ix.ora.close()
    print(f"reads of {rl}, D-d={span}: {len(cases)} pairs x 3 contexts, recovered {n_rec}, end-trimmed {n_chim}, not at the first planted window {n_later}, "
          f"displaced {n_displaced}")
    assert n_rec >= 30 and n_chim >= 10 and n_later >= 5
    assert n_displaced == (1 if rl > 512 else 0)
