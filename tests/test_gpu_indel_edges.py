"""k_indel (bk_rescue.hip: LocateInDels / LocateSpliceJuncts and their Explore* routines) against the oracle at its edges: every run of
tests/golden/indeledge - on which tests/test_oracle_indel_edges.py pins the oracle to the reference - with 4-byte and with 5-byte suffix
elements (k_indel<false> / k_indel<true>), in one chunk, in chunks of 64 reads and without the wave kernel; and a seeded sweep of planted
insertions, deletions and introns at uniformly random read offsets and loci, sequence ends included."""
import json
import os

import numpy as np
import pytest

import helpers
from test_gpu_parity import _assert_loci_equal, _bk, assert_hits_equal, assert_seg2_equal

pytestmark = pytest.mark.gpu

with open(os.path.join(helpers.GOLDEN, "indeledge", "cases.json")) as _f:
    TAGS = sorted(json.load(_f)["cases"])


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("indeledge"))
    cases, sfx, reads = helpers.indel_edge_fixture(d)
    wide = {g: helpers.rewrite_sfx_5byte(p, os.path.join(d, g + "5.sfx"), g) for g, p in sfx.items()}
    return cases, {4: sfx, 5: wide}, reads, {}


def oracle_expected(fixture, tag):
    """the oracle's records of a run, made once (on the 4-byte index: the element size does not reach the oracle's answer)"""
    cases, sfx, reads, cache = fixture
    if tag not in cache:
        cs = cases["cases"][tag]
        kw, lo, hi = helpers.indel_edge_params(cs["flags"])
        names, bases, offs, lens = reads[cs["reads"]]
        keep = helpers.filter_reads_by_len(names, bases, offs, lens, lo, hi)
        o = helpers.OracleSfx(sfx[4][cs["genome"]])
        if kw.get("max_ml", 0) > 1:
            exp = helpers.oracle_align_multi_indel(o, bases, offs[keep], lens[keep], helpers.make_params(**kw))
        else:
            exp = helpers.oracle_align_indel(o, bases, offs[keep], lens[keep], helpers.make_params(**kw))
        o.close()
        cache[tag] = (kw, [names[i] for i in keep], bases, offs[keep], lens[keep], exp)
    return cache[tag]


@pytest.mark.parametrize("el_size", [4, 5])
@pytest.mark.parametrize("tag", TAGS)
def test_indel_edge_runs_match_oracle(fixture, tag, el_size):
    """every hit field and every bk_seg2 field, the loci lists of the -r run; of the -c run the effect of k_indel's `flags == 0x80` state
    records on the result records (the chimeric call takes and clears them, so none is left in bk_seg2 to compare)"""
    bk = _bk()
    cases, sfx, _, _ = fixture
    kw, names, bases, offs, lens, exp = oracle_expected(fixture, tag)
    path = sfx[el_size][cases["cases"][tag]["genome"]]
    for knobs in ([], [("chunk_reads", 64)], [("use_wave", 0)]):
        with bk.Aligner(path, bk.AlignParams(**kw)) as al:
            assert al.lib.bk_sfx_el_size(al.h) == el_size
            for k, v in knobs:
                al.tune(k, v)
            got = al.align(bases, offs, lens)
            seg = al.batch_seg2()
            if kw.get("max_ml", 0) > 1:
                _assert_loci_equal(bk, al, len(lens), got, exp[0], exp[1], exp[2])
        assert_hits_equal(got, exp[0], names)
        assert_seg2_equal(seg, exp[-1], names)
    if kw.get("min_chimeric_len"):
        # an ambiguous junction search leaves its counts behind (k_indel's `flags == 0x80` state record, which the chimeric call takes and
        # clears): two placements without a mismatch, and with that nothing more is searched - the tie|two_seqs junction reads
        e = exp[0]
        left = (e["rslt"] == 3) & (e["low_hit_instances"] == 2) & (e["low_mm"] == 0) & (e["nxt_low_mm"] == 2)
        assert np.count_nonzero(left) >= 4 and not np.any(exp[-1]["flags"] == 0x80)


# ------------------------------------------------------------------------------------------------
def suffix_array(seq):
    """plain suffix order of the byte string (a shorter suffix before the longer one it starts), by prefix doubling"""
    n = len(seq)
    rank = seq.astype(np.int64)
    k = 1
    while True:
        r2 = np.full(n, -1, dtype=np.int64)
        r2[:n - k] = rank[k:]
        order = np.lexsort((r2, rank))
        step = (rank[order][1:] != rank[order][:-1]) | (r2[order][1:] != r2[order][:-1])
        rank = np.zeros(n, dtype=np.int64)
        rank[order[1:]] = np.cumsum(step)
        if rank.max() == n - 1:
            return order.astype(np.uint32)
        k *= 2


SWEEP_SEED, SWEEP_READS, SWEEP_KW = 7348, 2000, dict(max_subs=3, micro_indel_len=20, splice_junct_len=3000)


def sweep_case(seed=SWEEP_SEED, n_genome=50000, n_reads=SWEEP_READS):
    """two sequences with a planted repeat family (as _synth_case of test_gpu_parity.py has them); reads of 30..600 bases with an insertion or
    a deletion of 1..20 bases or an intron of 25..2900 at a uniformly random read offset, the placement uniformly random within a sequence
    (its first and last locus included), 0..3 substitutions, either strand, an N in one read of twenty"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, n_genome, dtype=np.uint8)
    fam = rng.integers(0, 4, 60, dtype=np.uint8)
    for p in rng.integers(0, n_genome - 100, 50):
        g[p:p + 60] = fam
    cut = n_genome // 2
    parts = [g[:cut], g[cut:]]
    seq = np.concatenate([parts[0], [7], parts[1], [7]]).astype(np.uint8)
    comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    reads = []
    for _ in range(n_reads):
        ln = int(rng.integers(30, 601))
        kind = int(rng.integers(0, 3))                       # 0 insertion, 1 deletion, 2 intron
        gap = int(rng.integers(25, 2901)) if kind == 2 else int(rng.integers(1, 21))
        a = int(rng.integers(0, ln + 1 - (gap if kind == 0 else 0)))
        t = parts[int(rng.integers(0, 2))]
        if kind == 0:
            b = ln - a - gap
            p = int(rng.integers(0, len(t) - (a + b) + 1))
            r = np.concatenate([t[p:p + a], rng.integers(0, 4, gap, dtype=np.uint8), t[p + a:p + a + b]])
        else:
            b = ln - a
            p = int(rng.integers(0, len(t) - (ln + gap) + 1))
            r = np.concatenate([t[p:p + a], t[p + a + gap:p + a + gap + b]])
        assert len(r) == ln
        for q in rng.choice(ln, int(rng.integers(0, 4)), replace=False):
            r[q] = (r[q] + rng.integers(1, 4)) % 4
        if rng.integers(0, 2):
            r = comp[r[::-1]]
        if rng.integers(0, 20) == 0:
            r[int(rng.integers(0, ln))] = 4
        reads.append(r.astype(np.uint8))
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return seq, [("s1", cut), ("s2", n_genome - cut)], np.concatenate(reads), offs, lens


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    d = tmp_path_factory.mktemp("indelsweep")
    seq, entries, bases, offs, lens = sweep_case()
    sa = suffix_array(seq)
    paths = {}
    for el in (4, 5):
        paths[el] = str(d / f"sweep{el}.sfx")
        helpers.write_sfx(paths[el], "sweep", entries, seq, sa.astype(np.uint64) if el == 5 else sa, el_size=el)
    o = helpers.OracleSfx(paths[4])
    exp, eseg = helpers.oracle_align_indel(o, bases, offs, lens, helpers.make_params(**SWEEP_KW), nthreads=8)
    o.close()
    return paths, bases, offs, lens, exp, eseg


@pytest.mark.parametrize("el_size", [4, 5])
def test_planted_gaps_anywhere_match_oracle(sweep, el_size):
    """-a20 -A3000 on the sweep: the GPU equals the oracle exactly; more than a fifth of the planted reads are placed in two segments (0.51
    with this seed, from the oracle alone on the CPU)"""
    bk = _bk()
    paths, bases, offs, lens, exp, eseg = sweep
    assert np.count_nonzero(eseg["flags"] & 5) > SWEEP_READS // 5
    with bk.Aligner(paths[el_size], bk.AlignParams(**SWEEP_KW)) as al:
        assert al.lib.bk_sfx_el_size(al.h) == el_size
        got = al.align(bases, offs, lens)
        seg = al.batch_seg2()
    assert_hits_equal(got, exp)
    assert_seg2_equal(seg, eseg)
