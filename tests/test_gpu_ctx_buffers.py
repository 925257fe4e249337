"""GPU tests of the context's grown-on-demand buffers (run with -m gpu on an MI355X): one context is taken through every path that grows
a buffer group - batch scratch, pass B's work list, sort buffers, the staging set of host batches with the packed form's 16-bit lengths,
the second-segment buffer, the loci temporaries - with sizes that leave each group in turn too small, large enough and too small again.
Every result is compared with what a fresh context gives for the same call (the results the rest of the suite holds to the oracle).
Who frees what, and when, is checked on the host (test_host_devbuf.py); free device memory is not measured here - on a shared card it
moves under other processes."""
import os

import numpy as np
import pytest

import helpers
from test_gpu_iv_records import COMP, _batch, _cut_reads
from test_gpu_parity import assert_hits_equal

pytestmark = pytest.mark.gpu


def _bk():
    import biokanga_amd
    return biokanga_amd


@pytest.fixture(scope="module")
def repeat(golden_tmp):
    path = os.path.join(golden_tmp["repeat"], "genome.sfx")
    seq, sa, _ = helpers.read_sfx(path)
    return {"sfx": path, "seq": seq, "sa": sa}


def _reads(repeat, seed, n, lo, hi, n_with_n=0):
    rng = np.random.default_rng(seed)
    return _cut_reads(repeat["seq"], rng, rng.integers(lo, hi + 1, size=n), max_e=3, n_with_n=n_with_n)


def _pairs(repeat, seed, n_pairs, read_len=100):
    """mates of fragments of 250 .. 450 bases cut from the target: PE1 from the fragment's start, PE2 the reverse complement of its end"""
    rng = np.random.default_rng(seed)
    seq, rows = repeat["seq"], []
    while len(rows) < 2 * n_pairs:
        frag = int(rng.integers(250, 451))
        s = int(rng.integers(0, len(seq) - frag))
        w = seq[s:s + frag] & 7
        if (w > 3).any():
            continue
        rows += [w[:read_len].copy(), COMP[w[frag - read_len:][::-1]]]
    return _batch(rows)


def _repeat_derived_reads(repeat, seed, n_rep, n_other, read_len=40):
    """n_rep reads that lie in the target more than once - a 40-mer that two neighbours of the suffix array share (one in twenty do: the
    index's repeat family, 2 .. 9 copies each), either strand - among n_other ordinary ones of 40 .. 100 bases"""
    rng = np.random.default_rng(seed)
    seq, sa, rows = repeat["seq"], repeat["sa"], []
    while len(rows) < n_rep:
        i = int(rng.integers(0, len(sa) - 1))
        w = seq[int(sa[i]):int(sa[i]) + read_len] & 7
        if len(w) < read_len or (w > 3).any() or not np.array_equal(w, seq[int(sa[i + 1]):int(sa[i + 1]) + read_len] & 7):
            continue
        rows.append(COMP[w[::-1]] if rng.integers(0, 2) else w.copy())
    bases, offs, lens = _cut_reads(seq, rng, rng.integers(40, 101, size=n_other), max_e=3)
    rows += [bases[int(o):int(o) + int(n)] for o, n in zip(offs, lens)]
    return _batch([rows[k] for k in rng.permutation(len(rows))])


def _fresh(repeat, kw, fn):
    bk = _bk()
    with bk.Aligner(repeat["sfx"], bk.AlignParams(**kw)) as al:
        return fn(al)


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp), f"{what}: differs from a fresh context's"


def test_one_context_through_growing_and_shrinking_batches(repeat):
    bk = _bk()
    kw = dict(max_subs=3)
    small = _reads(repeat, 1, 63, 40, 60)
    mid = _reads(repeat, 2, 257, 20, 150, n_with_n=9)
    pairs = _pairs(repeat, 3, 40)
    large = _reads(repeat, 4, 1500, 20, 300)
    most = _reads(repeat, 5, 2000, 20, 150, n_with_n=25)
    pe = bk.PEParams(pe_mode=3, pair_min_len=100, pair_max_len=1000)

    def do_pair(al):
        return al.pair(*pairs, al.align(*pairs), pe)

    steps = [("align 63", lambda al: al.align(*small)),
             ("align_packed 257", lambda al: al.align_packed(*bk.pack_reads(*mid))),
             ("pair 40", do_pair),
             ("align 1500", lambda al: al.align(*large)),
             ("align_packed 63", lambda al: al.align_packed(*bk.pack_reads(*small))),
             ("align_packed 2000", lambda al: al.align_packed(*bk.pack_reads(*most))),
             ("align 63 again", lambda al: al.align(*small))]
    with bk.Aligner(repeat["sfx"], bk.AlignParams(**kw)) as al:
        got = [fn(al) for _, fn in steps]
    exp = {}
    for (what, fn), g in zip(steps, got):
        key = what.replace(" again", "")
        if key not in exp:
            exp[key] = _fresh(repeat, kw, fn)
        assert_hits_equal(g, exp[key])
    assert_hits_equal(got[4], got[0])                 # (the packed form of a batch gives what its byte form gives)
    assert int((got[2]["nar"] == 1).sum()) > 0        # the pair pass had accepted reads to look at


def test_reserve_then_a_larger_batch(repeat):
    bk = _bk()
    kw = dict(max_subs=3)
    b200 = _reads(repeat, 11, 200, 40, 100)
    b1500 = _reads(repeat, 12, 1500, 40, 200)
    with bk.Aligner(repeat["sfx"], bk.AlignParams(**kw)) as al:
        al.reserve(300, 100)
        got = [al.align(*b200), al.align(*b1500)]
        al.reserve(100, 50)                           # (nothing to do: everything is larger already)
        got.append(al.align(*b200))
    e200, e1500 = _fresh(repeat, kw, lambda a: a.align(*b200)), _fresh(repeat, kw, lambda a: a.align(*b1500))
    for g, e in zip(got, (e200, e1500, e200)):
        assert_hits_equal(g, e)


@pytest.mark.parametrize("kw", [dict(max_subs=3, max_ml=5, min_chimeric_len=50), dict(max_subs=3, max_ml=5, best_matches=1)], ids=["max_ml", "best_matches"])
def test_multi_loci_modes_on_a_used_context(repeat, kw):
    """the loci lists of a batch cut into chunks of 97 reads (several chunks: the later ones append behind the earlier ones' loci) on a
    context an ordinary batch has sized, against one chunk on a fresh context"""
    bk = _bk()
    batch = _repeat_derived_reads(repeat, 22, 300, 100)
    n = len(batch[2])
    first = _reads(repeat, 21, 1500, 40, 200)

    def run(al):
        hits = al.align(*batch)
        return (hits,) + al.batch_loci(n) + (al.batch_loci_trims(),)

    with bk.Aligner(repeat["sfx"], bk.AlignParams(**kw)) as al:
        al.align(*first)
        al.tune("chunk_reads", 97)
        got = run(al)
    exp = _fresh(repeat, kw, run)
    assert_hits_equal(got[0], exp[0])
    for g, e, what in zip(got[1:], exp[1:], ("loci offsets", "loci", "loci trims")):
        _same(g, e, what)
    assert int(exp[1][-1]) == len(exp[2]) and (np.diff(exp[1].astype(np.int64)) > 1).any()          # lists of more than one locus among them
    assert len(exp[3]) == (len(exp[2]) if kw.get("min_chimeric_len") else 0)


def test_micro_indels_then_pairs_share_seg2(repeat):
    """the second-segment buffer grows in the batch driver (300 reads), then in the pair pass (200 pairs), and is then large enough"""
    bk = _bk()
    kw = dict(max_subs=3, micro_indel_len=5, min_chimeric_len=50)
    b300 = _reads(repeat, 31, 300, 60, 150)
    pairs = _pairs(repeat, 32, 200)
    pe = bk.PEParams(pe_mode=3, pair_min_len=100, pair_max_len=1000)

    def align_seg2(al):
        return al.align(*b300), al.batch_seg2()

    def align_pairs(al):
        return al.align(*pairs), al.batch_seg2()

    e_hits, e_seg2 = _fresh(repeat, kw, align_seg2)
    p_hits, p_seg2 = _fresh(repeat, kw, align_pairs)
    e_pair = _fresh(repeat, kw, lambda al: al.pair(*pairs, p_hits.copy(), pe, seg2=p_seg2.copy()))
    with bk.Aligner(repeat["sfx"], bk.AlignParams(**kw)) as al:
        g1 = align_seg2(al)
        g_pair = al.pair(*pairs, p_hits.copy(), pe, seg2=p_seg2.copy())
        g2 = align_seg2(al)
    for g in (g1, g2):
        assert_hits_equal(g[0], e_hits)
        _same(g[1], e_seg2, "second segments")
    assert_hits_equal(g_pair[0], e_pair[0])
    _same(g_pair[1], e_pair[1], "second segments behind the pair pass")
    assert len(e_seg2) == 300 and len(g_pair[1]) == 400


def test_timing_kinds(repeat):
    """what the timed spans of a batch count into (bk_timing): the search span holds pass A and pass B, the call holds every span"""
    bk = _bk()
    with bk.Aligner(repeat["sfx"], bk.AlignParams(max_subs=3)) as al:
        al.align(*_reads(repeat, 41, 1500, 40, 200))
        t = al.timing()
    assert t["n_search_launches"] > 0 and t["n_extend_launches"] > 0 and t["n_search_b_launches"] > 0, t
    assert t["ms_search"] >= t["ms_search_a"] + t["ms_search_b"], t
    assert t["ms_total"] >= t["ms_search"] + t["ms_extend"] + t["ms_heavy"], t
