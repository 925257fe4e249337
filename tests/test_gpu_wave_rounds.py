"""The wave kernel's rounds (biokanga_amd/csrc/bk_wave.hip): the length-specialised forms k_wave<8, .., ND> and the lean round change no
record and no counter.  The genome is made of repeat families whose copy counts put the reference's sequential rules on and next to the
boundaries of a round of 64 candidates: 64 / 65 / 66 copies (one round and just beyond), 99 .. 165 (the copy check at IterCnt == 100, on and
beside a boundary), 400 and 900 (long walks, where the lean round runs), exact families of 70 and 300 (more than max_hits candidates
without mismatch in one round: the early exit cuts inside it), and two large families run under the PMode whose MaxIter is 2500: one
beyond MaxIter + 100, which the copy check abandons, and one a few dozen copies above MaxIter, which is walked until the MaxIter stop
fires in the middle of a round.  The copies are laid side by side, never over each other, so the counts are what the table says; the
divergent copies make longer cores select parts of the runs.

Every batch is a uniform length that picks one compiled form - 96 (ND 6, no partial dword), 97 / 100 / 112 (ND 7), 113 / 128 (ND 8), 75
with -s2 (ND 5) - or mixed 96 .. 113, which has to take the generic form (the rule itself: tests/test_host_wave_form.py).  Each runs with
"wave_len_spec" 1 and 0, the window array on and off, and with every read through the wave kernel; all give the oracle's records and
counters, and the two "wave_len_spec" settings the same bytes.

The node cap (1 024 000 candidates of one strand pass) cannot be reached by a genome of this size; its branch is covered by the `repeat`
golden of tests/test_gpu_parity.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import helpers  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("chrom_id", "match_loci", "match_len", "low_hit_instances", "rslt", "nar", "strand", "low_mm", "nxt_low_mm", "num_hits", "mismatches")

N_GENOME = 760_000
N_READS = 20_000
PMODE = 3                  # MaxIter 2500 (bk_image.cpp: CAligner::Align's table)
MAX_ITER = 2500
# (copies, divergence per base, family length)
FAMILIES = ((64, 0.02, 130), (65, 0.01, 130), (66, 0.03, 130),
            (99, 0.02, 130), (100, 0.01, 130), (101, 0.03, 130), (128, 0.02, 130), (129, 0.01, 130), (163, 0.03, 130), (164, 0.02, 130), (165, 0.01, 130),
            (400, 0.02, 130), (900, 0.01, 130),
            (70, 0.0, 130), (300, 0.0, 130))
# (exact copies, copies with one to three substitutions, family length): intervals of 2650 .. 2700 suffixes - num_copies at the copy
# check is beyond MaxIter - and of 2530 .. 2570: the check lets the walk go on (2570 - 100 + 2 <= 2500) and MaxIter stops it
BIG_FAMILIES = ((MAX_ITER + 150, 50, 50), (MAX_ITER + 30, 40, 50))


def _bk():
    import biokanga_amd
    return biokanga_amd


def family_genome(seed=4242):
    """-> (seq of two sequences with their ends, spots): spots[f] = the starts of family f's copies and its length"""
    rng = np.random.default_rng(seed)
    copies = []                                       # (family, bases)
    fam_len = []
    for copies_n, div, flen in FAMILIES:
        fam = rng.integers(0, 4, flen, dtype=np.uint8)
        for _ in range(copies_n):
            cp = fam.copy()
            mut = rng.random(flen) < div
            cp[mut] = (cp[mut] + rng.integers(1, 4, int(mut.sum()))) % 4
            copies.append((len(fam_len), cp))
        fam_len.append(flen)
    for exact, near, flen in BIG_FAMILIES:
        fam = rng.integers(0, 4, flen, dtype=np.uint8)
        for k in range(exact + near):
            cp = fam.copy()
            if k >= exact:
                for q in rng.choice(flen, int(rng.integers(1, 4)), replace=False):
                    cp[q] = (cp[q] + rng.integers(1, 4)) % 4
            copies.append((len(fam_len), cp))
        fam_len.append(flen)
    total = sum(len(cp) for _, cp in copies)
    assert total < N_GENOME - 20_000
    order = rng.permutation(len(copies))
    gaps = rng.multinomial(N_GENOME - total, np.full(len(copies) + 1, 1.0 / (len(copies) + 1)))
    g = rng.integers(0, 4, N_GENOME, dtype=np.uint8)
    spots = [[] for _ in fam_len]
    at = 0
    for k, i in enumerate(order):
        at += int(gaps[k])
        f, cp = copies[i]
        g[at:at + len(cp)] = cp
        spots[f].append(at)
        at += len(cp)
    cut = N_GENOME // 2
    seq = np.concatenate([g[:cut], [7], g[cut:], [7]]).astype(np.uint8)
    return g, seq, cut, [(np.array(s), fam_len[f]) for f, s in enumerate(spots)]


def make_reads(g, spots, lens, max_e, seed):
    """reads of the given lengths: two in three start in or beside a copy of a family drawn evenly from the families (then a copy of it),
    each with 0 .. max_e substitutions, on either strand -> (bases, offs, lens)"""
    rng = np.random.default_rng(seed)
    comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    out = []
    for i, L in enumerate(lens):
        L = int(L)
        if i % 3:
            starts, flen = spots[int(rng.integers(0, len(spots)))]
            p = int(starts[int(rng.integers(0, len(starts)))])
            st = int(np.clip(p + rng.integers(-L // 2, flen), 0, N_GENOME - L - 1))
        else:
            st = int(rng.integers(0, N_GENOME - L - 1))
        r = g[st:st + L].copy()
        for q in rng.choice(L, int(rng.integers(0, max_e + 1)), replace=False):
            r[q] = (r[q] + rng.integers(1, 4)) % 4
        if rng.integers(0, 2):
            r = comp[r[::-1]]
        out.append(r)
    lens = np.asarray(lens, dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return np.concatenate(out), offs, lens


# name -> (read lengths, max_subs)
BATCHES = {
    "96": (np.full(N_READS, 96), 3), "97": (np.full(N_READS, 97), 3), "100": (np.full(N_READS, 100), 3), "112": (np.full(N_READS, 112), 3),
    "113": (np.full(N_READS, 113), 3), "128": (np.full(N_READS, 128), 3), "75, -s2": (np.full(N_READS, 75), 2),
    "96 .. 113 mixed": (96 + np.arange(N_READS) % 18, 3),
}


def batch_reads(g, spots, name):
    lens, max_subs = BATCHES[name]
    return make_reads(g, spots, lens, max_subs + 1, 1000 + sorted(BATCHES).index(name)), max_subs


@pytest.fixture(scope="module")
def fam(tmp_path_factory):
    import torch
    bk = _bk()
    g, seq, cut, spots = family_genome()
    n = len(seq)
    dev = torch.device("cuda:0")
    d_seq = torch.from_numpy(seq).to(dev)
    d_sa = torch.empty(n, dtype=torch.int32, device=dev)
    bk.build_sa_device(d_seq.data_ptr(), n, d_sa.data_ptr(), 4, 0)
    sa = d_sa.cpu().numpy().view(np.uint32)
    path = str(tmp_path_factory.mktemp("wave_rounds") / "fam.sfx")
    helpers.write_sfx(path, "fam", [("s1", cut), ("s2", N_GENOME - cut)], seq, sa)
    o = helpers.OracleSfx(path)
    yield {"g": g, "spots": spots, "path": path, "oracle": o}
    o.close()


def _same(got, exp, what):
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != exp[f])
        assert bad.size == 0, f"{what}: field {f} differs for {bad.size} reads, first {bad[:5]}: {got[f][bad[:5]]} vs {exp[f][bad[:5]]}"


@pytest.mark.parametrize("name", list(BATCHES))
def test_rounds_and_forms_give_the_oracles_records(fam, name):
    bk = _bk()
    (bases, offs, lens), max_subs = batch_reads(fam["g"], fam["spots"], name)
    exp, octr = fam["oracle"].align(bases, offs, lens, helpers.make_params(max_subs=max_subs, pmode=PMODE), nthreads=8)
    # from the oracle alone: the sample holds what the test is for - a MaxIter rule fires (under the 5000 PMode both large families are
    # walked whole), reads have several instances of their best hit, reads end as multi-hit
    _, c5000 = fam["oracle"].align(bases, offs, lens, helpers.make_params(max_subs=max_subs, pmode=0), nthreads=8)
    assert octr.n_cand != c5000.n_cand
    assert np.count_nonzero(exp["low_hit_instances"] > 1) >= 50
    assert np.count_nonzero(exp["nar"] == 5) >= 50                      # BK_NAR_MULTIALIGN
    with bk.Aligner(fam["path"], bk.AlignParams(max_subs=max_subs, pmode=PMODE)) as al:
        for use_swin in (2, 0):
            for heavy_thresh in (64, 0):
                recs = {}
                for spec in (1, 0):
                    what = f"reads of {name} bases, use_swin {use_swin}, heavy_thresh {heavy_thresh}, wave_len_spec {spec}"
                    al.tune("use_swin", use_swin)
                    al.tune("heavy_thresh", heavy_thresh)
                    al.tune("wave_len_spec", spec)
                    al.counters(reset=True)
                    got = al.align(bases, offs, lens)
                    ctr = al.counters()
                    _same(got, exp, what)
                    assert (ctr["n_search"], ctr["n_cand"], ctr["n_lcm_calls"]) == (octr.n_search, octr.n_cand, octr.n_lcm_calls), what
                    assert al.tune("swin_resident", 0) == (1 if use_swin else 0), what
                    recs[spec] = got.tobytes()
                assert recs[1] == recs[0], f"reads of {name} bases, use_swin {use_swin}, heavy_thresh {heavy_thresh}: the two forms' records differ"
