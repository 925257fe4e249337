"""The read preparation that also runs phase 0's pass A ("prep_search0", k_prep_fused<.., SEARCH0> in biokanga_amd/csrc/bk_prep.hip).
The lane that built a read's rows goes on to look the read's phase-0 core up - from the bases it holds - and stores the interval records
in slots numbered by READ (bk_iv_slot.h), where pass A as a launch of its own numbers them by position in the active list.  Nothing a
batch leaves may change: the phase-0 records of the two settings are compared with the reference's LocateFirstExact / LocateLastExact
(restated in the oracle) and with each other read by read, the result records and the three counters byte for byte - for reads handed
in as bytes and in the packed form, whose N the preparing lane has to take from the exception list.

The genome (600 kbp, two sequences, an N gap in each) holds unique sequence and families of 5, 17, 64, 65 and 300 copies that share
their first 130 bases: k-mer buckets of one key, of at most 16 and of more than 16.  Reads: exact ones; 1 .. 3 substitutions inside or
beyond the first 31 bases; an N in the k-mer, among bases 16 .. 30, beyond base 31; 14, 20, 31, 96, 100, 113 and 128 bases, mixed in one
batch; reads the N policy excludes at the batch's start, in its middle and at its end, so that position and read number differ behind
them.  Before the device runs, the inputs alone have to show that every class is there: the test fails, and never skips, where it is not."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import helpers  # noqa: E402
from test_gpu_search_split import COMP, FIELDS, KIND_MASK, LAZY, LAZY_BUCKET, _core_offsets, _plan  # noqa: E402

pytestmark = pytest.mark.gpu

N_GENOME = 600_000
MAX_SUBS = 3
MAX_NS = 1                      # the default N policy: a read of up to 199 bases may hold one
SHARED, OWN = 130, 70
FAMILIES = (5, 17, 64, 65, 300)
LENGTHS = (14, 20, 31, 96, 100, 113, 128)
KINDS = ("exact", "sub_in", "fam", "n_kmer", "sub_out", "n_keys", "fam", "n_far", "exact", "excluded", "fam_sub")
SIZES = (1, 63, 64, 65, 257, 1500)
SEED = 7301


def _bk():
    import biokanga_amd
    return biokanga_amd


def family_genome(seed=SEED):
    rng = np.random.default_rng(seed)
    copies = []
    for f, n_copies in enumerate(FAMILIES):
        shared = rng.integers(0, 4, SHARED, dtype=np.uint8)
        for _ in range(n_copies):
            copies.append((f, np.concatenate([shared, rng.integers(0, 4, OWN, dtype=np.uint8)])))
    total = len(copies) * (SHARED + OWN)
    order = rng.permutation(len(copies))
    gaps = rng.multinomial(N_GENOME - total - 2000, np.full(len(copies) + 1, 1.0 / (len(copies) + 1)))
    g = rng.integers(0, 4, N_GENOME, dtype=np.uint8)
    cut = N_GENOME // 2
    spots = [[] for _ in FAMILIES]
    at = 0
    for k, i in enumerate(order):
        at += int(gaps[k])
        if at < cut < at + SHARED + OWN:              # (no copy lies across the two sequences' boundary)
            at = cut + 1
        f, cp = copies[i]
        g[at:at + len(cp)] = cp
        spots[f].append(at)
        at += len(cp)
    assert at < N_GENOME
    # an N gap inside each sequence, in unique sequence (between two copies)
    taken = np.zeros(N_GENOME, dtype=bool)
    for fam_spots in spots:
        for s in fam_spots:
            taken[s:s + SHARED + OWN] = True
    for lo, hi in ((cut // 3, cut // 2), (cut + cut // 3, cut + cut // 2)):
        free = [p for p in range(lo, hi) if not taken[p:p + 60].any()]
        g[free[0]:free[0] + 60] = 4
    seq = np.concatenate([g[:cut], [7], g[cut:], [7]]).astype(np.uint8)
    return g, seq, cut, [np.array(s) for s in spots]


def make_read(rng, g, spots, kind, length):
    """one read in the genome's orientation, then either strand"""
    while True:
        if kind in ("fam", "fam_sub"):
            starts = spots[int(rng.integers(0, len(spots)))]                 # (a family, then one of its copies)
            st = int(starts[int(rng.integers(0, len(starts)))]) + int(rng.integers(0, 20))
        else:
            st = int(rng.integers(0, N_GENOME - length - 1))
        r = g[st:st + length].copy()
        if not (r == 4).any():
            break
    def subst(positions):
        for q in positions:
            r[q] = (r[q] + rng.integers(1, 4)) % 4
    if kind == "sub_in":
        subst(rng.choice(min(31, length), int(rng.integers(1, MAX_SUBS + 1)), replace=False))
    elif kind in ("sub_out", "fam_sub") and length > 34:
        subst(31 + rng.choice(length - 31, int(rng.integers(1, MAX_SUBS + 1)), replace=False))
    elif kind == "n_kmer":
        r[int(rng.integers(0, 8))] = 4
    elif kind == "n_keys" and length > 16:
        r[int(rng.integers(16, min(31, length)))] = 4
    elif kind == "n_far" and length > 32:
        r[int(rng.integers(32, length))] = 4
    elif kind == "excluded":
        r[rng.choice(length, 3, replace=False)] = 4
    if rng.integers(0, 2):
        r = COMP[r[::-1]]
    return r


def batch_kinds(n, excluded_at_ends=True):
    kinds = [KINDS[i % len(KINDS)] for i in range(n)]
    lens = [LENGTHS[(i // 3) % len(LENGTHS)] if i % 3 == 0 else 100 for i in range(n)]
    if n >= 3 and excluded_at_ends:
        for i in (0, n // 2, n - 1):
            kinds[i] = "excluded"
    if not excluded_at_ends:
        kinds = ["exact" if k == "excluded" else k for k in kinds]
    return kinds, lens


def batch_reads(g, spots, n, excluded=True):
    rng = np.random.default_rng(SEED + n + (0 if excluded else 100000))
    kinds, lens = batch_kinds(n, excluded)
    reads = [make_read(rng, g, spots, k, l) for k, l in zip(kinds, lens)]
    lens = np.array(lens, dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    return np.concatenate(reads).astype(np.uint8), offs, lens


def read_rows(bases, offs, lens):
    """per read (forward, reverse complement)"""
    out = []
    for o, l in zip(offs.tolist(), lens.tolist()):
        b = bases[int(o):int(o) + int(l)] & 7
        out.append((b, COMP[b[::-1]]))
    return out


class Expected:
    """what the oracle and the restated rules say of one batch, computed once: the N policy's verdict, phase 0's core of every read and
    its interval on either strand, and per align_strand the result records and the counters"""

    def __init__(self, osfx, batch, mcl):
        bases, offs, lens = batch
        self.n = n = len(lens)
        rows = read_rows(bases, offs, lens)
        num_ns = np.array([int((f == 4).sum()) for f, _ in rows])
        self.listed = num_ns <= np.maximum((lens.astype(np.int64) * MAX_NS) // 100, MAX_NS)      # Aligner.cpp:9041-9063
        self.cl = np.zeros(n, dtype=np.int32)
        self.n_cores = np.zeros(n, dtype=np.int32)
        flat, p_ofs, p_len, at = [], [], [], 0
        for r, (f, v) in enumerate(rows):
            phases, max_slides = _plan(len(f), MAX_SUBS, mcl)
            cl, cd = phases[0]
            cores = _core_offsets(len(f), cl, cd, max_slides)
            assert len(cores) <= 1 and (not cores or cores[0] == 0), "phase 0 of a read has one core at most, at offset 0"
            self.cl[r], self.n_cores[r] = cl, len(cores)
            flat += [f, v]
            p_ofs += [at, at + len(f)]
            p_len += [min(cl, len(f))] * 2
            at += 2 * len(f)
        flat = np.ascontiguousarray(np.concatenate(flat))
        p_ofs, p_len = np.array(p_ofs, dtype=np.uint64), np.array(p_len, dtype=np.int32)
        fi, la = np.zeros(2 * n, dtype=np.int64), np.zeros(2 * n, dtype=np.int64)
        osfx.lib.ora_locate_cores(osfx.h, flat.ctypes.data, p_ofs.ctypes.data, p_len.ctypes.data, 2 * n, fi.ctypes.data, la.ctypes.data, 8)
        self.e_first = (fi - 1).reshape(n, 2)
        self.e_n = np.where(fi > 0, la - fi + 1, 0).reshape(n, 2)
        self.rows = rows
        self.hits = {}
        for strand in (0, 1, 2):
            self.hits[strand] = osfx.align(bases, offs, lens, helpers.make_params(max_subs=MAX_SUBS, align_strand=strand), nthreads=8)


def class_counts(exp):
    """reads of each class in a batch, from its bases and the oracle's intervals alone (either strand counts)"""
    c = dict.fromkeys(("exact", "sub_in", "sub_out", "n_kmer", "n_keys", "n_far", "excluded", "bucket_1", "bucket_small", "bucket_big") +
                      tuple(f"len_{l}" for l in LENGTHS), 0)
    for r, (f, v) in enumerate(exp.rows):
        ns = np.flatnonzero(f == 4)
        c[f"len_{len(f)}"] = c.get(f"len_{len(f)}", 0) + 1
        if not exp.listed[r]:
            c["excluded"] += 1
            continue
        for row in (f, v):
            nr = np.flatnonzero(row == 4)
            c["n_kmer"] += int((nr < 8).any())
            c["n_keys"] += int(((nr >= 16) & (nr <= 30)).any())
            c["n_far"] += int((nr >= 32).any())
        if ns.size == 0 and exp.n_cores[r]:
            c["exact"] += int(exp.e_n[r].max() > 0)
    return c


def phase0_records(al, batch, packed):
    """the interval records phase 0's search left, by read: first[strand, read], raw count[strand, read] of core 0, listed[read]"""
    bk = _bk()
    bases, offs, lens = batch
    n = len(lens)
    al.tune("debug_stop_phase", 1)
    try:
        al.timing(reset=True)
        if packed:
            al.align_packed(*bk.pack_reads(bases, offs, lens))
        else:
            al.align(bases, offs, lens)
        ms_search_a = al.timing()["ms_search_a"]
        na, ivc = ctypes.c_uint32(0), ctypes.c_uint32(0)
        assert al.lib.bk_debug_intervals(al.h, 0, ctypes.byref(na), ctypes.byref(ivc), None, None, None) == 0
        m, c = int(na.value), int(ivc.value)
        act = np.zeros(max(m, 1), dtype=np.uint32)
        first = np.zeros((2 * c, max(m, 1)), dtype=np.uint64)
        count = np.zeros((2 * c, max(m, 1)), dtype=np.uint32)
        if m:
            assert al.lib.bk_debug_intervals(al.h, m, ctypes.byref(na), ctypes.byref(ivc), act.ctypes.data, first.ctypes.data, count.ctypes.data) == 0
    finally:
        al.tune("debug_stop_phase", 0)
    act = act[:m]
    assert len(np.unique(act)) == m and (m == 0 or act.max() < n)
    f = np.zeros((2, n), dtype=np.uint64)
    q = np.zeros((2, n), dtype=np.uint32)
    listed = np.zeros(n, dtype=bool)
    listed[act] = True
    f[:, act] = first[[0, c], :m]
    q[:, act] = count[[0, c], :m]
    return f, q, listed, ms_search_a


def check_phase0(exp, f, q, listed, strand, lazy, what):
    assert np.array_equal(listed, exp.listed), f"{what}: the first active list holds other reads than the N policy lets through"
    has = listed & (exp.n_cores > 0)
    n_probes = 0
    for st in ((0, 1) if strand == 0 else ((0,) if strand == 1 else (1,))):
        e_first, e_n = exp.e_first[has, st], exp.e_n[has, st]
        got_first, raw = f[st, has].astype(np.int64), q[st, has]
        got_n = (raw & KIND_MASK).astype(np.int64)
        assert not ((raw >> 30) & 1).any(), f"{what}: a work item, an element record or a slot nobody wrote is left in a record of strand {st}"
        is_lazy = (raw & LAZY) != 0
        assert lazy or not is_lazy.any(), f"{what}: a lazy record with lazy_search off"
        inside = (e_n == 0) | ((got_first <= e_first) & (e_first + e_n <= got_first + got_n))
        ok = np.where(is_lazy, (got_n >= 1) & (got_n <= LAZY_BUCKET) & inside, (got_n == e_n) & ((e_n == 0) | (got_first == e_first)))
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, (f"{what}, strand {'+-'[st]}: {bad.size} probes differ, first reads {np.flatnonzero(has)[bad[:6]]}: device "
                               f"[{got_first[bad[:6]]}, +{got_n[bad[:6]]}) raw {raw[bad[:6]]}, oracle [{e_first[bad[:6]]}, +{e_n[bad[:6]]})")
        n_probes += int(has.sum())
    return n_probes


def run(al, exp, batch, strand, lazy, packed, what, expect_fused):
    """-> everything the configuration leaves, as bytes: phase 0's records of the strands it searches, by read; the result records; the
    three counters"""
    bk = _bk()
    bases, offs, lens = batch
    f, q, listed, ms_a = phase0_records(al, batch, packed)
    check_phase0(exp, f, q, listed, strand, lazy, what)
    if expect_fused is not None and exp.listed.any() and (exp.n_cores[exp.listed] > 0).any():
        assert (ms_a == 0) == expect_fused, f"{what}: pass A's own launch in phase 0 took {ms_a} ms"
    keep = [0, 1] if strand == 0 else ([0] if strand == 1 else [1])
    has = listed & (exp.n_cores > 0)
    al.counters(reset=True)
    got = al.align_packed(*bk.pack_reads(bases, offs, lens)) if packed else al.align(bases, offs, lens)
    ctr = al.counters()
    e_hits, e_ctr = exp.hits[strand]
    for fld in FIELDS:
        bad = np.flatnonzero(got[fld] != e_hits[fld])
        assert bad.size == 0, f"{what}: field {fld} differs from the oracle's for {bad.size} reads, first {bad[:5]}"
    three = (ctr["n_search"], ctr["n_cand"], ctr["n_lcm_calls"])
    assert three == (e_ctr.n_search, e_ctr.n_cand, e_ctr.n_lcm_calls), what
    return [f[keep][:, has].tobytes(), q[keep][:, has].tobytes(), listed.tobytes(), got.tobytes(), repr(three).encode()]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import torch
    bk = _bk()
    g, seq, cut, spots = family_genome()
    n = len(seq)
    dev = torch.device("cuda:0")
    d_seq = torch.from_numpy(seq).to(dev)
    d_sa = torch.empty(n, dtype=torch.int32, device=dev)
    bk.build_sa_device(d_seq.data_ptr(), n, d_sa.data_ptr(), 4, 0)          # (the suffix array builder, not the search)
    sa = d_sa.cpu().numpy().view(np.uint32)
    tmp = tmp_path_factory.mktemp("prep_search0")
    paths = {}
    for el_size in (4, 5):
        paths[el_size] = str(tmp / f"fam{el_size}.sfx")
        helpers.write_sfx(paths[el_size], "fam", [("s1", cut), ("s2", N_GENOME - cut)], seq, sa.astype(np.uint64) if el_size == 5 else sa, el_size=el_size)
    o = helpers.OracleSfx(paths[4])
    with bk.Aligner(paths[4], bk.AlignParams(max_subs=MAX_SUBS)) as al:
        mcl = al.min_core_len
    batches = {size: batch_reads(g, spots, size) for size in SIZES}
    batches["257 without excluded reads"] = batch_reads(g, spots, 257, excluded=False)
    exp = {name: Expected(o, b, mcl) for name, b in batches.items()}
    # -- from the inputs and the oracle alone: the batches hold what the test is for
    inputs_hold_every_class(exp, batches)
    yield {"paths": paths, "batches": batches, "exp": exp, "mcl": mcl}
    o.close()


def inputs_hold_every_class(exp, batches):
    c = class_counts(exp[1500])
    e = exp[1500]
    kinds, _ = batch_kinds(1500)
    for kind in ("sub_in", "sub_out"):
        c[kind] = sum(1 for r, k in enumerate(kinds) if k == kind and e.listed[r] and e.n_cores[r])
    wide = e.e_n.max(axis=1)
    # (the interval of a whole read bounds its k-mer bucket from below; a read of a unique region has a bucket of a few keys at most)
    c["bucket_1"] = int(((wide == 1) & e.listed).sum())
    c["bucket_small"] = int(((wide >= 2) & (wide <= 16) & e.listed).sum())
    c["bucket_big"] = int(((wide > 16) & e.listed).sum())
    short = [k for k, v in c.items() if v < 20]
    assert not short, f"mis-built inputs: fewer than 20 reads of {short} in the batch of 1500: {c}"
    assert len(set(batches[1500][2].tolist())) == len(LENGTHS), "mis-built inputs: the batch of 1500 does not mix the lengths"
    for size in SIZES:
        if size >= 63:
            x = exp[size]
            first_excluded = int(np.flatnonzero(~x.listed)[0])
            searched = np.flatnonzero(x.listed & (x.n_cores > 0))
            assert (searched > first_excluded).any(), f"mis-built inputs: no excluded read in front of a searched one in the batch of {size}"
            assert not x.listed[0] and not x.listed[size // 2] and not x.listed[size - 1]
    assert exp["257 without excluded reads"].listed.all()


def _set_image(al, image):
    if image == "lean":
        al.tune("use_k3", 0)
        al.tune("use_ktab2", 0)
        assert al.tune("k3_resident", 0) == 0 and al.tune("ktab2_resident", 0) == 0


@pytest.mark.parametrize("strand", [0, 1, 2], ids=["both_strands", "plus_only", "minus_only"])
@pytest.mark.parametrize("image", ["full", "lean"])
def test_prep_search0_changes_no_record(world, image, strand):
    """(the lean image has no two-word k-mer table: both settings take the two launches there, and must say so)"""
    bk = _bk()
    with bk.Aligner(world["paths"][4], bk.AlignParams(max_subs=MAX_SUBS, align_strand=strand)) as al:
        assert al.min_core_len == world["mcl"]
        _set_image(al, image)
        for lazy in (1, 0):
            al.tune("lazy_search", lazy)
            for async_phases in (1, 0):
                al.tune("async_phases", async_phases)
                for size in SIZES:
                    for packed in (False, True):
                        left = {}
                        for s0 in (1, 0):
                            al.tune("prep_search0", s0)
                            assert al.tune("prep_search0", s0) == s0
                            what = (f"{size} reads {'packed' if packed else 'as bytes'}, {image} image, align_strand {strand}, lazy {lazy}, "
                                    f"async_phases {async_phases}, prep_search0 {s0}")
                            left[s0] = run(al, world["exp"][size], world["batches"][size], strand, lazy, packed, what, bool(s0) and image == "full")
                        assert left[1] == left[0], f"{what[:-2]}: the two settings leave different bytes"


@pytest.mark.parametrize("async_phases", [1, 0])
def test_every_slot_a_consumer_reads_is_written(world, async_phases):
    """"iv_poison" fills the records with ones in front of the search: a slot of phase 0 that the preparing lane did not store, or that a
    consumer looks for at the read's position instead of its number, shows in the interval check and in the result records"""
    bk = _bk()
    with bk.Aligner(world["paths"][4], bk.AlignParams(max_subs=MAX_SUBS)) as al:
        al.tune("async_phases", async_phases)
        for lazy in (1, 0):
            al.tune("lazy_search", lazy)
            for size in SIZES:
                for packed in (False, True):
                    left = {}
                    for s0, poison in ((1, 0), (1, 1), (0, 1)):
                        al.tune("prep_search0", s0)
                        al.tune("iv_poison", poison)
                        what = f"{size} reads {'packed' if packed else 'as bytes'}, lazy {lazy}, async_phases {async_phases}, prep_search0 {s0}, iv_poison {poison}"
                        left[(s0, poison)] = run(al, world["exp"][size], world["batches"][size], 0, lazy, packed, what, bool(s0))
                    assert left[(1, 1)] == left[(1, 0)] == left[(0, 1)], f"{what}: iv_poison changes what a batch leaves"


@pytest.mark.parametrize("async_phases", [1, 0])
def test_excluded_reads_behind_a_batch_without_any(world, async_phases):
    """one context: a batch in which position and read number agree for every read, then batches in which they do not - against a fresh
    context, byte for byte (a slot or a list that outlives its batch would show)"""
    bk = _bk()

    def ctx():
        al = bk.Aligner(world["paths"][4], bk.AlignParams(max_subs=MAX_SUBS))
        al.tune("async_phases", async_phases)
        return al

    plain = "257 without excluded reads"
    with ctx() as used, ctx() as fresh:
        run(used, world["exp"][plain], world["batches"][plain], 0, 1, True, f"{plain}, async_phases {async_phases}", True)
        for size in (63, 257, 1500):
            for packed in (True, False):
                used.align(*world["batches"][plain])
                a = run(used, world["exp"][size], world["batches"][size], 0, 1, packed, f"{size} reads behind a batch without excluded reads, async_phases {async_phases}", True)
                b = run(fresh, world["exp"][size], world["batches"][size], 0, 1, packed, f"{size} reads on a fresh context, async_phases {async_phases}", True)
                assert a == b, f"{size} reads, async_phases {async_phases}: a reused context leaves other bytes than a fresh one"


@pytest.mark.parametrize("which", ["5_byte_elements", "no_ktab2"])
def test_other_configurations_keep_the_two_launches(world, which):
    bk = _bk()
    with bk.Aligner(world["paths"][5 if which == "5_byte_elements" else 4], bk.AlignParams(max_subs=MAX_SUBS)) as al:
        if which == "no_ktab2":
            al.tune("use_ktab2", 0)
            assert al.tune("ktab2_resident", 0) == 0
        assert al.tune("prep_search0", 1) == 1
        for size in (65, 1500):
            for packed in (False, True):
                run(al, world["exp"][size], world["batches"][size], 0, 1, packed, f"{size} reads, {which}", False)
