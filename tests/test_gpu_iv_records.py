"""GPU tests of the interval records' ownership (run with -m gpu on an MI355X): nothing clears the records between phases or batches,
so every (read, strand, core) slot a kernel behind the search reads must have been stored by that phase's search - empty results
included - and slots of cores a read does not have must never be looked at.  "iv_poison" (bk_ctx_tune) fills the slots a phase can
use with ones in front of its search: a slot read without having been written then changes results and counters.  Everything runs on
the `repeat` golden index and is compared with the CPU oracle, or with the same batch on a fresh context."""
import os

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

FIELDS = ["chrom_id", "match_loci", "match_len", "low_hit_instances", "rslt", "nar", "strand", "low_mm",
          "nxt_low_mm", "num_hits", "mismatches"]
COMP = np.array([3, 2, 1, 0, 4, 5, 6, 7], dtype=np.uint8)
IMAGES = {"every_table": (), "lean_image": (("use_k3", 0), ("use_ktab2", 0))}


def _bk():
    import biokanga_amd
    return biokanga_amd


@pytest.fixture(scope="module")
def repeat(golden_tmp):
    path = os.path.join(golden_tmp["repeat"], "genome.sfx")
    seq, sa, ents = helpers.read_sfx(path)
    return {"sfx": path, "seq": seq, "sa": sa, "ents": ents}


@pytest.fixture(scope="module")
def repeat_el5(repeat, tmp_path_factory):
    """the same index with 5-byte suffix elements: separate start / count arrays instead of one word per slot"""
    path = str(tmp_path_factory.mktemp("iv_el5") / "genome5.sfx")
    helpers.write_sfx(path, "repeat5", repeat["ents"], repeat["seq"], repeat["sa"].astype(np.uint64), el_size=5)
    return path


def _cut_reads(seq, rng, lens, max_e=4, n_with_n=0, many_n=0):
    """reads cut from the target, either strand, 0 .. max_e substitutions; the first n_with_n with one N, the next many_n with a quarter of
    their bases N (the read preparation finishes those)"""
    rows = []
    for k, L in enumerate(lens):
        L = int(L)
        while True:
            s = int(rng.integers(0, len(seq) - L))
            w = seq[s:s + L] & 7
            if not (w > 3).any():
                break
        w = w.copy()
        for p in rng.choice(L, size=int(rng.integers(0, max_e + 1)), replace=False):
            w[p] = (w[p] + 1 + rng.integers(0, 3)) & 3
        if rng.integers(0, 2):
            w = COMP[w[::-1]]
        if k < n_with_n:
            w[int(rng.integers(0, L))] = 4
        elif k < n_with_n + many_n:
            w[rng.choice(L, size=L // 4, replace=False)] = 4
        rows.append(w)
    return _batch(rows)


def _batch(rows):
    lens = np.array([len(w) for w in rows], dtype=np.uint32)
    offs = np.concatenate(([0], np.cumsum(lens[:-1], dtype=np.uint64))).astype(np.uint64)
    return np.ascontiguousarray(np.concatenate(rows), dtype=np.uint8), offs, lens


def _random_reads(rng, lens, n_with_n=0):
    rows = []
    for k, L in enumerate(lens):
        w = rng.integers(0, 4, size=int(L)).astype(np.uint8)
        if k < n_with_n:
            w[rng.choice(int(L), size=int(rng.integers(1, 3)), replace=False)] = 4
        rows.append(w)
    return _batch(rows)


def _assert_records(got, exp, what):
    for f in FIELDS:
        if not np.array_equal(got[f], exp[f]):
            bad = np.nonzero(got[f] != exp[f])[0]
            i = int(bad[0])
            raise AssertionError(f"{what}: field {f}: {len(bad)} reads differ; first {i}: device {got[i]} oracle {exp[i]}")


def _oracle(path, batch, **kw):
    o = helpers.OracleSfx(path)
    exp, ctr = o.align(*batch, helpers.make_params(**kw))
    o.close()
    return exp, ctr


# one oracle run per (index, batch size), shared by the knob combinations below
@pytest.fixture(scope="module")
def mixed(repeat, repeat_el5):
    out = {}
    for n in (63, 257, 1500):
        rng = np.random.default_rng(4100 + n)
        batch = _cut_reads(repeat["seq"], rng, rng.choice([40, 70, 100], size=n), n_with_n=n // 20)
        exp, ctr = _oracle(repeat["sfx"], batch, max_subs=3)
        out[n] = (batch, exp, ctr)
    return out


@pytest.mark.parametrize("lazy", [0, 1], ids=["verified_buckets", "unverified_buckets"])
@pytest.mark.parametrize("image", sorted(IMAGES))
@pytest.mark.parametrize("el_size", [4, 5], ids=["4_byte_elements", "5_byte_elements"])
@pytest.mark.parametrize("n_reads", [63, 257, 1500])
def test_mixed_read_lengths_with_poisoned_records(repeat, repeat_el5, mixed, n_reads, el_size, image, lazy):
    """reads of 40 / 70 / 100 bases in one batch: another core count per read in every phase, so every phase has slots of cores some of
    its reads do not have - poisoned, never written, never to be read"""
    bk = _bk()
    batch, exp, octr = mixed[n_reads]
    assert len(set(np.unique(exp["rslt"]))) > 1
    with bk.Aligner(repeat["sfx"] if el_size == 4 else repeat_el5, bk.AlignParams(max_subs=3)) as al:
        assert al.lib.bk_sfx_el_size(al.h) == el_size
        for kv in IMAGES[image]:
            al.tune(*kv)
        al.tune("lazy_search", lazy)
        assert al.tune("iv_poison", 1) == 0
        for sync in (1, 0):                     # the schedule that launches everything from bounds, and the one that reads its counts back
            al.tune("async_phases", sync)
            al.counters(reset=True)
            got = al.align(*batch)
            ctr = al.counters()
            what = f"{n_reads} reads, {image}, lazy {lazy}, async_phases {sync}"
            _assert_records(got, exp, what)
            assert (ctr["n_search"], ctr["n_cand"]) == (octr.n_search, octr.n_cand), what
        assert al.tune("iv_poison", 0) == 1


@pytest.mark.parametrize("poison", [0, 1], ids=["stale_records", "poisoned_records"])
@pytest.mark.parametrize("image", sorted(IMAGES))
def test_second_batch_on_a_used_context_equals_a_fresh_context(repeat, image, poison):
    """a batch of repeat-derived reads leaves large intervals in most slots; the batch behind it on the same context - reads that match
    nowhere, reads with an N, longer active lists in the late phases - must not see any of them"""
    bk = _bk()
    n = 3000
    rng = np.random.default_rng(977)
    first = _cut_reads(repeat["seq"], rng, np.full(n, 100), max_e=2)
    second = _random_reads(rng, rng.choice([60, 100], size=n), n_with_n=n // 4)

    def run(batches):
        with bk.Aligner(repeat["sfx"], bk.AlignParams(max_subs=3)) as al:
            for kv in IMAGES[image]:
                al.tune(*kv)
            al.tune("iv_poison", poison)
            for b in batches:
                al.counters(reset=True)
                got = al.align(*b)
                ctr = al.counters()
        return got, ctr

    fresh, c_fresh = run([second])
    used, c_used = run([first, second])
    assert used.tobytes() == fresh.tobytes()
    assert c_used == c_fresh
    exp, octr = _oracle(repeat["sfx"], second, max_subs=3)
    _assert_records(used, exp, f"second batch, {image}, iv_poison {poison}")
    assert (c_used["n_search"], c_used["n_cand"]) == (octr.n_search, octr.n_cand)


def test_result_records_byte_for_byte(repeat):
    """reads that finish in every phase (0 .. 5 substitutions at -s3), reads that never align, reads the preparation finishes (too many
    N): the fields are the oracle's, and a read without an alignment has the record the layout prescribes - zeros, its NAR, strand '?'"""
    bk = _bk()
    rng = np.random.default_rng(31)
    n = 1200
    cut = _cut_reads(repeat["seq"], rng, rng.choice([70, 100], size=n), max_e=5, n_with_n=40, many_n=60)
    rnd = _random_reads(rng, np.full(300, 100), n_with_n=30)
    batch = _batch([cut[0][int(o):int(o) + int(l)] for o, l in zip(cut[1], cut[2])] + [rnd[0][int(o):int(o) + int(l)] for o, l in zip(rnd[1], rnd[2])])
    exp, _ = _oracle(repeat["sfx"], batch, max_subs=3)
    lost = exp["rslt"] == 0
    assert np.count_nonzero(lost) > 100 and np.count_nonzero(~lost) > 500 and len(np.unique(exp["nar"][lost])) >= 2
    want = np.zeros(int(np.count_nonzero(lost)), dtype=helpers.HIT_DTYPE)
    want["nar"] = exp["nar"][lost]
    want["strand"] = ord("?")
    for poison in (0, 1):
        with bk.Aligner(repeat["sfx"], bk.AlignParams(max_subs=3)) as al:
            al.tune("iv_poison", poison)
            got = al.align(*batch)
        _assert_records(got, exp, f"iv_poison {poison}")
        assert got[lost].tobytes() == want.tobytes()


def test_paired_ends_with_poisoned_records(golden_tmp, tmp_path):
    """-U3: the association and the orphan recovery run behind the phases, on the records the phases left"""
    from test_oracle_pe import PE_RUNS, pe_inputs
    bk = _bk()
    cfg = PE_RUNS["U3"]
    names, bases, offs, lens = pe_inputs(tmp_path)
    sfx_path = os.path.join(golden_tmp["basic"], "genome.sfx")
    pe = bk.PEParams(cfg["pe"], cfg["d"], cfg["D"], cfg.get("E", False))
    with bk.Aligner(sfx_path, bk.AlignParams(max_subs=cfg["s"])) as al:
        al.tune("iv_poison", 1)
        hits = al.pair(bases, offs, lens, al.align(bases, offs, lens), pe)
    o = helpers.OracleSfx(sfx_path)
    p = helpers.make_params(max_subs=cfg["s"])
    exp, _ = o.align(bases, offs, lens, p, nthreads=8)
    helpers.oracle_process_pe(o, p, cfg["pe"], cfg["d"], cfg["D"], cfg.get("E", False), bases, offs, lens, exp)
    o.close()
    _assert_records(hits, exp, "-U3")
    assert np.array_equal(hits["flags"] & 0x80, exp["flags"] & 0x80)


def test_micro_indels_with_poisoned_records(repeat):
    """-a 20: LocateInDels takes the reads the phases left unaligned"""
    bk = _bk()
    rng = np.random.default_rng(58)
    rows = []
    for _ in range(600):                       # target windows with a few bases taken out of, or put into, their middle
        s = int(rng.integers(0, len(repeat["seq"]) - 130))
        w = repeat["seq"][s:s + 120] & 7
        if (w > 3).any():
            continue
        d = int(rng.integers(0, 8))
        w = np.concatenate((w[:50], w[50 + d:100 + d])) if rng.integers(0, 2) else np.concatenate((w[:50], rng.integers(0, 4, size=d).astype(np.uint8), w[50:100 - d]))
        rows.append(np.ascontiguousarray(w, dtype=np.uint8))
    batch = _batch(rows)
    kw = dict(max_subs=3, micro_indel_len=20)
    o = helpers.OracleSfx(repeat["sfx"])
    exp, eseg = helpers.oracle_align_indel(o, *batch, helpers.make_params(**kw))
    o.close()
    with bk.Aligner(repeat["sfx"], bk.AlignParams(**kw)) as al:
        al.tune("iv_poison", 1)
        got = al.align(*batch)
        seg = al.batch_seg2()
    _assert_records(got, exp, "-a 20")
    for f in ("match_loci", "match_len", "read_ofs", "mismatches", "flags", "score"):
        assert np.array_equal(seg[f], eseg[f]), f
