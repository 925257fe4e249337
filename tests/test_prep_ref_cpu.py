"""The references of tests/prep_ref.py checked on the CPU, and the inputs of tests/test_gpu_prep.py counted: every case that module's
comment names is present in the generated batches; the vectorised row forms equal the plain ones; the reference packer equals
bk_pack_reads; the refuse / keep decision equals the CPU oracle's (nar == BK_NAR_NS) at max_ns 0, 1 and 5."""
import numpy as np
import pytest

import helpers
import index_ref
import prep_ref as ref
from prep_ref import N

NWS = (8, 16, ref.NW_LONG, ref.NW_LONGEST)


def _runs_of(codes):
    """maximal runs of N: (start, length)"""
    out, j = [], 0
    while j < len(codes):
        if codes[j] == N:
            k = j
            while k < len(codes) and codes[k] == N:
                k += 1
            out.append((j, k - j))
            j = k
        else:
            j += 1
    return out


def _check_planting(case, maxlen):
    b = case.batch
    codes = b.codes()
    # every start and every run length was planted, every pair of them at least once where reads are long enough for all
    assert {name for _, name, _, _, _ in case.runs} == set(ref.N_STARTS)
    assert {run for _, _, run, _, _ in case.runs} == set(ref.N_RUNS)
    assert len({(name, run) for _, name, run, _, _ in case.runs}) == len(ref.N_STARTS) * len(ref.N_RUNS)
    assert 0.12 * b.n < len(case.runs) < 0.3 * b.n
    for i, name, run, at, cnt in case.runs:
        assert all(c == N for c in codes[i][at:at + cnt]) and cnt >= 1
    uncut = [(i, at, cnt) for i, _, run, at, cnt in case.runs if cnt == run]
    # a run crossing a 16-base word and a 32-base word, on the forward strand and - counted from the read's end - on the reverse strand
    for unit in (16, 32):
        assert sum(1 for i, at, cnt in uncut if at // unit != (at + cnt - 1) // unit) >= 3
        assert sum(1 for i, at, cnt in uncut if (len(codes[i]) - at - cnt) // unit != (len(codes[i]) - 1 - at) // unit) >= 3
    assert sum(1 for i, at, cnt in uncut if at == 0) >= 1 and sum(1 for i, at, cnt in uncut if at + cnt == len(codes[i])) >= 1
    # the special reads
    lab = case.labels
    assert all(c == N for c in codes[lab["all_n"]]) and len(codes[lab["all_n"]]) >= 1
    for code in (5, 6, 7):
        for where, at in (("first", 0), ("middle", None), ("last", -1)):
            c = codes[lab[f"code{code}_{where}"]]
            at = len(c) // 2 if at is None else at
            assert c[at] == code and sum(1 for x in c if x > 3) == 1
    for max_ns in ref.MAX_NS:
        rels = [rel for rel in ("below", "equal", "above") if f"ns{max_ns}_{rel}_at" in lab]
        if max_ns == 0:
            assert rels                                                  # (MaxNsSeq is 0 whatever the length)
        else:
            want = {"below"} | ({"equal"} if maxlen * max_ns // 100 >= max_ns else set()) | ({"above"} if maxlen * max_ns // 100 > max_ns else set())
            assert set(rels) == want, (max_ns, rels)
        for rel in rels:
            for tag, extra in (("at", 0), ("over", 1)):
                c = codes[lab[f"ns{max_ns}_{rel}_{tag}"]]
                q, m = len(c) * max_ns // 100, ref.max_ns_seq(len(c), max_ns)
                assert sum(1 for x in c if x == N) == m + extra and not any(x > N for x in c)
                if max_ns:
                    assert {"below": q < max_ns, "equal": q == max_ns, "above": q > max_ns}[rel]
                assert ref.refused(c, max_ns) == bool(extra)
    # upper bits 3..7 of the bytes are in use
    assert len(np.unique(b.bases >> 3)) == 32


@pytest.mark.parametrize("nw", NWS)
def test_fused_batches_hold_the_cases(nw):
    case = ref.fused_case(nw)
    b = case.batch
    cnt = np.bincount(b.lens, minlength=16 * nw + 1)
    assert cnt[0] == 0 and (cnt[1:] >= 5).all() and b.maxlen == 16 * nw
    assert (b.lens % 16 == 0).sum() >= 5 * nw and (b.lens % 32 == 1).sum() >= 5 * (nw // 2)
    _check_planting(case, 16 * nw)
    if nw >= 16:
        assert all(f"ns{m}_above_at" in case.labels for m in (1, 5))
    # no long run of one kind: reads with and without N within the first wave and the last
    hasn = ref.has_n_plain(b)
    assert 0 < hasn[:64].sum() < 64 and 0 < hasn[-64:].sum() < 64


def test_fused_variants_hold_the_cases():
    ns = {k: ref.fused_variant(k).n for k in ("n512", "n577", "n639")}
    assert ns["n512"] % 256 == 0 and ns["n577"] % 64 == 1 and ns["n639"] % 64 == 63 and min(ns.values()) > 256        # (full and partial waves, several blocks)
    for kind, top, wpr in (("max100", 100, 8), ("max32", 32, 4)):
        b = ref.fused_variant(kind)
        assert b.maxlen == top and ref.words_per_read(top) == wpr and b.n > 64 and b.n % 64 != 0
        assert 0 < ref.has_n_plain(b).sum() < b.n
    assert ref.words_per_read(128) == 10 and ref.fused_case(8).batch.n % 64 != 0                 # (the whole batch ends in a partial wave too)


def test_unfused_batch_holds_the_cases():
    case = ref.unfused_case()
    b = case.batch
    cnt = np.bincount(b.lens, minlength=ref.MAX_READ_LEN + 1)
    assert all(cnt[length] >= 3 for length in ref.UNFUSED_LENS) and b.maxlen == ref.MAX_READ_LEN and b.n > 250
    _check_planting(case, ref.MAX_READ_LEN)
    runs = _runs_of(b.codes()[case.labels["long_run"]])
    assert runs == [(123, 300)]
    _, _, _, exc = ref.pack_plain(b)
    mine = exc[exc["read"] == case.labels["long_run"]]
    assert len(mine) == 2 and int(mine["run"][0]) == 255 and int(mine["pos"][1]) == 123 + 256 and int(mine["run"][1]) == 300 - 256 - 1
    # a batch of (a) that the unfused path takes as well
    assert ref.fused_case(ref.NW_LONGEST).batch.maxlen <= 512


def _small_batches():
    return [ref.fused_case(nw).batch for nw in NWS] + [ref.fused_variant(k) for k in ref.FUSED_VARIANTS] + [ref.unfused_case().batch]


def test_vectorised_rows_equal_the_plain_ones():
    for b in _small_batches():
        wpr = ref.words_per_read(b.maxlen)
        w2 = (b.maxlen + 31) // 32 if b.maxlen <= 512 else 0
        rd4, rd2, ns, bad = ref.rows_vec(b.bases, b.offs, b.lens, wpr, w2, chunk=500)          # (several chunks)
        assert np.array_equal(rd4, ref.rows4_plain(b, wpr))
        if w2:
            assert np.array_equal(rd2, ref.rows2_plain(b, w2))
        pns, pbad = ref.n_counts(b)
        assert np.array_equal(ns, pns) and np.array_equal(bad, pbad)
        for max_ns in ref.MAX_NS:
            assert np.array_equal(ref.refused_vec(b.lens, ns, bad, max_ns), ref.refused_plain(b, max_ns))
        assert np.array_equal(bad | (ns > 0), ref.has_n_plain(b))


def test_big_case_generator_and_vector_packer():
    """the inputs of the one large case, at a small size: lengths, the share of reads with an N, and pack_vec against the plain packer"""
    bases, offs, lens = ref.big_lens_bases(30000)
    assert lens.min() == 20 and lens.max() == 128 and len(np.unique(bases >> 3)) == 32
    b = ref.Batch([bases[int(o):int(o) + int(n)] for o, n in zip(offs, lens)])
    hasn = ref.has_n_plain(b)
    assert 200 <= hasn.sum() <= 400 and hasn[:2048].any()
    _, rd2, _, _ = ref.rows_vec(bases, offs, lens, ref.words_per_read(128), 4)
    words, woffs, exc = ref.pack_vec(bases, offs, lens, rd2[:, 0])
    pw, po, _, pe = ref.pack_plain(b)
    assert np.array_equal(words, pw) and np.array_equal(woffs, po) and np.array_equal(exc, pe)


def test_reference_packer_equals_bk_pack_reads():
    import biokanga_amd as bk
    assert bk.NBASE_DTYPE == ref.NBASE_DTYPE
    for b in _small_batches():
        words, woffs, lens16, exc = ref.pack_plain(b)
        w, l16, e = bk.pack_reads(b.bases, b.offs, b.lens)
        assert np.array_equal(words, w) and np.array_equal(lens16, l16) and np.array_equal(exc, e)
        assert np.array_equal(woffs[1:], np.cumsum((b.lens.astype(np.int64) + 15) // 16)[:-1].astype(np.uint64))
        assert ref.check_exc_ref(exc, b.lens) == 0
        # random fields under the exceptions change those fields and nothing else
        rw, _, _, re_ = ref.pack_plain(b, np.random.default_rng(3))
        assert np.array_equal(re_, exc) and not np.array_equal(rw, words)
        f0, f1 = ref.packed_fields(b, words, woffs), ref.packed_fields(b, rw, woffs)
        for c, x0, x1 in zip(b.codes(), f0, f1):
            assert all((a == c_ and b_ == c_) if c_ < 4 else a == 0 for c_, a, b_ in zip(c, x0, x1))


def test_check_exc_reference_counts_each_violation():
    lens = np.array([40, 40, 7], dtype=np.uint32)
    good = np.array([(0, 3, 4, 0), (0, 4, 4, 2), (0, 7, 5, 0), (0, 39, 4, 0), (1, 0, 4, 39), (2, 6, 7, 0)], dtype=ref.NBASE_DTYPE)
    assert ref.check_exc_ref(good, lens) == 0
    for k, change, bad in ((1, dict(code=3), 1), (1, dict(code=8), 1), (5, dict(read=3), 1), (3, dict(pos=38, run=2), 1), (2, dict(pos=4, run=0), 1),
                           (2, dict(pos=6), 1), (4, dict(read=0, pos=0, run=0), 1)):
        e = good.copy()
        for f, v in change.items():
            e[f][k] = v
        assert ref.check_exc_ref(e, lens) == bad, (k, change)


def test_compact_reference():
    cap = 4
    stage = [np.arange(ref.LIST_STRIPES * cap, dtype=np.uint32) + 1000 * li for li in range(2)]
    sizes = np.zeros((ref.LIST_STRIPES, 3), dtype=np.uint32)
    sizes[0] = (2, 0, 0)
    sizes[5] = (4, 1, 0)
    sizes[63] = (1, 3, 0)
    dense = [np.full(16, 9, dtype=np.uint32), np.full(16, 9, dtype=np.uint32)]
    d, t = ref.compact_ref(stage, cap, sizes, dense, [3, 0])
    assert t == [10, 4]
    assert d[0].tolist() == [9, 9, 9, 0, 1, 20, 21, 22, 23, 252] + [9] * 6
    assert d[1].tolist() == [1020, 1252, 1253, 1254] + [9] * 12


def test_n_decision_equals_the_oracle(tmp_path):
    """the same reads through the reference program's own scan: refused means nar == BK_NAR_NS there, at max_ns 0, 1 and 5"""
    n = index_ref.GENOME_SIZES[0]
    seq, sa = index_ref.tricky_genome(n), index_ref.genome_sa(n)
    ends = np.flatnonzero(seq == index_ref.EOS)
    assert len(ends) == 2
    path = str(tmp_path / "tricky.sfx")
    helpers.write_sfx(path, "tricky", [("s1", int(ends[0])), ("s2", int(ends[1] - ends[0] - 1))], seq, sa)
    o = helpers.OracleSfx(path)
    try:
        for b in (ref.fused_case(8).batch, ref.fused_case(16).batch, ref.unfused_case().batch):
            seen = set()
            for max_ns in ref.MAX_NS:
                hits, _ = o.align(b.bases, b.offs, b.lens, helpers.make_params(max_ns=max_ns))
                mine = ref.refused_plain(b, max_ns)
                assert np.array_equal(hits["nar"] == ref.NAR_NS, mine), np.flatnonzero((hits["nar"] == ref.NAR_NS) != mine)[:10]
                seen |= {(max_ns, bool(v)) for v in mine}
            assert len(seen) == 6                                        # both answers at every setting
    finally:
        o.close()
