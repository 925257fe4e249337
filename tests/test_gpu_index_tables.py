"""GPU unit tests of the index set-up kernels (biokanga_amd/csrc/bk_index.hip), table by table, through their launchers under the
test-only entry points of tests/hip/indextest.hip.  The references are those of tests/index_ref.py - numpy over the 1 B/base sequence
and a suffix array sorted on the CPU, nothing a kernel made - and every comparison is exact.  Every buffer has the size bk_image.cpp
gives it and is filled with 0xA5 where a kernel is to write, so that an entry left out or written beside its place shows.  The tables a
kernel READS are the references'.  tests/test_index_ref_cpu.py checks that the genomes hold the cases named here.
Out of scope: suffix array elements of 2^32 and more (sa_get<true> with a non-zero fifth byte needs a target of 2 GB) - the paths for
5-byte elements run with zero fifth bytes, except in k_split_sa5's test; reading tables back out of a live context.
torch only carries the buffers to the device and back: every comparison is numpy's, on the host."""
import ctypes

import numpy as np
import pytest

import helpers
import index_ref as ref
from index_ref import FLAG_SHIFT, K_DERIVED, KEY_KS, KTAB_KS, LEVEL_SETS
from test_k2_levels_logic import K2_LEVELS, build_levels

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
INVALID = 1                       # hipErrorInvalidValue
P32, P64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


class Buf:
    """a device buffer holding a numpy array's bytes"""

    def __init__(self, a):
        import torch
        a = np.ascontiguousarray(a)
        assert a.size
        self.dtype, self.shape = a.dtype, a.shape
        self.t = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to("cuda")

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        return self.t.cpu().numpy().view(self.dtype).reshape(self.shape)


def ptr(b):
    return None if b is None else b.ptr


@pytest.fixture(scope="module")
def lib():
    import torch                  # (first: the library then shares the HIP runtime torch brings, and the tensors' pointers are its own)
    assert torch.cuda.is_available()
    lib = helpers.indextest_lib()
    assert lib.kK2Bases == ref.KEY_BASES and lib.kMaxReadLenAbs == ref.MAX_READ_LEN and lib.kK2Levels == K2_LEVELS
    assert lib.kSwBlkShift == 5 and lib.kSwLevels >= 8 and lib.kSwHead > 32 and lib.kSwMinRun > 32
    return lib


class Genome:
    def __init__(self, n):
        self.n = n
        self.seq = ref.tricky_genome(n)
        self.sa = ref.genome_sa(n)
        self.tgt4 = Buf(ref.target4(self.seq))
        self.tgt2 = Buf(ref.target2(self.seq))
        self.sa_lo = Buf(self.sa)
        self.sa_hi = Buf(np.zeros(n, dtype=np.uint8))
        self.t4w, self.t2w = ref.tgt4_words(n), ref.tgt2_words(n)


@pytest.fixture(scope="module")
def genomes():
    return {n: Genome(n) for n in ref.GENOME_SIZES}


def ok(rc):
    assert rc == 0, f"hipError_t {rc}"


# ------------------------------------------------------------------------------------------------
# (a) target

@pytest.mark.parametrize("n", ref.GENOME_SIZES)
def test_pack_target(lib, n):
    rng = np.random.default_rng(n)
    raw = ref.tricky_genome(n) | (rng.integers(0, 16, n).astype(np.uint8) << 4)          # the kernel keeps a byte's low nibble
    words = ref.tgt4_words(n)
    seq, out = Buf(raw), Buf(ref.poison(words, U64))
    ok(lib.bkit_pack_target(seq.ptr, n, out.ptr, words))
    exp = ref.target4(raw)
    assert len(exp) == words and (exp[(n + 15) // 16:] == 0x7777777777777777).all()
    assert np.array_equal(out.get(), exp)


@pytest.mark.parametrize("shift", [6, 9, 12])
@pytest.mark.parametrize("n", ref.GENOME_SIZES)
def test_pack_target2(lib, genomes, n, shift):
    g = genomes[n]
    nbytes = ref.nflag_bytes(n, shift)
    tgt2 = Buf(np.concatenate([ref.poison(g.t2w - 8, U64), np.zeros(8, dtype=U64)]))
    nflag = Buf(np.zeros(nbytes, dtype=np.uint8))
    ok(lib.bkit_pack_target2(g.tgt4.ptr, g.t4w, tgt2.ptr, g.t2w, nflag.ptr, nbytes, shift))
    assert np.array_equal(tgt2.get(), ref.target2(g.seq))                                 # (its zeroed tail among them)
    bits = ref.nflag_bits(g.seq, shift)
    assert bits.any() and (shift == 12 or not bits.all())
    assert np.array_equal(nflag.get(), ref.bits_to_bytes(bits, nbytes))                    # (no bit beyond the regions)


# ------------------------------------------------------------------------------------------------
# (b) 5-byte elements

@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_split_sa5(lib, n):
    rng = np.random.default_rng(n)
    el = rng.integers(0, 256, (n, 5)).astype(np.uint8)
    el[:, 4] = rng.integers(1, 256, n)
    sa5, lo, hi = Buf(el), Buf(ref.poison(n + 8, U32)), Buf(ref.poison(n + 8, np.uint8))
    ok(lib.bkit_split_sa5(sa5.ptr, n, lo.ptr, hi.ptr))
    e = el.astype(U32)
    assert np.array_equal(lo.get()[:n], e[:, 0] | e[:, 1] << 8 | e[:, 2] << 16 | e[:, 3] << 24)
    assert np.array_equal(hi.get()[:n], el[:, 4])
    assert (lo.get()[n:] == P32).all() and (hi.get()[n:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------
# (c) k-mer table

FORMS = {"u32": (U32, 1, 0, 0), "u64": (U64, 1, 1, 0), "pairs": (U32, 2, 0, 1)}          # dtype, words per entry, tab64, pairs


def _ktab_cuts(bk, n):
    """range ends: multiples of 64 and others, a range of one index, one in front of a stretch of empty buckets, a last range to n + 1"""
    gap = np.diff(bk[1:n + 1])                                    # gap[i - 1] = bucket(i) - bucket(i - 1)
    mid = 1100 + int(np.argmax(gap[1100:2000])) + 1
    return sorted({0, 64, 65, 333, mid, 2048, n - 1, n + 1}), mid


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k,n", list(zip(KTAB_KS, (3200, 3201, 3215, 3201))))
def test_build_ktab(lib, genomes, k, n, form):
    g = genomes[n]
    dtype, stride, tab64, pairs = FORMS[form]
    entries = ref.ktab_entries(k)
    whole = ref.ktab(g.seq, g.sa, k).astype(dtype)
    bk = ref.buckets_along(g.seq, g.sa, k)                         # bk[i + 1] = bucket(i), i = -1 .. n
    st_bits = ref.starts_bits(g.seq, g.sa, k)
    sw = ref.starts_words(n)
    poison_val = dtype(P64 if dtype == U64 else P32)

    def words(buf):
        """the table's first words, and its second words (pairs); compared on the host"""
        v = buf.get().reshape(entries, stride)
        return v[:, 0], (v[:, 1] if stride == 2 else None)

    cuts, mid = _ktab_cuts(bk, n)
    assert k < 8 or bk[mid + 1] - bk[mid] > 1                      # empty buckets between the two ranges' suffixes
    assert (k == 2 or st_bits[65:333].any()) and 333 % 64          # a start that a range from no multiple of 64 on leaves out
    for wide in (False, True):
        hi = g.sa_hi if wide else None
        # whole
        tab, starts = Buf(ref.poison(entries * stride, dtype)), Buf(np.zeros(sw, dtype=U64))
        ok(lib.bkit_build_ktab(g.tgt4.ptr, g.t4w, g.sa_lo.ptr, ptr(hi), n, tab.ptr, entries, k, tab64, pairs, 0, 0, starts.ptr, sw))
        first, second = words(tab)
        assert np.array_equal(first, whole), (k, form, wide)
        assert second is None or (second == P32).all()
        assert np.array_equal(starts.get(), ref.bits_to_words(st_bits, sw))
        # range by range: every range on a table of its own, the bitmap shared
        starts = Buf(np.zeros(sw, dtype=U64))
        exp_bits = np.zeros(n + 1, dtype=bool)
        union = np.zeros(entries, dtype=bool)
        for i0, i1 in zip(cuts[:-1], cuts[1:]):
            tab = Buf(ref.poison(entries * stride, dtype))
            ok(lib.bkit_build_ktab(g.tgt4.ptr, g.t4w, g.sa_lo.ptr, ptr(hi), n, tab.ptr, entries, k, tab64, pairs, i0, i1, starts.ptr, sw))
            lo, top = int(bk[i0]) + 1, int(bk[i1])                 # entries (bucket(i0 - 1), bucket(i1 - 1)]
            first, second = words(tab)
            assert np.array_equal(first[lo:top + 1], whole[lo:top + 1]), (k, form, wide, i0, i1)
            assert (first[:lo] == poison_val).all() and (first[top + 1:] == poison_val).all(), (k, form, wide, i0, i1)
            assert second is None or (second == P32).all()
            assert not union[lo:top + 1].any()
            union[lo:top + 1] = True
            if i0 % 64 == 0:
                exp_bits[i0:i1] = st_bits[i0:i1]
        assert union.all()
        assert exp_bits[2048:n - 1].any() and not exp_bits[65:333].any()
        assert np.array_equal(starts.get(), ref.bits_to_words(exp_bits, sw))


# ------------------------------------------------------------------------------------------------
# (d) keys

def _build_k2(lib, g, k, sa_lo, hi, k2, k3, k4, kw, bad, i0, i1, write_k2=1):
    ok(lib.bkit_build_k2(g.tgt4.ptr, g.t4w, sa_lo.ptr, ptr(hi), g.n, k, k2.ptr, ptr(k3), ptr(k4), kw, bad.ptr, i0, i1, write_k2))


def _keys_equal(buf, exp, upto, n):
    got = buf.get()
    assert np.array_equal(got[:upto], exp[:upto])
    assert (got[upto:] == P32).all()                               # later ranges' keys, the levels' room


@pytest.mark.parametrize("k,n", [(KEY_KS[0], 3201), (KEY_KS[0], 3215), (KEY_KS[1], 3200)])
def test_build_keys(lib, genomes, k, n):
    g = genomes[n]
    kw = ref.key_words(n, lib.kK2Levels)
    e2, e3, e4 = ref.keys(g.seq, g.sa, k)
    cuts = [0, 64, 65, 1000, 2048, n]
    fresh = lambda: Buf(ref.poison(kw, U32))
    for wide in (False, True):
        hi = g.sa_hi if wide else None
        for levels in (1, 2, 3):
            for ranges in ([0, 0], cuts):
                k2, k3, k4 = fresh(), fresh() if levels > 1 else None, fresh() if levels > 2 else None
                bad = Buf(np.zeros(2, dtype=U64))
                for i0, i1 in zip(ranges[:-1], ranges[1:]):
                    _build_k2(lib, g, k, g.sa_lo, hi, k2, k3, k4, kw, bad, i0, i1)
                    upto = i1 if i1 else n
                    for buf, exp in ((k2, e2), (k3, e3), (k4, e4)):
                        if buf is not None:
                            _keys_equal(buf, exp, upto, n)
                assert bad.get().tolist() == [0, 0]
        # the second-level keys in place and in use: the further levels behind them
        k2 = Buf(np.concatenate([e2, ref.poison(kw - n, U32)]))
        before = k2.get().copy()
        for ranges in ([0, 0], cuts):
            k3, k4, bad = fresh(), fresh(), Buf(np.zeros(2, dtype=U64))
            for i0, i1 in zip(ranges[:-1], ranges[1:]):
                _build_k2(lib, g, k, g.sa_lo, hi, k2, k3, k4, kw, bad, i0, i1, write_k2=0)
            assert np.array_equal(k2.get(), before)
            _keys_equal(k3, e3, n, n)
            _keys_equal(k4, e4, n, n)
            assert bad.get().tolist() == [0, 0]


@pytest.mark.parametrize("k,n", [(KEY_KS[0], 3201), (KEY_KS[1], 3200)])
def test_check_k2_counts_planted_swaps(lib, genomes, k, n):
    g = genomes[n]
    kw = ref.key_words(n, lib.kK2Levels)
    places = ref.planted_places(g.seq, g.sa, k)
    taken = []
    chosen = {}
    for cls in ("keys", "deep", "border"):
        chosen[cls] = ref.pick_apart(places[cls], 3, taken)
        assert chosen[cls]
        taken += chosen[cls]
    fresh = lambda: Buf(ref.poison(kw, U32))
    for name, plant in (("all", sorted(taken)), ("border", chosen["border"])):
        sa = ref.swapped(g.sa, plant)
        assert np.array_equal(np.sort(sa), np.arange(n))
        sa_lo = Buf(sa)
        e2, e3, e4 = ref.keys(g.seq, sa, k)
        # a range that begins between the two suffixes of a planted pair, for one place of every class
        cuts = sorted({0, n} | {i + 1 for i in (chosen["keys"][0], chosen["deep"][0], chosen["border"][0])})
        for levels in (1, 2, 3):
            b0, b1 = ref.check_counts(g.seq, sa, k, e2, e3 if levels > 1 else None, e4 if levels > 2 else None)
            exp = [int(b0.sum()), int(b1.sum())]
            if name == "border":
                assert exp == [0, 0]
            else:
                assert exp[0] >= len(chosen["keys"]) and (levels == 1 or exp[1] >= len(chosen["deep"]))
            for wide in (False, True):
                for ranges in ([0, 0], cuts):
                    k2, k3, k4 = fresh(), fresh() if levels > 1 else None, fresh() if levels > 2 else None
                    bad = Buf(np.zeros(2, dtype=U64))
                    for i0, i1 in zip(ranges[:-1], ranges[1:]):
                        _build_k2(lib, g, k, sa_lo, g.sa_hi if wide else None, k2, k3, k4, kw, bad, i0, i1)
                    assert bad.get().tolist() == exp, (name, levels, wide, ranges)
                    _keys_equal(k2, e2, n, n)
        assert np.array_equal(sa_lo.get(), sa)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 4097, 65537])
def test_build_k2_levels(lib, n):
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
    kw = ref.key_words(n, lib.kK2Levels)
    buf = Buf(np.concatenate([keys, ref.poison(kw - n, U32)]))
    ok(lib.bkit_build_k2_levels(buf.ptr, n, kw))
    exp = build_levels(keys)
    assert len(exp) == kw
    assert np.array_equal(buf.get().astype(np.uint64), exp)        # (every word that is no key or level entry: all ones)


# ------------------------------------------------------------------------------------------------
# (e) derived tables

def _ktab2_both(lib, tab, k2, n, sa_elem):
    entries = len(tab)
    d_tab, d_k2 = Buf(tab.astype(U32)), Buf(k2)
    d_sa = Buf(sa_elem) if sa_elem is not None else None
    out = Buf(ref.poison(entries * 2, U32).reshape(entries, 2))
    ok(lib.bkit_make_ktab2(d_tab.ptr, d_k2.ptr, entries, n, out.ptr, ptr(d_sa)))
    pairs = Buf(np.stack([tab.astype(U32), ref.poison(entries, U32)], axis=1))
    ok(lib.bkit_fill_ktab2_y(pairs.ptr, d_k2.ptr, entries, ptr(d_sa)))
    exp = np.stack([tab.astype(U32), ref.ktab2_y(tab, k2, lib.kTab2BitmapMax, sa_elem)], axis=1)
    assert np.array_equal(out.get(), exp)
    assert np.array_equal(pairs.get(), exp)
    none = Buf(np.stack([tab.astype(U32), ref.poison(entries, U32)], axis=1))
    ok(lib.bkit_fill_ktab2_y(none.ptr, None, entries, ptr(d_sa)))
    assert np.array_equal(none.get(), np.stack([tab.astype(U32), np.full(entries, ref.ABOVE, dtype=U32)], axis=1))
    return exp


@pytest.mark.parametrize("n", ref.GENOME_SIZES)
def test_ktab2_of_a_genome(lib, genomes, n):
    g = genomes[n]
    tab = ref.ktab(g.seq, g.sa, K_DERIVED)
    k2 = ref.keys(g.seq, g.sa, K_DERIVED)[0]
    by_key = _ktab2_both(lib, tab, k2, n, None)
    by_elem = _ktab2_both(lib, tab, k2, n, np.asarray(g.sa))
    lone = np.flatnonzero(np.diff(tab) == 1)
    assert len(lone) and not np.array_equal(by_key[lone, 1], by_elem[lone, 1])
    assert by_key[-1, 1] == 0 and by_key[-1, 0] == n


def test_ktab2_of_chosen_bucket_sizes(lib):
    rng = np.random.default_rng(65)
    big = lib.kTab2BitmapMax
    sizes = [0, 1, 2, big, big + 1, 1, 0, 0, 3, big - 1, big + 1, big, 2, 1, 5, 1] + rng.integers(0, 6, 200).tolist() + [big, 1]
    tab = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(tab[-1])
    k2 = ((rng.integers(0, 32, n).astype(np.uint64) << 27) | rng.integers(0, 1 << 27, n).astype(np.uint64)).astype(U32)
    k2[rng.random(n) < 0.1] = ref.ABOVE
    k2[tab[14]:tab[15]] = ref.ABOVE                                # a bucket of five all-ones keys: no bit
    k2[tab[15]] = ref.ABOVE                                        # a lone all-ones key: handed on as it is
    k2[tab[3]:tab[4]] = (np.arange(big) % 32).astype(U32) << 27    # 64 keys with every value of the five bits
    k2[tab[11]:tab[12]] = (np.arange(big) % 16).astype(U32) << 27  # .. and with half of them: the largest bucket that still has a map
    exp = _ktab2_both(lib, tab, k2, n, None)
    _ktab2_both(lib, tab, k2, n, rng.permutation(n).astype(U32))
    assert exp[14, 1] == 0 and exp[15, 1] == ref.ABOVE and exp[3, 1] == ref.ABOVE and exp[4, 1] == ref.ABOVE and exp[0, 1] == 0
    assert sizes[11] == big and exp[11, 1] == 0xFFFF
    assert exp[-1, 1] == 0


def test_pack_ktab64(lib):
    rng = np.random.default_rng(9)
    entries = ref.ktab_entries(9)
    hw = ref.ktab_hi_words(entries)
    tab = np.concatenate([[0], np.cumsum(rng.integers(0, 40000, entries - 1))]).astype(U64)
    assert int(tab[-1]) > 1 << 32
    groups = (entries - 1 >> 16) + 1
    assert all(int(tab[min(entries - 1, (q << 16) + 0xFFFF)]) - int(tab[q << 16]) < 1 << 32 for q in range(groups))

    def run(t):
        d_tab, off, hi, flag = Buf(t), Buf(ref.poison(entries, U32)), Buf(ref.poison(hw, U64)), Buf(np.zeros(1, dtype=U32))
        ok(lib.bkit_pack_ktab64(d_tab.ptr, entries, off.ptr, hi.ptr, hw, flag.ptr))
        return off.get(), hi.get(), int(flag.get()[0])

    off, hi, flag = run(tab)
    assert flag == 0
    assert np.array_equal(hi[np.arange(entries) >> 16] + off.astype(U64), tab)
    assert np.array_equal(hi[:groups], tab[::1 << 16]) and (hi[groups:] == P64).all()
    wide = tab.copy()
    wide[(1 << 16) + 5000:] += U64(1 << 32)                        # the second group now spans 2^32 and more
    off, hi, flag = run(wide)
    assert flag == 1


@pytest.mark.parametrize("n", ref.GENOME_SIZES)
def test_build_isa(lib, genomes, n):
    g = genomes[n]
    exp = np.empty(n, dtype=U32)
    exp[g.sa] = np.arange(n, dtype=U32)
    isa = Buf(ref.poison(n, U32))
    ok(lib.bkit_build_isa(g.sa_lo.ptr, n, isa.ptr, 0, 0))
    assert np.array_equal(isa.get(), exp)
    isa = Buf(ref.poison(n, U32))
    done = np.zeros(n, dtype=bool)
    for i0, i1 in zip([0, 64, 65, 1000, 2048], [64, 65, 1000, 2048, n]):
        ok(lib.bkit_build_isa(g.sa_lo.ptr, n, isa.ptr, i0, i1))
        done[g.sa[i0:i1]] = True
        assert np.array_equal(isa.get(), np.where(done, exp, P32))
    assert done.all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100003])
def test_count_nonzero(lib, n):
    rng = np.random.default_rng(n)
    flags = np.where(rng.random(n) < 0.4, rng.integers(1, 1 << 32, n, dtype=np.uint64), 0).astype(U32)
    flags[-1] = 7
    d_flags = Buf(np.concatenate([flags, ref.poison(64, U32)]))     # (what lies behind the n flags is not counted)
    count = Buf(np.array([1000], dtype=U64))
    ok(lib.bkit_count_nonzero(d_flags.ptr, n, count.ptr))
    assert int(count.get()[0]) == 1000 + int((flags != 0).sum())
    ok(lib.bkit_count_nonzero(d_flags.ptr, n, count.ptr))
    assert int(count.get()[0]) == 1000 + 2 * int((flags != 0).sum())


# ------------------------------------------------------------------------------------------------
# (f) window array entries

def _pre(lib, E):
    return lib.kSwPre3 if E == 3 else lib.kSwPre5


@pytest.mark.parametrize("E", [3, 5])
@pytest.mark.parametrize("n", ref.GENOME_SIZES)
def test_build_swin(lib, genomes, n, E):
    g = genomes[n]
    pre = _pre(lib, E)
    ents = ref.swin_entries(n)
    words = ref.swin_entry_words(g.seq, g.sa, E, pre)
    where = {int(p): int(np.flatnonzero(g.sa == p)[0]) for p in (0, 1, pre - 1, pre, pre + 1, pre - 32, n - 1)}
    assert (words[where[0], :pre // 32] == 0).all() and words[where[pre], 0] != 0          # bases in front of the target's start: 0
    exp = ref.poison(ents * E * 2, U64)
    ref.swin_scatter(exp, np.arange(n), words, E)
    for hi in (None, g.sa_hi):
        swin = Buf(ref.poison(ents * E * 2, U64))
        ok(lib.bkit_build_swin(g.tgt2.ptr, g.t2w, g.sa_lo.ptr, ptr(hi), n, swin.ptr, ents, E))
        got = swin.get()
        for p, i in where.items():
            for q in range(E):
                at = 2 * ref.swin_word_index(i, q, E)
                assert got[at:at + 2].tolist() == words[i, 2 * q:2 * q + 2].tolist(), (p, q)
        assert np.array_equal(got, exp)


@pytest.mark.parametrize("E", [3, 5])
def test_swin_fill_follows_the_map(lib, genomes, E):
    n = 3215
    g = genomes[n]
    words = ref.swin_entry_words(g.seq, g.sa, E, _pre(lib, E))
    n_blocks = (n + 31) >> 5
    none = 0xFFFFFFFF
    covered = np.flatnonzero(np.arange(n_blocks) % 3 != 2)
    assert covered[-1] == n_blocks - 1                             # the partial last block among them
    swin_blocks = len(covered) + 2
    m = np.full(n_blocks, none, dtype=U32)
    m[covered] = np.random.default_rng(E).permutation(swin_blocks)[:len(covered)]          # slot numbers in no order
    a, e = 40, n - 5
    i = np.arange(a, e)
    i = i[m[i >> 5] != none]
    exp = ref.poison(swin_blocks * 32 * E * 2, U64)
    ref.swin_scatter(exp, (m[i >> 5].astype(np.int64) << 5) + (i & 31), words[i], E)
    d_map, swin = Buf(m), Buf(ref.poison(swin_blocks * 32 * E * 2, U64))
    ok(lib.bkit_swin_fill(g.tgt2.ptr, g.t2w, g.sa_lo.ptr, None, n, d_map.ptr, n_blocks, swin.ptr, swin_blocks, E, a, e))
    assert np.array_equal(swin.get(), exp)
    # in two ranges, 5-byte elements
    swin = Buf(ref.poison(swin_blocks * 32 * E * 2, U64))
    for i0, i1 in ((a, 1001), (1001, e)):
        ok(lib.bkit_swin_fill(g.tgt2.ptr, g.t2w, g.sa_lo.ptr, g.sa_hi.ptr, n, d_map.ptr, n_blocks, swin.ptr, swin_blocks, E, i0, i1))
    assert np.array_equal(swin.get(), exp)


def test_swin_map_and_advance(lib):
    rng = np.random.default_rng(3)
    none = 0xFFFFFFFF
    used0, cap = 3, 300
    used = Buf(np.array([used0], dtype=U32))
    u = used0
    for n_blocks in (517, 400):                                    # the second range runs into the cap
        flags = (rng.random(n_blocks) < 0.5).astype(U32) * rng.integers(1, 9, n_blocks).astype(U32)
        incl = np.cumsum(flags != 0).astype(U32)
        d_map = Buf(ref.poison(n_blocks + 4, U32))
        d_flags, d_incl = Buf(flags), Buf(incl)
        ok(lib.bkit_swin_map(d_flags.ptr, d_incl.ptr, n_blocks, cap, used.ptr, d_map.ptr))
        slot = u + incl.astype(np.int64) - 1
        exp = np.where((flags != 0) & (slot < cap), slot, none).astype(U32)
        got = d_map.get()
        assert np.array_equal(got[:n_blocks], exp) and (got[n_blocks:] == P32).all()
        assert (exp != none).any()
        u = min(u + int(incl[-1]), cap)
        assert int(used.get()[0]) == u
    assert u == cap and (exp == none).sum() > (flags == 0).sum()


# ------------------------------------------------------------------------------------------------
# (g) coverage rule

def _breaks(lib, g, k, levels, k2, tab, nflag, nbytes, a, e, starts, hi=None):
    length = e - a
    bw, n_words = ref.brk_words(length), (length >> 6) + 2
    brk = Buf(ref.poison(len(levels) * bw, U64).reshape(len(levels), bw))
    w = (ctypes.c_int * len(levels))(*levels)
    ok(lib.bkit_swin_breaks(g.tgt4.ptr, g.tgt2.ptr, g.t2w, nflag.ptr, nbytes, FLAG_SHIFT, g.sa_lo.ptr, ptr(hi), k2.ptr, tab.ptr, g.n, k, w, len(levels),
                            brk.ptr, bw, a, e, n_words, ptr(starts), ref.starts_words(g.n)))
    return brk.get(), n_words


@pytest.mark.parametrize("k,levels", LEVEL_SETS)
@pytest.mark.parametrize("n", ref.GENOME_SIZES)
def test_swin_breaks(lib, genomes, n, k, levels):
    g = genomes[n]
    nbytes = ref.nflag_bytes(n, FLAG_SHIFT)
    nflag = Buf(ref.bits_to_bytes(ref.nflag_bits(g.seq, FLAG_SHIFT), nbytes))
    k2 = Buf(ref.keys(g.seq, g.sa, k)[0])
    tab = Buf(ref.ktab(g.seq, g.sa, k).astype(U32))
    starts = Buf(ref.bits_to_words(ref.starts_bits(g.seq, g.sa, k), ref.starts_words(n)))
    cut = ref.repeat_cut(g.seq, g.sa)
    for a, e in ((0, n), (0, cut), (cut, n)):
        shared, _ = ref.breaks_shared(g.seq, g.sa, k, levels[-1], FLAG_SHIFT, a, e)
        with_starts, n_words = _breaks(lib, g, k, levels, k2, tab, nflag, nbytes, a, e, starts)
        without, _ = _breaks(lib, g, k, levels, k2, tab, nflag, nbytes, a, e, None, g.sa_hi)
        assert np.array_equal(with_starts, without)
        for l, w in enumerate(levels):
            assert np.array_equal(with_starts[l, :n_words], ref.breaks_bitmap(shared, w, n_words)), (a, e, w)
            assert (with_starts[l, n_words:] == P64).all()
            # soundness against the sequences themselves: a clear bit = that many bases of a, c, g, t shared
            bits = ref.words_to_bits(with_starts[l, :n_words], e - a + 1)
            assert bits[0] and bits[e - a]
            for j in np.flatnonzero(~bits):
                i = a + int(j)
                assert ref.common_acgt(g.seq, int(g.sa[i - 1]), int(g.sa[i]), w) >= w, (a, e, w, i)


def _planted_runs(max_run):
    """break positions: runs of every length named, each starting at every phase of a block of 32 (runs of 1 .. 31 between them set the phase)"""
    lengths = [1, 31, 32, 33, 64, 65, 66, 191, 192, 193, max_run - 1, max_run, max_run + 1, max_run + 500]
    starts, at = [], 0
    for phase in range(32):
        for L in lengths:
            fill = (phase - at) % 32
            if fill:
                starts.append(at)
                at += fill
            assert at % 32 == phase
            starts.append(at)
            at += L
    return np.array(starts, dtype=np.int64), at


@pytest.mark.parametrize("min_run", [65, 96, 256])
@pytest.mark.parametrize("max_run", [257, 1256])
def test_swin_cover(lib, max_run, min_run):
    assert max_run > lib.kSwHead and min_run >= lib.kSwMinRun
    starts, length = _planted_runs(max_run)
    bits = np.zeros(length + 1, dtype=bool)
    bits[starts] = True
    bits[length] = True                                            # the range's end closes the last run
    bw = ref.brk_words(length)
    brk = Buf(ref.bits_to_words(bits, bw))
    n_blocks = (length + 31) >> 5
    exp = ref.cover_flags(starts, length, max_run, min_run, lib.kSwHead, lib.kSwBlkShift)
    assert exp.any() and not exp.all()
    flags = Buf(ref.poison(n_blocks + 4, U32))
    ok(lib.bkit_swin_cover(brk.ptr, bw, length, max_run, min_run, flags.ptr, n_blocks, 1))
    got = flags.get()
    assert np.array_equal(got[:n_blocks], exp.astype(U32)), np.flatnonzero(got[:n_blocks] != exp)[:10]
    assert (got[n_blocks:] == P32).all()
    # a later level: its blocks are added to the earlier level's
    earlier = (np.random.default_rng(max_run + min_run).random(n_blocks) < 0.3).astype(U32)
    flags = Buf(earlier)
    ok(lib.bkit_swin_cover(brk.ptr, bw, length, max_run, min_run, flags.ptr, n_blocks, 0))
    assert np.array_equal(flags.get() != 0, (earlier != 0) | exp)


# ------------------------------------------------------------------------------------------------
# the entry points refuse what would leave a buffer

def test_entry_points_refuse_bad_arguments(lib, genomes):
    g = genomes[3200]
    n = g.n
    scratch = Buf(ref.poison(1 << 16, U64))
    p = scratch.ptr
    assert lib.bkit_pack_target(p, 0, p, 8) == INVALID and lib.bkit_pack_target(p, 200, p, 12) == INVALID
    assert lib.bkit_pack_target2(g.tgt4.ptr, g.t4w, p, g.t2w, p, 64, 5) == INVALID
    assert lib.bkit_pack_target2(g.tgt4.ptr, g.t4w, p, g.t4w // 2 - 1, p, 64, 9) == INVALID
    assert lib.bkit_pack_target2(g.tgt4.ptr, g.t4w, p, g.t2w, p, 8, 6) == INVALID
    assert lib.bkit_split_sa5(p, 0, p, p) == INVALID
    for k in (1, 17):
        assert lib.bkit_build_ktab(g.tgt4.ptr, g.t4w, g.sa_lo.ptr, None, n, p, 1 << 16, k, 0, 0, 0, 0, None, 0) == INVALID
        assert lib.bkit_build_k2(g.tgt4.ptr, g.t4w, g.sa_lo.ptr, None, n, k, p, None, None, 1 << 16, p, 0, 0, 1) == INVALID
    assert lib.bkit_build_ktab(g.tgt4.ptr, g.t4w, g.sa_lo.ptr, None, n, p, 4 ** 4, 4, 0, 0, 0, 0, None, 0) == INVALID
    assert lib.bkit_build_ktab(g.tgt4.ptr, g.t4w, g.sa_lo.ptr, None, n, p, 4 ** 4 + 1, 4, 0, 0, 0, n + 2, None, 0) == INVALID
    assert lib.bkit_build_ktab(g.tgt4.ptr, g.t4w, g.sa_lo.ptr, None, 0, p, 4 ** 4 + 1, 4, 0, 0, 0, 0, None, 0) == INVALID
    assert lib.bkit_build_k2(g.tgt4.ptr, g.t4w, g.sa_lo.ptr, None, n, 4, p, None, None, n - 1, p, 0, 0, 1) == INVALID
    assert lib.bkit_build_k2_levels(p, 100, ref.key_words(100, lib.kK2Levels) - 1) == INVALID and lib.bkit_build_k2_levels(p, 0, 1 << 16) == INVALID
    assert lib.bkit_build_isa(g.sa_lo.ptr, n, p, 0, n + 1) == INVALID and lib.bkit_count_nonzero(p, 0, p) == INVALID
    assert lib.bkit_build_swin(g.tgt2.ptr, g.t2w, g.sa_lo.ptr, None, n, p, n - 32, 3) == INVALID
    assert lib.bkit_build_swin(g.tgt2.ptr, g.t2w, g.sa_lo.ptr, None, n, p, n, 4) == INVALID
    assert lib.bkit_pack_ktab64(p, (1 << 16) + 1, p, p, 1, p) == INVALID
    assert (scratch.get() == P64).all()
