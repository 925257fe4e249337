"""The genomes and references of tests/index_ref.py hold what tests/test_gpu_index_tables.py relies on: no GPU test there passes because
a case it names does not occur.  CPU only."""
import numpy as np
import pytest

import index_ref as ref

from index_ref import FLAG_SHIFT, K_BREAKS, K_DERIVED, KEY_KS, KTAB_KS, LEVEL_SETS

ALL_KS = sorted(set(KTAB_KS + KEY_KS + (K_DERIVED, K_BREAKS, 12)))


def _find(hay, needle):
    hay, needle = bytes(hay), bytes(needle)
    out, at = [], hay.find(needle)
    while at >= 0:
        out.append(at)
        at = hay.find(needle, at + 1)
    return out


@pytest.mark.parametrize("n", ref.GENOME_SIZES)
def test_the_genome_holds_what_it_promises(n):
    seq = ref.tricky_genome(n)
    assert len(seq) == n and 3000 <= n <= 6000
    assert {3200: n % 64 == 0 and n % 16 == 0, 3201: n % 16 == 1, 3215: n % 16 == 15}[n]
    ends = np.flatnonzero(seq == ref.EOS)
    assert len(ends) == 2 and ends[1] == n - 1
    assert seq[0] == 4 and seq[ends[0] - 1] == 4                                   # N first, N last before a sequence end
    isn = seq == 4
    lone = isn & ~np.roll(isn, 1) & ~np.roll(isn, -1)
    assert lone[1:-1].any()
    run = _find(isn.astype(np.uint8), np.ones(40, dtype=np.uint8))
    assert any(p // 16 != (p + 39) // 16 and p // 64 != (p + 39) // 64 and not isn[p - 1] and not isn[p + 40] for p in run)
    assert _find(seq, ref._codes("ACGT" + "T" * 16)) and _find(seq, ref._codes("ACGN"))
    assert _find(seq, np.zeros(300, dtype=np.uint8))
    tandem = [p for p in range(n - 200) if np.array_equal(seq[p:p + 193], seq[p + 7:p + 200]) and len(set(seq[p:p + 7].tolist())) > 1]
    assert tandem
    assert any(len(_find(seq, seq[p:p + 400])) >= 3 and seq[p:p + 400].max() < 4 for p in (1600,))
    assert len(_find(seq, seq[n - 61:n - 1])) == 2


@pytest.mark.parametrize("n", ref.GENOME_SIZES)
def test_the_suffix_array_is_a_sorted_permutation(n):
    seq, sa = ref.tricky_genome(n), ref.genome_sa(n)
    assert np.array_equal(np.sort(sa), np.arange(n))
    ext = ref.extended(seq, n + 8).astype(np.int64)
    for i in range(n - 1):
        p, q = int(sa[i]), int(sa[i + 1])
        d = np.flatnonzero(ext[p:p + n + 1] != ext[q:q + n + 1])
        assert len(d) and ext[p + d[0]] < ext[q + d[0]], i


@pytest.mark.parametrize("n", ref.GENOME_SIZES)
def test_buckets_follow_the_suffix_array(n):
    seq, sa = ref.tricky_genome(n), ref.genome_sa(n)
    for k in ALL_KS:
        b = ref.bucket(seq, sa, k)
        assert (np.diff(b) >= 0).all() and 0 <= b.min() and b.max() < 4 ** k, k
        tab = ref.ktab(seq, sa, k)
        assert tab[0] == 0 and tab[-1] == n and len(tab) == ref.ktab_entries(k)
        # a suffix with an N / sequence end inside its first k bases, in a bucket that a suffix whose k bases are real shares with it
        padded = ref.has_n_in_first(seq, sa, k)
        assert padded.any() and (~padded).any()
        assert np.intersect1d(b[padded], b[~padded]).size, k
        st = ref.starts_bits(seq, sa, k)
        assert st[0] and st[n] and int(st[:n].sum()) == len(np.unique(b))
    # the empty stretches the k = 11 fills run over, and every size class of (e)
    size = np.diff(ref.ktab(seq, sa, K_DERIVED))
    assert (size == 0).any() and (size == 1).any() and ((size >= 2) & (size <= 64)).any() and (size >= 65).any()
    assert (np.diff(ref.ktab(seq, sa, 11)) == 0).mean() > 0.99


@pytest.mark.parametrize("n", ref.GENOME_SIZES)
def test_the_keys_are_in_order_and_every_planted_class_has_a_place(n):
    seq, sa = ref.tricky_genome(n), ref.genome_sa(n)
    for k in KEY_KS:
        k2, k3, k4 = ref.keys(seq, sa, k)
        bad0, bad1 = ref.check_counts(seq, sa, k, k2, k3, k4)
        assert not bad0.any() and not bad1.any()
        assert (k2 == ref.ABOVE).any() and ((k2 & 3) == 1).any() and ((k2 & 3) == 0).any()
        assert ((k3 != ref.ABOVE) & ((k3 & 3) == 1)).any() and ((k4 != ref.ABOVE) & ((k4 & 3) == 1)).any()
        assert (k4 != ref.ABOVE).any() and ((k3 == ref.ABOVE) & (k2 != ref.ABOVE)).any()
        places = ref.planted_places(seq, sa, k)
        for cls in ("keys", "deep", "border"):
            assert len(places[cls]), (k, cls)
        # what a swap at each class's place does, by the rule
        i = int(places["keys"][0])
        s = ref.swapped(sa, [i])
        b0, b1 = ref.check_counts(seq, s, k, *ref.keys(seq, s, k))
        assert b0[i] and not b1[i]
        i = int(places["deep"][0])
        s = ref.swapped(sa, [i])
        b0, b1 = ref.check_counts(seq, s, k, *ref.keys(seq, s, k))
        assert b1[i] and not b0[i]
        s = ref.swapped(sa, ref.pick_apart(places["border"], 5, []))
        b0, b1 = ref.check_counts(seq, s, k, *ref.keys(seq, s, k))
        assert not b0.any() and not b1.any()


@pytest.mark.parametrize("n", ref.GENOME_SIZES)
def test_every_branch_of_the_breaks_rule_decides_a_pair(n):
    seq, sa = ref.tricky_genome(n), ref.genome_sa(n)
    seen = set()
    for k, levels in LEVEL_SETS:
        shared, branch = ref.breaks_shared(seq, sa, k, levels[-1], FLAG_SHIFT, 0, n)
        for br in np.unique(branch):
            at = branch == br
            # "decides": the bit the branch sets is set at one level or clear at one
            seen.add((br, bool((shared[at][:, None] < np.array(levels)[None, :]).any()), bool((shared[at][:, None] >= np.array(levels)[None, :]).any())))
        if levels[-1] > k + ref.KEY_BASES + 32:
            deep2 = shared[branch == "deep2"]
            assert ((deep2 >= k + ref.KEY_BASES + 32) & (deep2 < levels[-1])).any()          # a difference found in a later 32-base step
            assert (deep2 >= levels[-1]).any()                                                 # .. and none found at all
        # soundness: a clear bit means that many bases of a, c, g, t really shared
        for w in levels:
            for j in np.flatnonzero(shared >= w):
                i = int(j)
                assert 0 < i < n and ref.common_acgt(seq, int(sa[i - 1]), int(sa[i]), w) >= w, (k, w, i, branch[i])
    # a range boundary inside the repeated segment's suffixes
    cut = ref.repeat_cut(seq, sa)
    assert cut is not None and cut % 64 == 0 and 0 < cut < n
    p, q = int(sa[cut - 1]), int(sa[cut])
    assert 1600 <= p < 3000 and 1600 <= q < 3000
    names = {s[0] for s in seen}
    assert names == {"edge", "bucket", "above", "differ", "nkind", "shallow", "end", "flagged", "deep1", "deep2"}
    for br in ("differ", "deep1", "deep2"):
        assert (br, True, True) in seen, br                     # breaks at one level, none at another
    for br in ("nkind", "end", "flagged"):
        assert (br, True, False) in seen or (br, True, True) in seen, br


def test_the_cover_rule_on_a_hand_made_bitmap():
    # runs: 10 (short), 70 (whole), 300 (long: its first 192), 40 (short); blocks of 32, min 65, max 257
    got = ref.cover_flags([0, 10, 80, 380], 420, 257, 65, 192, 5)
    exp = np.zeros(14, dtype=bool)
    exp[0:3] = True                   # 10 .. 79 lies in blocks 0 .. 2
    exp[2:9] = True                   # 80 .. 271 in blocks 2 .. 8
    assert np.array_equal(got, exp)


def test_the_sizes_follow_the_image():
    assert ref.tgt4_words(3200) == 332 and ref.tgt2_words(3200) == 174 and ref.nflag_bytes(3200, 9) == 20
    assert ref.key_words(1, 7) == 8 * 32 and ref.swin_entries(33) == 64 and ref.ktab_hi_words(4 ** 9 + 1) == 6
