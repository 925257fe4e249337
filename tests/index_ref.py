"""Plain references of the index image tables (biokanga_amd/csrc/bk_index.hip) and the genomes they are checked on: numpy over the
1 B/base sequence (A0 C1 G2 T3 N4, sequence end 7; the concatenation of the sequences, each followed by its end) and the suffix array,
base by base.  Nothing here reads a table the kernels made, and the suffix array is sorted here.  tests/test_index_ref_cpu.py checks
that the genomes hold every case the GPU tests (tests/test_gpu_index_tables.py) rely on."""
import functools

import numpy as np

U64 = np.uint64
EOS = 7
ABOVE = 0xFFFFFFFF
POISON8 = 0xA5
KEY_BASES = 15                 # kK2Bases
MAX_READ_LEN = 2000            # kMaxReadLenAbs


# ------------------------------------------------------------------------------------------------
# buffer sizes, as bk_image.cpp has them

def tgt4_words(n):
    return ((n + 15) // 16 + MAX_READ_LEN // 16 + 4 + 3) & ~3


def tgt2_words(n):
    return tgt4_words(n) // 4 * 2 + 8          # two words per 64-base block, 64 bytes of zeros behind them


def nflag_bytes(n, shift):
    nblocks = tgt4_words(n) // 4
    return ((((nblocks * 64) >> shift) + 1) + 31) // 32 * 4 + 16


def ktab_entries(k):
    return 4 ** k + 1


def starts_words(n):
    return (n >> 6) + 4


def brk_words(length):
    return (length >> 6) + 4


def ktab_hi_words(n_entries):
    return (n_entries >> 16) + 2


def swin_entries(n):
    return (n + 31) & ~31


def k2s_pad(w):
    return (w + 15) & ~15


def k2s_count(n, j):
    return (n + (1 << (4 * j)) - 1) >> (4 * j)


def key_words(n, levels):
    """k2s_start(n, levels + 1): the keys, their sampled levels and the padding between them"""
    o = k2s_pad(n) + 16
    for i in range(1, levels + 1):
        o += k2s_pad(k2s_count(n, i)) + 16
    return o


def poison(count, dtype):
    return np.frombuffer(bytes([POISON8]) * (count * np.dtype(dtype).itemsize), dtype=dtype).copy()


# ------------------------------------------------------------------------------------------------
# genome and suffix array

def _codes(s):
    return np.array(["ACGTN".index(c) for c in s], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def tricky_genome(n_total):
    """two sequences, n_total bases with their two ends.  The first holds every N: as its first base, as the last base before its end, lone
    ones, a run of 40 over a 16-base word and a 64-base block boundary, ACGN beside ACGT + 16 T, a 25-base context that ends in N
    twice, a poly-A run of 300 and a period-7 tandem repeat of 200.  The second, N-free and from base 1600 on in 512-base regions without
    N or sequence end, holds a 400-base segment three times and - near its start - a copy of its last 60 bases."""
    rng = np.random.default_rng(4177)
    R = lambda m: rng.integers(0, 4, m).astype(np.uint8)
    N = np.array([4], dtype=np.uint8)
    ctx = R(25)
    s1 = [N, R(120), _codes("ACGT" + "T" * 16), R(30), _codes("ACGN"), R(40), ctx, N, R(35), ctx, N, R(20)]
    at = sum(len(p) for p in s1)
    s1.append(R((50 - at) % 64))                               # the N run: bases 64 q + 50 .. 64 q + 89
    s1 += [np.full(40, 4, dtype=np.uint8), R(60), np.zeros(300, dtype=np.uint8), R(50) | np.uint8(1), np.tile(R(7), 30)[:200], R(30), N]
    s1 = np.concatenate(s1)
    assert s1[0] == 4 and s1[-1] == 4 and len(s1) < 1500
    tail = R(60)
    S = R(400)
    head = [R(20), tail, R(8)]
    head.append(R(1600 - (len(s1) + 1) - sum(len(p) for p in head)))
    body = [S, R(100), S, R(100), S]                           # 1600 .. 3000
    filler = n_total - 3000 - 60 - 1
    assert filler >= 40
    s2 = np.concatenate(head + body + [R(filler), tail])
    seq = np.concatenate([s1, [EOS], s2, [EOS]]).astype(np.uint8)
    assert len(seq) == n_total
    seq.setflags(write=False)
    return seq


GENOME_SIZES = (3200, 3201, 3215)          # n % 64 == 0 (and so n % 16 == 0), n % 16 == 1, n % 16 == 15

# what the GPU tests run with, and tests/test_index_ref_cpu.py checks the genomes for
KTAB_KS = (2, 4, 8, 11)                    # k-mer table orders
KEY_KS = (4, 11)                           # .. of the key arrays
K_DERIVED = 6                              # .. of the tables made from table and keys
K_BREAKS = 8                               # .. of the coverage rule, and its core lengths
LEVEL_SETS = ((K_BREAKS, (25, 33, 50, 100)), (K_BREAKS, (120,)), (K_BREAKS, (20, 25, 33, 40, 50, 66, 100, 120)), (12, (20, 25)))
FLAG_SHIFT = 9                             # N / sequence end flags per 512 bases, as a small index has them


def extended(seq, extra=MAX_READ_LEN + 128):
    """the sequence with sequence ends behind it, as the target's padding reads"""
    return np.concatenate([seq & 15, np.full(extra, EOS, dtype=np.uint8)])


def suffix_array(seq):
    """positions 0 .. n - 1 in the order of their suffixes: nibble order (a < c < g < t < N < sequence end), compared through the
    sequence ends, the concatenation followed by sequence ends"""
    n = len(seq)
    b = (np.asarray(seq) & 15).astype(np.uint8).tobytes()
    pad = bytes([EOS]) * n
    return np.array(sorted(range(n), key=lambda p: b[p:] + pad[:p]), dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def genome_sa(n_total):
    sa = suffix_array(tricky_genome(n_total))
    sa.setflags(write=False)
    return sa


# ------------------------------------------------------------------------------------------------
# target

def _or_reduce(v):
    return np.bitwise_or.reduce(v, axis=-1)


def pack4(b):
    """16 bases per word, base j of a word in nibble 15 - j"""
    v = np.asarray(b).astype(U64).reshape(-1, 16)
    return _or_reduce(v << (U64(60) - U64(4) * np.arange(16, dtype=U64)))


def pack2(b):
    """32 bases per word, base j of a word at bits 63 - 2j, 62 - 2j"""
    v = np.asarray(b).astype(U64).reshape(-1, 32)
    return _or_reduce(v << (U64(62) - U64(2) * np.arange(32, dtype=U64)))


def nibbles(seq):
    """the nibble of every base the 4 bit/base target holds: the sequence's, then sequence ends through the last padded word"""
    n = len(seq)
    out = np.full(tgt4_words(n) * 16, EOS, dtype=np.uint8)
    out[:n] = np.asarray(seq) & 15
    return out


def target4(seq):
    return pack4(nibbles(seq))


def target2(seq):
    """the 2 bit/base words and the eight zero words behind them"""
    return np.concatenate([pack2(nibbles(seq) & 3), np.zeros(8, dtype=U64)])


def nflag_bits(seq, shift):
    """per region of 2^shift bases: does it hold a nibble with bit 2 set (N, sequence end - the padding's among them)?"""
    nb = nibbles(seq)
    bad = (nb & 4) != 0
    g = np.arange(len(nb)) >> shift
    out = np.zeros(int(g[-1]) + 1, dtype=bool)
    np.logical_or.at(out, g, bad)
    return out


def bits_to_bytes(bits, nbytes):
    """bit g at bit g % 8 of byte g / 8"""
    out = np.zeros(nbytes * 8, dtype=np.uint8)
    out[:len(bits)] = bits
    return np.packbits(out, bitorder="little")


def bits_to_words(bits, nwords):
    return bits_to_bytes(bits, nwords * 8).view(U64)


def words_to_bits(words, count):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:count].astype(bool)


# ------------------------------------------------------------------------------------------------
# buckets, k-mer table

def bucket(seq, pos, k):
    """code of the first k bases of the suffixes at pos (first base the most significant), T from the first N / sequence end on"""
    ext = extended(seq)
    b = ext[np.asarray(pos, dtype=np.int64)[:, None] + np.arange(k)[None, :]]
    bad = np.logical_or.accumulate((b & 4) != 0, axis=1)
    d = np.where(bad, 3, b & 3).astype(np.int64)
    return (d * (4 ** np.arange(k - 1, -1, -1, dtype=np.int64))[None, :]).sum(axis=1)


def has_n_in_first(seq, pos, k):
    ext = extended(seq)
    b = ext[np.asarray(pos, dtype=np.int64)[:, None] + np.arange(k)[None, :]]
    return ((b & 4) != 0).any(axis=1)


def buckets_along(seq, sa, k):
    """bucket(i) for i = -1 .. n: -1, the buckets of the suffix array's elements, 4^k"""
    return np.concatenate([[-1], bucket(seq, sa, k), [4 ** k]])


def ktab(seq, sa, k):
    """entry c = the number of suffixes whose bucket is below c; entry 4^k = n"""
    cnt = np.bincount(bucket(seq, sa, k), minlength=4 ** k)
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)


def starts_bits(seq, sa, k):
    """bit i (0 .. n): bucket(i) != bucket(i - 1)"""
    b = buckets_along(seq, sa, k)
    return b[1:] != b[:-1]


# ------------------------------------------------------------------------------------------------
# keys

def key_digits(seq, pos, frm):
    """the 15 bases from pos + frm on: (digits [m, 15] - the bases in front of the first N / sequence end, 3 from it on; nkind [m])"""
    ext = extended(seq)
    b = ext[np.asarray(pos, dtype=np.int64)[:, None] + frm + np.arange(KEY_BASES)[None, :]]
    bad = np.logical_or.accumulate((b & 4) != 0, axis=1)
    return np.where(bad, 3, b & 3).astype(np.int64), bad[:, -1]


def _key_word(d, nkind):
    v = (d << (30 - 2 * np.arange(KEY_BASES, dtype=np.int64))[None, :]).sum(axis=1)
    return v | nkind.astype(np.int64)


def keys(seq, sa, k):
    """(k2, k3, k4) of every suffix array element: the 15 bases behind the first k, behind those and behind these; all ones where an N /
    sequence end lies inside the first k bases, and where the level before is not made of a, c, g, t alone"""
    out = []
    dead = has_n_in_first(seq, sa, k)
    for lvl in range(3):
        d, nk = key_digits(seq, sa, k + KEY_BASES * lvl)
        out.append(np.where(dead, ABOVE, _key_word(d, nk)).astype(np.uint32))
        dead = dead | nk
    return out


def check_counts(seq, sa, k, k2, k3=None, k4=None):
    """[bad0, bad1] of the pairs (i, i + 1), i = 0 .. n - 2 - bad0[i]: same bucket and k2[i] > k2[i + 1]; bad1[i]: same bucket, equal k2
    of a, c, g, t alone and the further levels (as far as given) out of order"""
    b = bucket(seq, sa, k)
    same = b[:-1] == b[1:]
    a2, c2 = k2[:-1].astype(np.int64), k2[1:].astype(np.int64)
    bad0 = same & (a2 > c2)
    bad1 = np.zeros(len(sa) - 1, dtype=bool)
    if k3 is not None:
        a3, c3 = k3[:-1].astype(np.int64), k3[1:].astype(np.int64)
        deeper = a3 > c3
        if k4 is not None:
            deeper |= (a3 == c3) & ((a3 & 3) == 0) & (k4[:-1].astype(np.int64) > k4[1:].astype(np.int64))
        bad1 = same & (a2 == c2) & ((a2 & 3) == 0) & deeper
    return bad0, bad1


def planted_places(seq, sa, k):
    """suffix array indexes i where swapping elements i and i + 1 puts: 'keys' two different second-level keys of one bucket out of
    order; 'deep' two third-level keys behind equal second-level keys of a, c, g, t; 'border' the last suffix of a bucket behind the
    first of the next"""
    b = bucket(seq, sa, k)
    k2, k3, _ = keys(seq, sa, k)
    same = b[:-1] == b[1:]
    out = {"keys": np.flatnonzero(same & (k2[:-1] != k2[1:])),
           "deep": np.flatnonzero(same & (k2[:-1] == k2[1:]) & ((k2[:-1] & 3) == 0) & (k3[:-1] != k3[1:])),
           "border": np.flatnonzero(~same)}
    return out


def swapped(sa, places):
    out = np.array(sa, dtype=np.uint32)
    for i in places:
        out[i], out[i + 1] = out[i + 1], out[i]
    return out


def pick_apart(cands, count, taken, gap=4):
    """up to `count` of cands, spread over them, every one `gap` or more indexes from the ones taken so far"""
    got = []
    for i in cands[np.linspace(0, len(cands) - 1, min(len(cands), 8 * count)).astype(int)]:
        if all(abs(int(i) - j) >= gap for j in taken + got):
            got.append(int(i))
        if len(got) == count:
            break
    return got


# ------------------------------------------------------------------------------------------------
# derived tables

def ktab2_y(tab, k2, max_bitmap, sa_elem=None):
    """the second word of every entry of a table of bucket starts: a lone suffix's key (or element), the map of the first five key bits
    of up to max_bitmap suffixes (all-ones keys set nothing), all ones for more; 0 for an empty bucket and for the last entry"""
    n_entries = len(tab)
    y = np.zeros(n_entries, dtype=np.uint32)
    for c in range(n_entries - 1):
        lo, hi = int(tab[c]), int(tab[c + 1])
        if hi == lo + 1:
            y[c] = sa_elem[lo] if sa_elem is not None else k2[lo]
        elif hi > lo + max_bitmap:
            y[c] = ABOVE
        else:
            v = 0
            for key in k2[lo:hi]:
                if int(key) != ABOVE:
                    v |= 1 << (int(key) // (1 << 27))
            y[c] = v
    return y


# ------------------------------------------------------------------------------------------------
# window array

def swin_entry_words(seq, sa, E, pre):
    """[n, 2 E] 64-bit words: entry i = the 64 E bases of the 2 bit/base target from sa[i] - pre on, 32 to a word, 0 in front of base 0"""
    two = nibbles(seq) & 3
    p = np.asarray(sa, dtype=np.int64)[:, None] - pre + np.arange(64 * E)[None, :]
    b = np.where(p >= 0, two[np.maximum(p, 0)], 0)
    return pack2(b.reshape(-1, 32)).reshape(len(sa), 2 * E)


def swin_word_index(idx, q, E):
    """where 16-byte word q of entry idx lies: the entries of a block of 32 word by word"""
    return (idx >> 5) * (32 * E) + q * 32 + (idx & 31)


def swin_scatter(out64, slots, words, E):
    """writes the entries `words` [m, 2 E] to the entry numbers `slots` of a window array viewed as 64-bit words"""
    for q in range(E):
        at = 2 * swin_word_index(np.asarray(slots, dtype=np.int64), q, E)
        out64[at] = words[:, 2 * q]
        out64[at + 1] = words[:, 2 * q + 1]


# ------------------------------------------------------------------------------------------------
# the coverage rule's breaks

def common_acgt(seq, p, q, limit):
    """bases of a, c, g, t the suffixes at p and q share, up to limit"""
    ext = extended(seq)
    m = 0
    while m < limit and ext[p + m] == ext[q + m] and ext[p + m] < 4:
        m += 1
    return m


def repeat_cut(seq, sa):
    """a suffix array index, a multiple of 64, between two suffixes that share 120 and more bases (copies of the repeated segment)"""
    for c in range(64, len(sa), 64):
        if min(sa[c - 1], sa[c]) >= 1600 and max(sa[c - 1], sa[c]) < 3000 and common_acgt(seq, int(sa[c - 1]), int(sa[c]), 120) >= 120:
            return c
    return None


def _known(digits):
    """bases of a key in front of its trailing t's"""
    real = KEY_BASES
    while real > 0 and digits[real - 1] == 3:
        real -= 1
    return real


def breaks_shared(seq, sa, k, w_max, shift, a, e):
    """for i = a .. e: (shared [e - a + 1], branch [e - a + 1]) - the bases suffixes i - 1 and i share as far as the rule looks, and the
    branch of the rule that said so: 'edge' (a, e), 'bucket', 'above' (an all-ones key), 'differ' (k + common key bases), 'nkind' (equal
    keys, an N or sequence end among their bases: k + 15) - both no further than the bases in front of the trailing t's of a key with an
    N or sequence end, which it holds as t like everything behind it, 'shallow' (no level beyond k + 15: no break), 'end' / 'flagged' (k + 15: a window runs to n / lies in a
    flagged region), 'deep1' / 'deep2' (k + 15 + the 2 bit/base compare, ended in its first 32-base step / later)"""
    n = len(sa)
    two = nibbles(seq) & 3
    flag = nflag_bits(seq, shift)
    st = starts_bits(seq, sa, k)
    dead = has_n_in_first(seq, sa, k)
    dig, nk = key_digits(seq, sa, k)
    deep_from = k + KEY_BASES
    span = w_max - deep_from
    shared = np.zeros(e - a + 1, dtype=np.int64)
    branch = []
    NONE = 1 << 20
    for i in range(a, e + 1):
        if i == a or i == e:
            s, br = 0, "edge"
        elif st[i]:
            s, br = 0, "bucket"
        elif dead[i - 1] or dead[i]:
            s, br = 0, "above"
        else:
            diff = np.flatnonzero(dig[i - 1] != dig[i])
            known = min(_known(dig[j]) if nk[j] else KEY_BASES for j in (i - 1, i))
            if len(diff):
                s, br = k + min(int(diff[0]), known), "differ"
            elif nk[i - 1] or nk[i]:
                s, br = k + known, "nkind"
            elif w_max <= deep_from:
                s, br = NONE, "shallow"
            else:
                pa, pb = int(sa[i - 1]) + deep_from, int(sa[i]) + deep_from
                s = deep_from
                if pa + span >= n or pb + span >= n:
                    br = "end"
                elif flag[pa >> shift] or flag[(pa + span - 1) >> shift] or flag[pb >> shift] or flag[(pb + span - 1) >> shift]:
                    br = "flagged"
                else:
                    br = "deep1"
                    for q in range(0, span, 32):
                        d = np.flatnonzero(two[pa + q:pa + q + 32] != two[pb + q:pb + q + 32])
                        if len(d):
                            s += int(d[0])
                            break
                        s += 32
                        br = "deep2"
        shared[i - a] = s
        branch.append(br)
    return shared, np.array(branch)


def breaks_bitmap(shared, w, n_words):
    """a level's bitmap: bit i - a = suffixes i - 1 and i share fewer than w bases; nothing behind bit e - a"""
    return bits_to_words(shared < w, n_words)


# ------------------------------------------------------------------------------------------------
# the coverage rule's blocks

def cover_flags(starts, length, max_run, min_run, head, blk_shift):
    """starts: ascending run starts inside [0, length), 0 among them; the last run ends at length.  A run of min_run .. max_run suffixes is
    covered whole, a longer one for its first `head` suffixes, a shorter one not at all; a block of 2^blk_shift indexes is covered when
    one of its suffixes is"""
    starts = np.asarray(starts, dtype=np.int64)
    lens = np.diff(np.concatenate([starts, [length]]))
    run_len = np.repeat(lens, lens)
    ofs = np.arange(length) - np.repeat(starts, lens)
    cov = ((run_len >= min_run) & (run_len <= max_run)) | ((run_len > max_run) & (ofs < head))
    n_blocks = (length + (1 << blk_shift) - 1) >> blk_shift
    padded = np.zeros(n_blocks << blk_shift, dtype=bool)
    padded[:length] = cov
    return padded.reshape(n_blocks, -1).any(axis=1)
