"""GPU unit tests of the register window compares (biokanga_amd/csrc/bk_dev_window.h): eval_window2i<8|16, false|true>,
eval_window_rare<8|16> and window_to_iwindow under the test-only kernels of tests/hip/devtest.hip, one candidate per lane.
The reference is a loop over the bases in numpy: base j < len of a window mismatches if the read base is N or differs from
target[t + j]; mm is the number of such bases, im their map in the laid-together layout of IWindow, eos "an EOS lies in the
window".  The targets are packed here as the index image holds them (tgt4: 16 bases per word, first base in the top nibble,
A0 C1 G2 T3 N4 EOS7; tgt2: 32 bases per word, first base in the top bits, followed by 64 bytes of padding; tgt2s: tgt2 again
from its fifth word on); every padding word, and every bit of a read row behind the read's last base, is filled with rubbish."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

U64 = np.uint64


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.itemsize])).to("cuda")


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _or_reduce(v):
    return np.bitwise_or.reduce(v, axis=-1)


def pack2(b):
    """bases (their low two bits) -> 2 bit/base words, base j of a word at bits 63 - 2j, 62 - 2j"""
    v = (np.asarray(b).astype(U64) & U64(3)).reshape(-1, 32)
    return _or_reduce(v << (U64(62) - U64(2) * np.arange(32, dtype=U64)))


def pack4(b):
    """bases -> 4 bit/base words, base j of a word in nibble 15 - j"""
    v = (np.asarray(b).astype(U64) & U64(15)).reshape(-1, 16)
    return _or_reduce(v << (U64(60) - U64(4) * np.arange(16, dtype=U64)))


def imap(bits):
    """bool [n, 64 W] -> the laid-together map [n, W]: base 64i + j (j < 32) at bit 62 - 2j of word i, base 64i + 32 + j at bit 63 - 2j"""
    n = bits.shape[0]
    v = bits.reshape(n, -1, 2, 32).astype(U64)
    sh = U64(62) - U64(2) * np.arange(32, dtype=U64)
    return _or_reduce(v[:, :, 0, :] << sh) | _or_reduce(v[:, :, 1, :] << (sh + U64(1)))


def bitmap(bits):
    """bool [n, 64 W] -> Window::bm [n, W]: base b at bit b % 64 of word b / 64"""
    n = bits.shape[0]
    return _or_reduce(bits.reshape(n, -1, 64).astype(U64) << np.arange(64, dtype=U64))


LENS = {8: (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128), 16: (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256)}


def make_cases(nw, ts, tgt_at, rng, with_n=True, end=None):
    """every t of ts x every length x {no substitution, one at base 0, one at base len - 1, many (bases 0 and len - 1 among them), an N
    and a substitution} -> T [n], L [n], R [n, 16 nw] (read bases 0..3, N = 4; behind the read's end: rubbish).  With end: for every
    length the last window that fits in front of base `end` instead"""
    W = 16 * nw
    tt, ll, vv = np.meshgrid(np.asarray(ts, dtype=np.int64), np.array(LENS[nw], dtype=np.int64), np.arange(5 if with_n else 4), indexing="ij")
    T, L, V = tt.ravel(), ll.ravel(), vv.ravel()
    if end is not None:
        T = end - L
    n = len(T)
    j = np.arange(W, dtype=np.int64)[None, :]
    inside = j < L[:, None]
    R = tgt_at(np.where(inside, T[:, None] + j, T[:, None])).astype(np.uint8)
    assert int(R.max()) < 4
    sub = np.zeros((n, W), dtype=bool)
    sub[V == 1, 0] = True
    last = (np.arange(n), L - 1)
    sub[last] |= V == 2
    many = (rng.random((n, W)) < 0.3) & (V == 3)[:, None]
    many[:, 0] |= V == 3
    many[last] |= V == 3
    sub |= many
    npos = rng.integers(0, 1 << 30, n) % L
    spos = rng.integers(0, 1 << 30, n) % L
    sub[np.arange(n), spos] |= V == 4
    R = np.where(sub, (R + 1 + rng.integers(0, 3, (n, W))) & 3, R).astype(np.uint8)
    R[np.arange(n)[V == 4], npos[V == 4]] = 4
    R = np.where(inside, R, rng.integers(0, 4, (n, W))).astype(np.uint8)
    return T.astype(U64), L.astype(np.int32), R


def reference(T, L, R, tgt_at, n_always_differs=True):
    """the per-base loop: (mismatch bit per base [n, W], mm, eos)"""
    n, W = R.shape
    mis = np.zeros((n, W), dtype=bool)
    eos = np.zeros(n, dtype=bool)
    for j in range(W):
        live = j < L
        tb = tgt_at(np.where(live, T.astype(np.int64) + j, T.astype(np.int64)))
        differs = (R[:, j] != tb) | ((R[:, j] == 4) if n_always_differs else False)
        mis[:, j] = live & differs
        eos |= live & (tb == 7)
    return mis, mis.sum(axis=1).astype(np.int32), eos


def run_window2i(nw, wide, T, L, R, tgt):
    """tgt: (d_tgt2, d_tgt2s or None, n_bases).  -> im [n, nw / 4], mm, eos"""
    import torch
    lib = helpers.devtest_lib()
    d_tgt2, d_tgt2s, n_bases = tgt
    n, W = R.shape
    assert W == 16 * nw and int((T + L.astype(U64)).max()) <= n_bases and int(L.min()) >= 1 and int(L.max()) <= W
    assert d_tgt2.numel() == 2 * ((n_bases + 63) // 64) + 8 and (d_tgt2s is None or d_tgt2s.numel() == d_tgt2.numel())
    assert wide or int(T.max()) < (1 << 32)
    inside = np.arange(W)[None, :] < L[:, None]
    r2w = pack2(np.where(R == 4, 0, R).ravel()).reshape(n, nw // 2)               # (N held as A)
    rni = imap((R == 4) & inside)                                                # "this read base is N", zero behind the read
    d_r2w, d_rni, d_len, d_t = _dev(r2w), _dev(rni), _dev(L), _dev(T)
    d_im = torch.zeros(n * (nw // 4), dtype=torch.int64, device="cuda")
    d_mm = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_eos = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rc = lib.bkdt_window2i(nw, 1 if wide else 0, d_r2w.data_ptr(), d_rni.data_ptr(), d_len.data_ptr(), d_t.data_ptr(), d_tgt2.data_ptr(),
                           d_tgt2s.data_ptr() if d_tgt2s is not None else None, n, d_im.data_ptr(), d_mm.data_ptr(), d_eos.data_ptr())
    assert rc == 0, f"hipError_t {rc}"
    return _host(d_im, U64).reshape(n, nw // 4), _host(d_mm, np.int32), _host(d_eos, np.uint8) != 0


def run_window_rare(nw, four, T, L, R, d_tgt4, n_bases):
    """-> bm, im (window_to_iwindow of the result) [n, nw / 4], mm, eos"""
    import torch
    lib = helpers.devtest_lib()
    n, W = R.shape
    assert W == 16 * nw and int((T + L.astype(U64)).max()) <= n_bases and int(L.min()) >= 1 and int(L.max()) <= W
    assert d_tgt4.numel() >= (n_bases + 15) // 16 + 2                            # nib16 always loads the word behind
    if four:
        rows, row_words = pack4(R.ravel()).reshape(n, nw), nw
    else:
        assert int(R.max()) < 4
        rows, row_words = pack2(R.ravel()).reshape(n, nw // 2), nw // 2
    d_rows, d_len, d_t = _dev(rows), _dev(L), _dev(T)
    d_bm = torch.zeros(n * (nw // 4), dtype=torch.int64, device="cuda")
    d_im = torch.zeros(n * (nw // 4), dtype=torch.int64, device="cuda")
    d_mm = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_eos = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rc = lib.bkdt_window_rare(nw, d_rows.data_ptr(), row_words, 1 if four else 0, d_len.data_ptr(), d_t.data_ptr(), d_tgt4.data_ptr(), n,
                              d_bm.data_ptr(), d_im.data_ptr(), d_mm.data_ptr(), d_eos.data_ptr())
    assert rc == 0, f"hipError_t {rc}"
    return _host(d_bm, U64).reshape(n, nw // 4), _host(d_im, U64).reshape(n, nw // 4), _host(d_mm, np.int32), _host(d_eos, np.uint8) != 0


def _compare(what, T, L, got, want):
    im, mm, eos = got
    mis, wmm, weos = want
    wim = imap(mis)
    bad = np.nonzero((im != wim).any(axis=1) | (mm != wmm) | (eos != weos))[0]
    assert len(bad) == 0, (what, len(bad), [(int(T[i]), int(L[i]), int(mm[i]), int(wmm[i]), [hex(int(x)) for x in im[i]], [hex(int(x)) for x in wim[i]]) for i in bad[:4]])


def make_tgt2(n_bases, regions, rng):
    """device arrays (tgt2, tgt2s) of 2 * ceil(n_bases / 64) + 8 words, zero but for regions [(first base, bases)] (starts and lengths
    multiples of 32).  tgt2s[j] = tgt2[j + 4] for the words of the blocks, rubbish behind"""
    import torch
    nb2 = 2 * ((n_bases + 63) // 64)
    words = nb2 + 8
    d2 = torch.zeros(words, dtype=torch.int64, device="cuda")
    d2s = torch.zeros(words, dtype=torch.int64, device="cuda")
    for start, bases in regions:
        assert start % 32 == 0 and len(bases) % 32 == 0
        w = torch.from_numpy(pack2(bases).view(np.int64)).to("cuda")
        w0 = start // 32
        assert w0 + len(w) <= words
        d2[w0:w0 + len(w)] = w
        lo, hi = max(w0, 4), min(w0 + len(w), nb2)
        if lo < hi:
            d2s[lo - 4:hi - 4] = w[lo - w0:hi - w0]
    d2s[nb2 - 4:] = torch.from_numpy(rng.integers(1, 1 << 62, words - nb2 + 4, dtype=np.int64)).to("cuda")
    return d2, d2s


# ------------------------------------------------------------------------------------------------ eval_window2i, 4-byte form
N_SMALL = 1000                              # not a multiple of 64: the last block ends in padding


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(401)
    words = 2 * ((N_SMALL + 63) // 64) + 8
    bases = rng.integers(0, 4, words * 32).astype(np.uint8)                      # behind N_SMALL: the rubbish of the padding
    d2, d2s = make_tgt2(N_SMALL, [(0, bases)], rng)
    tb = bases[:N_SMALL].copy()
    # the same target at 4 bit/base, two words of rubbish behind
    b4 = np.concatenate([tb, rng.integers(0, 16, (-N_SMALL) % 16 + 64)]).astype(np.uint8)
    return dict(tb=tb, at=lambda p: tb[p], d2=d2, d2s=d2s, d4=_dev(pack4(b4)))


@pytest.mark.parametrize("stagger", [False, True])
@pytest.mark.parametrize("nw", [8, 16])
def test_eval_window2i(small, nw, stagger):
    rng = np.random.default_rng(402 + nw)
    # every t mod 64 in four consecutive 64-base blocks (both word parities; blocks that the staggered copy serves and blocks that it
    # does not), t = 0, and for every length the last window that fits
    T, L, R = make_cases(nw, [0] + list(range(256, 512)), small["at"], rng)
    T2, L2, R2 = make_cases(nw, [0], small["at"], rng, end=N_SMALL)
    T, L, R = np.concatenate([T, T2]), np.concatenate([L, L2]), np.concatenate([R, R2])
    tgt = (small["d2"], small["d2s"] if stagger else None, N_SMALL)
    want = reference(T, L, R, small["at"])
    assert int((want[1] == 0).sum()) > 1000 and int((want[1] == 1).sum()) > 1000 and int(want[1].max()) > 40
    got = run_window2i(nw, False, T, L, R, tgt)
    _compare(f"eval_window2i<{nw}, false>, tgt2s {stagger}", T, L, got, want)
    assert not got[2].any()
    # the rare form on the same (ACGT-only) windows, through window_to_iwindow: the same result
    bm, im, mm, eos = run_window_rare(nw, True, T, L, R, small["d4"], N_SMALL)
    assert np.array_equal(im, got[0]) and np.array_equal(mm, got[1]) and not eos.any()
    assert np.array_equal(bm, bitmap(want[0]))


# ------------------------------------------------------------------------------------------------ eval_window2i, 5-byte form
P32 = 1 << 32
N_WIDE = P32 + 1000
WIDE_LO = P32 - 128                          # first base of the part around 2^32 that is written


@pytest.fixture(scope="module")
def wide():
    """a tgt2 (and its staggered copy) of just over 2^32 bases, 1.07 GB each, made once: zero but for the blocks around 2^32 and - with
    other bases - the blocks at the same positions mod 2^32"""
    import torch
    rng = np.random.default_rng(403)
    words = 2 * ((N_WIDE + 63) // 64) + 8
    hi = rng.integers(0, 4, words * 32 - WIDE_LO).astype(np.uint8)               # up to the end of the padding
    lo = rng.integers(0, 4, 1024).astype(np.uint8)
    d2, d2s = make_tgt2(N_WIDE, [(0, lo), (WIDE_LO, hi)], rng)
    tb = hi[:N_WIDE - WIDE_LO]
    assert int((tb[128:128 + 896] != lo[:896]).sum()) > 600                      # a t truncated to 32 bits meets other bases
    yield dict(at=lambda p: tb[p - WIDE_LO], d2=d2, d2s=d2s)
    del d2, d2s
    torch.cuda.empty_cache()


@pytest.mark.parametrize("stagger", [False, True])
@pytest.mark.parametrize("nw", [8, 16])
def test_eval_window2i_wide_around_2_32(wide, nw, stagger):
    rng = np.random.default_rng(404 + nw)
    T, L, R = make_cases(nw, range(P32 - 64, P32 + 129), wide["at"], rng)
    T2, L2, R2 = make_cases(nw, [0], wide["at"], rng, end=N_WIDE)
    T, L, R = np.concatenate([T, T2]), np.concatenate([L, L2]), np.concatenate([R, R2])
    want = reference(T, L, R, wide["at"])
    assert int((want[1] == 0).sum()) > 400 and int(want[1].max()) > 40
    got = run_window2i(nw, True, T, L, R, (wide["d2"], wide["d2s"] if stagger else None, N_WIDE))
    _compare(f"eval_window2i<{nw}, true>, tgt2s {stagger}", T, L, got, want)


@pytest.mark.parametrize("nw", [8, 16])
def test_eval_window2i_wide_below_2_32(small, nw):
    """the 5-byte form on small positions gives what the 4-byte form gives"""
    rng = np.random.default_rng(405 + nw)
    T, L, R = make_cases(nw, range(256, 512, 3), small["at"], rng)
    want = reference(T, L, R, small["at"])
    for stagger in (False, True):
        got = run_window2i(nw, True, T, L, R, (small["d2"], small["d2s"] if stagger else None, N_SMALL))
        _compare(f"eval_window2i<{nw}, true> below 2^32, tgt2s {stagger}", T, L, got, want)


# ------------------------------------------------------------------------------------------------ eval_window_rare
N_RARE = 1500


@pytest.fixture(scope="module")
def rare():
    """N runs, single Ns and sequence ends (EOS) among random bases"""
    rng = np.random.default_rng(406)
    tb = rng.integers(0, 4, N_RARE).astype(np.uint8)
    tb[300:340] = 4
    tb[420] = 4
    tb[500] = 7
    tb[640:643] = 4
    tb[700] = 7
    tb[701] = 7
    tb[790:1000:30] = 4
    tb[1100] = 7
    b4 = np.concatenate([tb, rng.integers(1, 16, (-N_RARE) % 16 + 64)]).astype(np.uint8)
    return dict(tb=tb, at=lambda p: tb[p], d4=_dev(pack4(b4)))


def _rare_cases(nw, rare, rng, with_n):
    W = 16 * nw
    acgt = lambda p: np.where(rare["tb"][p] < 4, rare["tb"][p], 0)              # the reads hold A where the target holds N / EOS
    T, L, R = make_cases(nw, range(256, 1150, 3), acgt, rng, with_n=with_n)
    # an N of the read only over a base of the target: over an N of the target the 4-bit compare finds the codes equal, as the reference
    # aligner's loop does (see test_eval_window_rare_n_over_n), which is not the rule of this module's reference
    j = np.arange(W)[None, :]
    over = rare["tb"][np.minimum(T.astype(np.int64)[:, None] + j, N_RARE - 1)]
    R = np.where((R == 4) & (over >= 4), 0, R).astype(np.uint8)
    return T, L, R


@pytest.mark.parametrize("four", [True, False])
@pytest.mark.parametrize("nw", [8, 16])
def test_eval_window_rare(rare, nw, four):
    rng = np.random.default_rng(407 + nw)
    T, L, R = _rare_cases(nw, rare, rng, with_n=four)
    mis, mm, eos = reference(T, L, R, rare["at"])
    # an EOS inside the window, in front of it and behind it; windows with target Ns and without
    assert 1000 < int(eos.sum()) < len(T) - 1000 and int((mm == 0).sum()) > 500
    bm, im, gmm, geos = run_window_rare(nw, four, T, L, R, rare["d4"], N_RARE)
    assert np.array_equal(geos, eos), np.nonzero(geos != eos)[0][:8]
    bad = np.nonzero((bm != bitmap(mis)).any(axis=1) | (gmm != mm) | (im != imap(mis)).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), [(int(T[i]), int(L[i]), int(gmm[i]), int(mm[i])) for i in bad[:6]])


def test_eval_window_rare_n_over_n(rare):
    """the 4-bit compare is the reference aligner's: codes compared for equality (the CPU oracle's Hamming loop, `pb == tb`), so an N
    of the read over an N of the target is no mismatch - unlike an N over a base, and unlike the 2-bit form, which never meets an N in
    the target"""
    T = np.array([290, 290], dtype=U64)
    L = np.array([60, 60], dtype=np.int32)
    R = np.zeros((2, 128), dtype=np.uint8)
    R[:, :60] = np.where(rare["tb"][290:350] < 4, rare["tb"][290:350], 0)
    R[0, 15] = 4            # over target N (bases 300 .. 339 are N)
    R[1, 5] = 4             # over a base
    mis, mm, eos = reference(T, L, R, rare["at"], n_always_differs=False)
    assert mm.tolist() == [39, 41]
    bm, im, gmm, geos = run_window_rare(8, True, T, L, R, rare["d4"], N_RARE)
    assert gmm.tolist() == [39, 41] and np.array_equal(bm, bitmap(mis)) and np.array_equal(im, imap(mis)) and not geos.any()
