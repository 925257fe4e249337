"""GPU unit tests of the device AdaptiveTrim and the paired-end window check (biokanga_amd/csrc/bk_dev_trim.h): adaptive_trim_dev<8|32>,
pe_window_ok and pe_window_key<0|8|32> under the test-only kernels of tests/hip/devtest.hip, one candidate per lane, neighbouring lanes
with other lengths and parameters.  The reference is the CPU oracle's ora_adaptive_trim (one byte per base), all results are integers and
must be equal.  The cases come from the generator of tests/cpp/dev_trim_host.cpp (its `dump`), the one the CPU twin
(tests/test_host_devtrim.py) runs at 400 000 cases: substitutions at five rates, short and long alternating runs, constructed rows (a
mismatching run ending at bit 63 of a map word, matching runs over whole words, a single mismatch at either end, exact ties of both ratio
tests and their neighbours, equal-length ties), N in the read (with and without N in the target), EOS in the target, refused lengths and
parameters, every target phase 0..63.  Behind a read's last base and around the target windows lie random nibbles."""
import subprocess

import numpy as np
import pytest

import helpers
from test_gpu_dev_window import _dev, _host, pack4
from test_host_devtrim import trim_twin_exe

pytestmark = pytest.mark.gpu

U64 = np.uint64
N_CASES = {8: 4000, 32: 2500}                # 60 / 40 waves of 64 lanes
N_SCANS = {8: 300, 32: 100}
N_FAMILIES = 13
REFUSED = {1: "length 24", 2: "length above 64 ATW", 4: "min_trim 14", 8: "min_trim len + 1", 16: "max_mm 16", 32: "min_flank 11"}
NONE = 0xFFFFFFFFFFFFFFFF


def _load(path):
    with open(path, "rb") as f:
        n, row_bases, tgt_bases, _ = (int(x) for x in np.fromfile(f, dtype="<u4", count=4))
        c = {k: np.fromfile(f, dtype="<i4", count=n) for k in ("len", "min_trim", "max_mm", "min_flank", "family", "refused", "group", "order")}
        c["t"] = np.fromfile(f, dtype="<u8", count=n)
        c["reads"] = np.fromfile(f, dtype=np.uint8, count=n * row_bases).reshape(n, row_bases)
        c["tgt"] = np.fromfile(f, dtype=np.uint8, count=tgt_bases)
        assert len(c["tgt"]) == tgt_bases and f.read(1) == b""
    c["n"], c["row_bases"] = n, row_bases
    return c


def _oracle(c, i, min_trim, min_flank, out):
    """ora_adaptive_trim of case i -> (length, mismatches, trim5, trim3); refused parameters (-100) as 0 with zeros"""
    r = helpers.oracle_lib().ora_adaptive_trim(int(c["len"][i]), c["reads"].ctypes.data + int(i) * c["row_bases"], c["tgt"].ctypes.data + int(c["t"][i]),
                                               int(min_trim), int(c["max_mm"][i]), int(min_flank), out.ctypes.data, out.ctypes.data + 4, out.ctypes.data + 8)
    assert r >= 0 or r == -100
    return (0, 0, 0, 0) if r < 0 else (r, int(out[0]), int(out[1]), int(out[2]))


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """per ATW: the cases, on the host and on the device, and the oracle's answers (computed once, left unchanged): `trim` with the case's
    own min_trim and min_flank, `key` with min_flank 3, `whole` with min_trim = len and min_flank 3"""
    d = tmp_path_factory.mktemp("devtrim")
    exe = trim_twin_exe(d)
    out = {}
    buf = np.zeros(3, dtype=np.uint32)
    for atw in (8, 32):
        path = str(d / f"cases{atw}.bin")
        subprocess.check_call([exe, "dump", str(atw), str(N_CASES[atw]), str(N_SCANS[atw]), path])
        c = _load(path)
        n = c["n"]
        over = c["len"] > 64 * atw                                              # refused by the instantiation: the oracle is not consulted
        c["trim"] = np.array([(0, 0, 0, 0) if over[i] else _oracle(c, i, c["min_trim"][i], c["min_flank"][i], buf) for i in range(n)], dtype=np.int64)
        c["key"] = np.array([(0, 0, 0, 0) if over[i] else _oracle(c, i, c["min_trim"][i], 3, buf) for i in range(n)], dtype=np.int64)
        c["whole"] = np.array([_oracle(c, i, c["len"][i], 3, buf) for i in range(n)], dtype=np.int64)
        for a in ("trim", "key", "whole"):
            c[a].setflags(write=False)
        # on the device: rows of 4-bit words, the target with two more words of rubbish behind
        row_words = c["row_bases"] // 16
        assert row_words >= 4 * atw + 1 and int(c["len"].max()) <= 16 * (row_words - 1)       # (pe_window_ok reads the row before it looks at the length)
        assert int((c["t"] + c["len"].astype(U64)).max()) + 32 <= len(c["tgt"]) and len(c["tgt"]) % 16 == 0
        rng = np.random.default_rng(atw)
        c["row_words"] = row_words
        c["d_rows"] = _dev(pack4(c["reads"].ravel()).reshape(n, row_words))
        c["d_tgt"] = _dev(np.concatenate([pack4(c["tgt"]), rng.integers(0, 1 << 63, 2).astype(U64)]))
        for k in ("len", "t", "min_trim", "max_mm", "min_flank"):
            c["d_" + k] = _dev(c[k])
        c["d_order"] = _dev(c["order"].astype(U64))
        c["d_whole_put"] = _dev(c["len"])
        out[atw] = c
    return out


def run_pe_window(c, atw, d_min_put):
    """-> key, t5, t3, ok, mm of every case"""
    import torch
    n = c["n"]
    d_key = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_t5, d_t3, d_mm = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    d_ok = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    rc = helpers.devtest_lib().bkdt_pe_window(atw, c["d_rows"].data_ptr(), c["row_words"], c["d_len"].data_ptr(), c["d_t"].data_ptr(), c["d_tgt"].data_ptr(),
                                              c["d_max_mm"].data_ptr(), n, d_min_put.data_ptr(), c["d_order"].data_ptr(), d_key.data_ptr(), d_t5.data_ptr(),
                                              d_t3.data_ptr(), d_ok.data_ptr(), d_mm.data_ptr())
    assert rc == 0, f"hipError_t {rc}"
    return _host(d_key, U64), _host(d_t5, np.int32), _host(d_t3, np.int32), _host(d_ok, np.uint8), _host(d_mm, np.int32)


def _show(c, bad, *cols):
    return [(int(i), int(c["family"][i]), int(c["len"][i]), int(c["t"][i]) % 64, int(c["min_trim"][i]), int(c["max_mm"][i]), int(c["min_flank"][i])) +
            tuple(x[i].tolist() for x in cols) for i in bad[:6]]


@pytest.mark.parametrize("atw", [8, 32])
def test_adaptive_trim_dev(sets, atw):
    import torch
    c = sets[atw]
    n = c["n"]
    single = c["group"] < 0
    want = c["trim"]
    # the conditions on the case set, from the oracle's answers alone
    r, ln = want[single, 0], c["len"][single]
    print(f"ATW {atw}: {single.sum()} cases: {(r == 0).mean():.3f} zero, {((r > 0) & (r < ln)).mean():.3f} trimmed, {(r == ln).mean():.3f} full")
    assert (r == 0).mean() >= 0.1 and ((r > 0) & (r < ln)).mean() >= 0.1 and (r == ln).mean() >= 0.1
    for bit, what in REFUSED.items():
        assert (atw != 8 and bit == 2) or ((c["refused"][single] & bit) != 0).any(), what
    assert set(c["family"][single].tolist()) == set(range(N_FAMILIES))
    assert set((c["t"] % U64(64)).tolist()) == set(range(64))
    d = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(4)]
    rc = helpers.devtest_lib().bkdt_adaptive_trim(atw, c["d_rows"].data_ptr(), c["row_words"], c["d_len"].data_ptr(), c["d_t"].data_ptr(), c["d_tgt"].data_ptr(),
                                                  c["d_min_trim"].data_ptr(), c["d_max_mm"].data_ptr(), c["d_min_flank"].data_ptr(), n, *(x.data_ptr() for x in d))
    assert rc == 0, f"hipError_t {rc}"
    got = np.stack([_host(x, np.int32) for x in d], axis=1).astype(np.int64)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), _show(c, bad, got, want))
    assert helpers.devtest_lib().bkdt_adaptive_trim(16, c["d_rows"].data_ptr(), c["row_words"], c["d_len"].data_ptr(), c["d_t"].data_ptr(), c["d_tgt"].data_ptr(),
                                                    c["d_min_trim"].data_ptr(), c["d_max_mm"].data_ptr(), c["d_min_flank"].data_ptr(), n, *(x.data_ptr() for x in d)) == 1


def _want_whole(c):
    """pe_window_key<0>: accepted exactly when AdaptiveTrim(min_trim = len, flanks 3) keeps the read whole with at most max_mm mismatches"""
    w = c["whole"]
    ok = (w[:, 0] == c["len"]) & (w[:, 0] > 0)
    acc = ok & (w[:, 1] <= c["max_mm"])
    key = np.where(acc, ((4095 - c["len"]).astype(U64) << U64(52)) | (w[:, 1].astype(U64) << U64(40)) | c["order"].astype(U64), U64(NONE))
    return ok, acc, key


def _want_key(c):
    """pe_window_key<8|32>: no candidate exactly when r < min_put, r == 0 or (r == min_put and mismatches above max_mm)"""
    k = c["key"]
    r, mm, put = k[:, 0], k[:, 1], c["min_trim"]
    none = (r < put) | (r == 0) | ((r == put) & (mm > c["max_mm"]))
    key = np.where(none, U64(NONE), ((4095 - r).astype(U64) << U64(52)) | (mm.astype(U64) << U64(40)) | c["order"].astype(U64))
    return none, key


@pytest.mark.parametrize("atw", [8, 32])
def test_pe_window_whole(sets, atw):
    """pe_window_ok and pe_window_key<0> on the cases of either set"""
    c = sets[atw]
    ok, acc, wkey = _want_whole(c)
    assert 0.05 < acc.mean() < 0.95 and (ok & ~acc).any()
    key, t5, t3, gok, gmm = run_pe_window(c, 0, c["d_whole_put"])
    bad = np.nonzero((key != wkey) | ((gok != 0) != ok) | (acc & (gmm != c["whole"][:, 1])) | (t5 != 0) | (t3 != 0))[0]
    assert len(bad) == 0, (len(bad), _show(c, bad, key, wkey, gok, gmm, c["whole"]))


@pytest.mark.parametrize("atw", [8, 32])
def test_pe_window_key(sets, atw):
    c = sets[atw]
    none, wkey = _want_key(c)
    assert 0.1 < none.mean() < 0.9
    key, t5, t3, gok, gmm = run_pe_window(c, atw, c["d_min_trim"])
    # the trims beside a key of ~0 are not looked at: k_pe_orphan reads them from the lane with the smallest key only, and a stretch of
    # exactly min_put bases with too many mismatches leaves its trims there
    bad = np.nonzero((key != wkey) | (~none & ((t5 != c["key"][:, 2]) | (t3 != c["key"][:, 3]))))[0]
    assert len(bad) == 0, (len(bad), _show(c, bad, key, wkey, t5, t3, c["key"]))
    assert (gok == 255).all() and (gmm == -1).all()                              # pe_window_ok's outputs belong to atw 0


def _loop_pick(c, idx, min_put, buf):
    """AlignPairedRead's rule over the windows idx in order (SfxArrayV2.cpp:8400-8470): a window is taken when r > MinPutLen, or r == MinPutLen
    with fewer mismatches than the best so far; MinPutLen is then raised to r and handed to the next AdaptiveTrim call.  -> position in
    idx of the window the loop ends with, -1 = none"""
    prev_best = int(c["max_mm"][idx[0]]) + 1
    pick = -1
    for j, i in enumerate(idx):
        r, mm, _, _ = _oracle(c, i, min_put, 3, buf)
        if r > min_put or (r == min_put and mm < prev_best):
            prev_best, min_put, pick = mm, r, j
    return pick


@pytest.mark.parametrize("atw", [8, 32])
def test_smallest_key_is_the_window_the_sequential_scan_ends_with(sets, atw):
    """the claim pe_window_key rests on: the minimum of its key over the windows scanned (each computed with the initial min_put) is
    the window the reference ends with, which raises MinPutLen from window to window - for pe_window_key<ATW> and pe_window_key<0>"""
    c = sets[atw]
    buf = np.zeros(3, dtype=np.uint32)
    groups = [np.nonzero(c["group"] == g)[0] for g in range(N_SCANS[atw])]
    assert all(2 <= len(idx) <= 12 and (c["order"][idx] == np.arange(len(idx))).all() for idx in groups)
    for what, (key, *_), put in ((f"pe_window_key<{atw}>", run_pe_window(c, atw, c["d_min_trim"]), c["min_trim"]),
                                 ("pe_window_key<0>", run_pe_window(c, 0, c["d_whole_put"]), c["len"])):
        picks = []
        for idx in groups:
            want = -1 if c["len"][idx[0]] > 64 * atw and put is not c["len"] else _loop_pick(c, idx, int(put[idx[0]]), buf)
            k = key[idx]
            got = -1 if int(k.min()) == NONE else int(k.argmin())
            assert got == want, (what, int(c["len"][idx[0]]), int(put[idx[0]]), int(c["max_mm"][idx[0]]), [hex(int(x)) for x in k], got, want)
            picks.append(want)
        picks = np.array(picks)
        # scans without a placement, scans that end with the first window and scans that move on to a later one
        assert (picks < 0).sum() >= 3 and (picks == 0).sum() >= 3 and (picks > 0).sum() >= 3, (what, np.bincount(picks + 1))
