"""GPU unit tests of the search primitives of biokanga_amd/csrc/bk_dev_util.h and bk_dev_k2.h under the test-only kernels of tests/hip/devtest.hip,
one case per lane in blocks of 64, neighbouring lanes with other functions, lengths, offsets and caps (the cases are shuffled, so the
loops diverge inside a wave as they do in k_heavy and the rescue kernels).  The cases and the arrays behind them come from the generators
of tests/cpp/dev_search_host.cpp (its `dump`, a few thousand cases per group), the ones the CPU twin tests/test_host_devsearch.py runs
at their full counts; the calls of the functions under test are the text of tests/hip/dev_search_eval.h on both sides.  Expected values
are what the twin's plain references - per-base loops over one-byte-per-base arrays, none calling a function of the two headers - gave
for exactly these cases; for search_core they are computed here from the CPU oracle (helpers.OracleSfx) on the `repeat` and `basic`
golden indexes.  All results are integers and must be equal.

search_core<true> runs with a zero sa_hi: that exercises its code path only, element values above 2^32 are covered by the sa_get and
table-view cases.  The key array of k2_count_range / k2_bounds holds about 1.3 M keys (5 MB), so level 5 of the sampled levels is
reached; levels 6 and 7 need 16 M and 268 M keys and are left out."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers
from test_gpu_dev_window import _dev, _host, pack4
from test_host_devsearch import search_twin_exe, twin_indexes

pytestmark = pytest.mark.gpu

U64 = np.uint64
CASE = np.dtype([("op", "<i4"), ("i0", "<i4"), ("i1", "<i4"), ("i2", "<i4"), ("a", "<u8"), ("b", "<u8"), ("c", "<u8")])
RES = np.dtype([("x", "<u8"), ("y", "<u8"), ("z", "<u8")])
assert CASE.itemsize == 40 and RES.itemsize == 24
NAMES = {"a": ["nib16", "bits64_2", "RdRow::nib16 (4 bit)", "RdRow::nib16 (2 bit)", "RdRow::word16 (4 bit)", "RdRow::word16 (2 bit)", "spread2to4", "squeeze2",
               "top_mask", "flags_to_bits16"],
         "b": ["cmp_core (pointer row)", "cmp_core (RdRow, 4 bit)", "cmp_core (RdRow, 2 bit)", "cmp_core_from (pointer row)", "cmp_core_from (RdRow, 2 bit)",
               "hamming", "hamming_eos"],
         "c": ["ktab_get", "ktab_get_pair", "core_range", "sa_get<true>", "sa_get<false>"],
         "d": ["search_core<false> (pointer row)", "search_core<false> (RdRow, 4 bit)", "search_core<false> (RdRow, 2 bit)", "search_core<true> (pointer row)",
               "search_core<true> (RdRow, 4 bit)", "search_core<true> (RdRow, 2 bit)"],
         "e": ["k2_make", "kx_make", "k2_cmp", "k2_nkind", "k2_mask", "ktab2_absent", "k2_count_range", "k2_bounds"],
         "f": ["find_entry", "find_entry_lds", "classify", "write_result"]}
VIEWS = ["ktab32", "ktab64", "ktab_hi + ktab32", "ktab2", "k = 0"]
B_HAMMING = 5
NO_CAP = 0xFFFFFFFFFFFFFFFF >> 1


def _load(path):
    """the arrays of a dump by name (the file's layout is said at the top of tests/cpp/dev_search_host.cpp)"""
    out = {}
    with open(path, "rb") as f:
        (count,) = np.fromfile(f, dtype="<u4", count=1)
        for _ in range(int(count)):
            name = f.read(24).rstrip(b"\0").decode()
            (esize,) = np.fromfile(f, dtype="<u4", count=1)
            (nbytes,) = np.fromfile(f, dtype="<u8", count=1)
            raw = np.fromfile(f, dtype=np.uint8, count=int(nbytes))
            assert len(raw) == nbytes
            f.read(-int(nbytes) % 8)
            dt = CASE if name.endswith("_cases") else RES if name.endswith("_want") else {1: np.uint8, 4: np.uint32, 8: np.uint64}[int(esize)]
            out[name] = raw.view(dt)
        assert f.read(1) == b""
    return out


@pytest.fixture(scope="module")
def dump(tmp_path_factory, golden_tmp):
    d = tmp_path_factory.mktemp("devsearch")
    path = str(d / "cases.bin")
    run = subprocess.run([search_twin_exe(d), "dump"] + twin_indexes(golden_tmp) + [path], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-6000:] + run.stderr[-3000:]          # (the twin checks the cases it dumps on the host first)
    out = _load(path)
    for v in out.values():
        v.setflags(write=False)
    return out


def _up(a):
    return _dev(np.array(a))                                                         # (the dump's arrays are read-only: upload a copy)


def _run(launch, cases):
    """launch(cases pointer, n, results pointer) -> the results"""
    import torch
    n = len(cases)
    d_cases = _up(cases.view(np.uint8))
    d_out = torch.full((n * RES.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = launch(d_cases.data_ptr(), n, d_out.data_ptr())
    assert rc == 0, f"hipError_t {rc}"
    return _host(d_out, np.uint8).view(RES)


def _s64(v):
    return v.astype(np.uint64).view(np.int64)


def _compare(group, cases, got, want, ok=None, extra=None):
    """every case equal (or `ok`), the message naming the function of the first differing cases and their inputs"""
    if ok is None:
        ok = (got["x"] == want["x"]) & (got["y"] == want["y"]) & (got["z"] == want["z"])
    bad = np.nonzero(~ok)[0]
    show = [(NAMES[group][cases["op"][i]],) + ((extra(i),) if extra else ()) + (f"case {i}", cases[i].tolist(), "got", [hex(int(v)) for v in got[i].tolist()],
                                                                              "want", [hex(int(v)) for v in want[i].tolist()]) for i in bad[:6]]
    assert len(bad) == 0, (f"{len(bad)} of {len(cases)} cases differ, in: " + ", ".join(sorted({NAMES[group][o] for o in cases["op"][bad]})), show)


def _every_op(group, cases, at_least=1000):
    assert set(cases["op"].tolist()) == set(range(len(NAMES[group]))), "the case set misses a function"
    assert len(cases) >= at_least


def test_row_access_and_bit_helpers(dump):
    """(a): nib16 at every pos & 15 and bits64_2 at every pos & 31 over random words, RdRow::nib16 / word16 of the 2-bit form equal to the
    4-bit form of the same N-free reads at every position, spread2to4 / squeeze2 (bits 2 and 3 of a nibble ignored), top_mask for 1..16 and
    above, flags_to_bits16 on all 65536 patterns"""
    lib = helpers.devtest_lib()
    cases, want = dump["a_cases"], dump["a_want"]
    _every_op("a", cases)
    assert set((cases["a"][cases["op"] == 0] % U64(16)).tolist()) == set(range(16)) and set((cases["a"][cases["op"] == 1] % U64(32)).tolist()) == set(range(32))
    assert (cases["op"] == 9).sum() == 65536
    w, rd4, rd2 = _up(dump["a_w"]), _up(dump["a_rd4"]), _up(dump["a_rd2"])
    got = _run(lambda c, n, o: lib.bkdt_search_bits(w.data_ptr(), rd4.data_ptr(), rd2.data_ptr(), c, n, o), cases)
    _compare("a", cases, got, want)


def test_compare_and_distance(dump):
    """(b): cmp_core (pointer row, RdRow of either form), cmp_core_from, hamming, hamming_eos against the per-base loops.  hamming's contract:
    the exact count when that is <= limit, some value > limit otherwise - that and nothing stronger; hamming_eos: 127 exactly when the window
    holds a sequence end or the count exceeds the limit"""
    lib = helpers.devtest_lib()
    cases, want = dump["b_cases"], dump["b_want"]
    _every_op("b", cases)
    cmp_ops = cases["op"] <= 2
    w = _s64(want["x"])
    for s in (-1, 0, 1):
        assert (w[cmp_ops] == s).mean() >= 0.2, f"cmp_core: sign {s} in under a fifth of the cases"
    ham = cases["op"] == B_HAMMING
    over = ham & (w > cases["i2"])
    assert 0.2 <= over[ham].mean() <= 0.8, "hamming: a regime with under a fifth of the cases"
    assert set((cases["a"] % U64(16)).tolist()) == set(range(16)) and set(cases["i0"][cmp_ops].tolist()) == set(range(41))
    assert (np.diff(cases["i1"]) != 0).mean() > 0.9                                   # neighbouring lanes: other lengths
    rd4, rd2, tgt4 = _up(dump["b_rd4"]), _up(dump["b_rd2"]), _up(dump["b_tgt4"])
    got = _run(lambda c, n, o: lib.bkdt_search_cmp(rd4.data_ptr(), rd2.data_ptr(), tgt4.data_ptr(), c, n, o), cases)
    g = _s64(got["x"])
    ok = np.where(over, g > cases["i2"], g == w) & (got["y"] == 0) & (got["z"] == 0)
    _compare("b", cases, got, want, ok)


def test_kmer_table_views(dump):
    """(c): ktab_get, ktab_get_pair and core_range over ktab32, ktab64 (starts from 2^33 on), ktab_hi + ktab32 and ktab2 of one table of order 9,
    every group boundary of the packed view and both ends among the codes; core_range with cl < k and cl >= k, an N inside and just behind
    the bases looked at, the all-t core, k = 0; sa_get<true> with non-zero high bytes"""
    lib = helpers.devtest_lib()
    cases, want = dump["c_cases"], dump["c_want"]
    _every_op("c", cases)
    n_index, k = (int(v) for v in dump["c_head"])
    pair = cases[cases["op"] == 1]
    for v in range(4):
        codes = set(pair["a"][pair["i0"] == v].tolist())
        assert {0, 4 ** k - 1, 0xFFFF, 0x10000, 0x1FFFF, 0x2FFFF, 0x3FFFF} <= codes
    cr = cases["op"] == 2
    assert set(cases["i1"][cr].tolist()) == set(range(1, 21)) and set(cases["i0"][cr].tolist()) == set(range(5))
    assert int(dump["c_tab64"].min()) >= 1 << 33 and int(dump["c_tab32"].max()) >= 1 << 31
    d = {n: _up(dump["c_" + n]) for n in ("tab32", "tab64", "pk_hi", "pk_lo", "tab2", "sa_lo", "sa_hi")}
    got = _run(lambda c, n, o: lib.bkdt_search_ktab(d["tab32"].data_ptr(), d["tab64"].data_ptr(), d["pk_hi"].data_ptr(), d["pk_lo"].data_ptr(), d["tab2"].data_ptr(),
                                                    d["sa_lo"].data_ptr(), d["sa_hi"].data_ptr(), n_index, k, c, n, o), cases)
    _compare("c", cases, got, want, extra=lambda i: "view " + VIEWS[cases["i0"][i]])


def _cmp_at(seq, probe, pos):
    """the per-base compare of a probe with the suffix at pos (sequence ends beyond the array): -1 / 0 / 1"""
    t = np.full(len(probe), 7, dtype=np.uint8)
    m = min(len(probe), len(seq) - pos)
    t[:m] = seq[pos:pos + m]
    d = np.nonzero(probe != t)[0]
    return 0 if len(d) == 0 else (-1 if probe[d[0]] < t[d[0]] else 1)


@pytest.fixture(scope="module")
def search_sets(dump, golden_tmp):
    """per configuration (index, k): the cases and the oracle's answers (computed once): first index + 1 or 0, run length"""
    lib = helpers.oracle_lib()
    sfx = [helpers.OracleSfx(p) for p in twin_indexes(golden_tmp)]
    out = []
    for cfg in range(6):
        nm = f"d{cfg}"
        cases = dump[nm + "_cases"]
        n_index, k, which = (int(v) for v in dump[nm + "_head"])
        rows = dump[nm + "_rows"].reshape(len(cases), -1)
        first, run = np.zeros(len(cases), dtype=np.int64), np.zeros(len(cases), dtype=np.int64)
        for i in range(len(cases)):
            probe = np.ascontiguousarray(rows[i, cases["i0"][i]:cases["i0"][i] + cases["i1"][i]])
            first[i] = lib.ora_locate_first_exact(sfx[which].h, probe.ctypes.data, len(probe), 0, n_index - 1, None)
            if first[i]:
                run[i] = lib.ora_locate_last_exact(sfx[which].h, probe.ctypes.data, len(probe), 0, n_index - 1, None) - first[i] + 1
        first.setflags(write=False)
        run.setflags(write=False)
        out.append(dict(cases=cases, rows=rows, first=first, run=run, n=n_index, k=k, which=which, name=nm))
    for s in sfx:
        s.close()
    return out


def test_search_core_against_the_oracle(dump, search_sets):
    """(d): search_core<false> and <true>, pointer rows and RdRow of either form, on the `repeat` and `basic` golden indexes with k = 0 and with
    tables of order 4 (32-bit) and 8 (64-bit) counted in plain code by the twin.  first = the oracle's lower bound, count = min(run, cap) when
    the run is not empty; for an absent core count is 0 and `first` must part the suffixes below the core from those above it.  Probes: cores
    cut from the target, with one substitution, with an N, all a / all t, the repeat families at 20, 25 and 26 bases, lengths 12..100; caps
    ~0 >> 1 and 1, 2, 3, 64, the run length and the run length +- 1"""
    lib = helpers.devtest_lib()
    n_all = sum(len(s["cases"]) for s in search_sets)
    run_all = np.concatenate([s["run"] for s in search_sets])
    print(f"{n_all} probes: {(run_all == 0).sum()} absent, {(run_all == 1).sum()} runs of one, {(run_all > 64).sum()} runs longer than 64")
    assert (run_all == 0).mean() >= 0.1 and (run_all == 1).mean() >= 0.1 and (run_all > 64).mean() >= 0.1
    caps = np.concatenate([s["cases"]["a"] for s in search_sets])
    assert {1, 2, 3, 64, NO_CAP} <= set(caps.tolist()) and (caps[run_all > 64] < run_all[run_all > 64].astype(U64)).sum() >= 50
    for s in search_sets:
        cases, nm, which = s["cases"], s["name"], s["which"]
        _every_op("d", cases, 500)
        assert (np.diff(cases["i1"]) != 0).mean() > 0.5 and (np.diff(cases["i0"]) != 0).mean() > 0.9      # neighbouring lanes: other lengths, offsets
        seq, sa = dump[f"d_seq{which}"], dump[f"d_sa{which}"]
        assert len(seq) == s["n"] == len(sa)
        padded = np.concatenate([seq, np.full(16 - len(seq) % 16 + 16 * 12, 7, dtype=np.uint8)])
        d_tgt4, d_sa, d_hi = _up(pack4(padded)), _up(sa), _up(np.zeros(len(sa) + 8, dtype=np.uint8))
        tab32, tab64 = dump[nm + "_tab32"], dump[nm + "_tab64"]
        assert (len(tab32) == 4 ** s["k"] + 1) + (len(tab64) == 4 ** s["k"] + 1) == (1 if s["k"] else 0)
        d_t32, d_t64 = (_up(t) if len(t) else None for t in (tab32, tab64))
        rd4, rd2 = _up(dump[nm + "_rd4"]), _up(dump[nm + "_rd2"])
        got = _run(lambda c, n, o: lib.bkdt_search_core(d_tgt4.data_ptr(), d_sa.data_ptr(), d_hi.data_ptr(), d_t32.data_ptr() if d_t32 is not None else None,
                                                        d_t64.data_ptr() if d_t64 is not None else None, s["n"], s["k"], rd4.data_ptr(), rd2.data_ptr(), c, n, o), cases)
        want = np.zeros(len(cases), dtype=RES)
        want["x"] = np.maximum(s["first"] - 1, 0)
        want["y"] = np.minimum(s["run"].astype(U64), cases["a"])
        ok = (got["y"] == want["y"]) & (got["z"] == 0)
        for i in range(len(cases)):
            if s["first"][i]:
                ok[i] &= got["x"][i] == want["x"][i]
            else:
                f = int(got["x"][i])
                probe = s["rows"][i, cases["i0"][i]:cases["i0"][i] + cases["i1"][i]]
                ok[i] &= f <= s["n"] and (f == 0 or _cmp_at(seq, probe, int(sa[f - 1])) > 0) and (f == s["n"] or _cmp_at(seq, probe, int(sa[f])) < 0)
        _compare("d", cases, got, want, ok, extra=lambda i: f"index {which}, k {s['k']}" + ("" if s["first"][i] else ", absent: first must part the suffixes"))


def test_second_level_keys(dump):
    """(e): k2_make / kx_make on suffixes of `basic` and on stretches with an N or a sequence end at every place a key looks at, k2_cmp /
    k2_nkind / k2_mask for rem2 -3..20, ktab2_absent for every mask length, k2_count_range and k2_bounds on the 1.3 M-key array (buckets of
    1 .. 1048581 keys side by side, starts at every residue mod 16, mask lengths 1..15)"""
    lib = helpers.devtest_lib()
    cases, want = dump["e_cases"], dump["e_want"]
    _every_op("e", cases)
    n_keys = int(dump["e_head"][0])
    lay = (ctypes.c_uint64 * 2)()
    lib.bkdt_k2_layout(n_keys, lay)
    assert len(dump["e_k2"]) == lay[1] and 1_200_000 < n_keys < 1_600_000                # exactly the keys and their levels: whole-line loads stay inside
    bounds = cases[cases["op"] == 7]
    assert {1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 70000, 1048576 + 5} <= set(bounds["b"].tolist())
    assert set((bounds["a"] % U64(16)).tolist()) == set(range(16)) and set(bounds["i0"].tolist()) == set(range(1, 16))
    tgt4, k2 = _up(dump["e_tgt4"]), _up(dump["e_k2"])
    got = _run(lambda c, n, o: lib.bkdt_search_k2(tgt4.data_ptr(), k2.data_ptr(), n_keys, c, n, o), cases)
    _compare("e", cases, got, want)


@pytest.mark.parametrize("table", [0, 1, 2, 3])
def test_entries_and_the_result_record(dump, table):
    """(f): find_entry and find_entry_lds with 1, 2, 128 and 129 entries separated by one-base gaps - the table loaded into LDS by a real block,
    both sides of the n_ent <= 128 switch - at every entry's first and last position, every gap (-1), before the first entry and behind the
    last; with the last table classify over its small grid and write_result for every rslt (an unexpected one included) and low_inst
    0, 1, 2, max_hits, max_hits + 1, max_hits + 5, every field of the record"""
    import torch
    lib = helpers.devtest_lib()
    nm = f"f{table}"
    cases, want = dump[nm + "_cases"], dump[nm + "_want"]
    n_ent = len(dump[nm + "_start"])
    assert n_ent == (1, 2, 128, 129)[table] and set(cases["op"].tolist()) == ({0, 1, 2, 3} if table == 3 else {0, 1})
    start, end, ids = _up(dump[nm + "_start"]), _up(dump[nm + "_end"]), _up(dump[nm + "_id"])
    hits = torch.full((len(cases) * helpers.HIT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    got = _run(lambda c, n, o: lib.bkdt_search_entries(start.data_ptr(), end.data_ptr(), ids.data_ptr(), n_ent, hits.data_ptr(), c, n, o), cases)

    def record(i):
        return "" if cases["op"][i] != 3 else str(np.array([int(want[f][i]) for f in ("x", "y", "z")], dtype="<u8").view(np.uint8)[:20].view(helpers.HIT_DTYPE)[0])
    _compare("f", cases, got, want, extra=record)
