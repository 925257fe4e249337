"""CPU checks of bench.py's helper code (file writers of the reference leg, profile lookup) - nothing here
touches a GPU or times anything."""
import gzip
import importlib.util
import os
import struct

import numpy as np

import helpers


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(helpers.ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_sfx_writer_matches_reference_layout(golden_tmp, tmp_path):
    """bench.write_sfx_file reproduces a reference-written .sfx from its parts"""
    b = _bench()
    ref = open(os.path.join(golden_tmp["basic"], "genome.sfx"), "rb").read()
    blk = struct.unpack_from("<Q", ref, 44)[0]
    n = struct.unpack_from("<Q", ref, blk + 8)[0]
    seq = np.frombuffer(ref, np.uint8, n, blk + 20)
    sa = np.frombuffer(ref, "<u4", n, blk + 20 + n)
    out = str(tmp_path / "w.sfx")
    b.write_sfx_file(out, seq, sa, [("chrA", 100000), ("chrB", 100000)])
    got = open(out, "rb").read()
    assert len(got) == len(ref)
    assert got[blk:] == ref[blk:]                      # block and entries byte-identical
    assert got[:52] == ref[:52]                        # magic, version, sizes, offsets (names follow)
    o = helpers.OracleSfx(out)                         # and the oracle's loader accepts it
    o.close()


def test_fasta_writer_and_profile_lookup(tmp_path):
    b = _bench()
    reads = np.arange(7 * 100, dtype=np.uint8) % 5
    p = str(tmp_path / "r.fa")
    b.write_fasta_file(p, reads, 7, 100, chunk=3)
    names, bases, offs, lens = helpers.read_fasta_reads(p)
    assert names == [f"r{i:09d}" for i in range(1, 8)] and list(lens) == [100] * 7
    assert np.array_equal(bases & 7, np.where(reads > 3, 4, reads))
    t, src = b.profiled_traffic("k_wave")
    assert t is None or (t[0] > 1e9 and t[1] >= 0 and src.endswith("_pmc_summary.csv"))


def test_fetch_size_correction_follows_the_committed_calibration():
    """random-line patterns are counted exactly; the window array's streaming runs are counted at about half (profiles/*_fetch_calibration.csv)"""
    b = _bench()
    assert b.fetch_correction("k_flat", True)[0] == 1.0 and b.fetch_correction("k_wave", False)[0] == 1.0
    f, src = b.fetch_correction("k_wave", True)
    assert 1.5 < f < 2.5, (f, src)


def test_dump_outputs_sample_is_fixed_exact_and_bounded(tmp_path):
    """--dump-outputs: one float32 / float64 array per bk_hit field, every value exact, the same seeded sample of the reads in
    every run, at most 64 MB in all"""
    import biokanga_amd as bk
    b = _bench()
    n = b.DUMP_SAMPLE_READS * 3 + 11
    hits = np.zeros(n, dtype=bk.HIT_DTYPE)
    hits["match_loci"] = np.arange(n, dtype=np.uint32) * 1237 + 0xF0000000
    hits["chrom_id"] = np.arange(n) % 24
    hits["low_mm"] = -1
    hits["low_hit_instances"] = -(np.arange(n) % 300)
    hits["nar"] = np.arange(n) % 6
    r1 = b.dump_hits(hits, str(tmp_path / "a"))
    r2 = b.dump_hits(hits, str(tmp_path / "b"))
    assert r1["reads_sampled"] == b.DUMP_SAMPLE_READS and r1["reads"] == n
    assert sorted(r1["arrays"]) == sorted(list(bk.HIT_DTYPE.names) + ["read_index"])
    total = 0
    for f in r1["arrays"]:
        x = np.load(str(tmp_path / "a" / (f + ".npy")))
        y = np.load(str(tmp_path / "b" / (f + ".npy")))
        assert x.dtype in (np.float32, np.float64) and len(x) == b.DUMP_SAMPLE_READS
        assert np.array_equal(x, y)
        total += x.nbytes
    assert total <= 64 << 20
    idx = np.load(str(tmp_path / "a" / "read_index.npy")).astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[-1] < n
    for f in bk.HIT_DTYPE.names:
        assert np.array_equal(np.load(str(tmp_path / "a" / (f + ".npy"))), hits[f][idx].astype(np.float64)), f
    small = hits[:1000]
    b.dump_hits(small, str(tmp_path / "c"))
    assert np.array_equal(np.load(str(tmp_path / "c" / "match_loci.npy")), small["match_loci"].astype(np.float64))


def test_full_is_an_option():
    """every leg beyond the headline sits behind --full: the option is there and parses"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--gpus", "0", "--full"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--gpus must be >= 1" in r.stderr and "unrecognized" not in r.stderr
