"""Shared test helpers: golden-fixture access, a ctypes binding of the CPU oracle (oracle/ is test
infrastructure - only tests/, smoke() and bench.py's cpu_baseline leg may use it), a small FASTA
reader that follows the reference's read-ingest rules, and SAM/CSV parsers."""
import ctypes
import gzip
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ORACLE_DIR = os.path.join(ROOT, "oracle")

NAR_TAGS = ["NA", "AA", "EN", "NL", "MH", "ML", "ET", "OJ", "OM", "DP", "DS", "FC", "PR", "UI", "OI", "UP", "IS", "IT", "NP", "LC"]


# ------------------------------------------------------------------------------------------------
class OraParams(ctypes.Structure):
    _fields_ = [("max_subs", ctypes.c_int32), ("min_edit_dist", ctypes.c_int32),
                ("align_strand", ctypes.c_int32), ("pmode", ctypes.c_int32),
                ("max_ns", ctypes.c_int32), ("max_ml", ctypes.c_int32),
                ("clamp_ml", ctypes.c_int32), ("best_matches", ctypes.c_int32),
                ("micro_indel_len", ctypes.c_int32), ("splice_junct_len", ctypes.c_int32), ("min_chimeric_len", ctypes.c_int32), ("reserved2", ctypes.c_int32)]


HIT_DTYPE = np.dtype([("chrom_id", "<u4"), ("match_loci", "<u4"), ("match_len", "<u2"),
                      ("low_hit_instances", "<i2"), ("rslt", "u1"), ("nar", "u1"), ("strand", "u1"),
                      ("low_mm", "i1"), ("nxt_low_mm", "i1"), ("num_hits", "u1"),
                      ("mismatches", "u1"), ("flags", "u1")])
assert HIT_DTYPE.itemsize == 20


class OraCounters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("n_reads", "n_search", "n_probe", "n_last_search", "n_cand", "n_cand_seen", "n_lcm_calls")]


def make_params(max_subs=10, min_edit_dist=1, align_strand=0, pmode=0, max_ns=1, max_ml=1, clamp_ml=0, best_matches=0, micro_indel_len=0,
                splice_junct_len=0, min_chimeric_len=0, cls=OraParams):
    p = cls()
    p.min_chimeric_len = min_chimeric_len
    p.splice_junct_len = splice_junct_len
    p.micro_indel_len = micro_indel_len
    p.clamp_ml = clamp_ml
    p.best_matches = best_matches
    p.max_subs, p.min_edit_dist, p.align_strand, p.pmode, p.max_ns, p.max_ml = \
        max_subs, min_edit_dist, align_strand, pmode, max_ns, max_ml
    return p


_oracle = None


def cxx():
    """compiler command for the C++ harnesses under tests/cpp; BK_TEST_CXXFLAGS replaces -O2, e.g.
    BK_TEST_CXXFLAGS="-O1 -g -fsanitize=address,undefined" ASAN_OPTIONS=detect_leaks=0 python -m pytest tests -m "not gpu" -k host"""
    flags = os.environ.get("BK_TEST_CXXFLAGS", "-O2").split()
    return ["g++"] + flags + ["-std=c++17"]


def oracle_lib():
    """Builds (if needed) and loads oracle/libbk_oracle.so."""
    global _oracle
    if _oracle is not None:
        return _oracle
    so = os.path.join(ORACLE_DIR, "libbk_oracle.so")
    src = os.path.join(ORACLE_DIR, "bk_oracle.c")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "libbk_oracle.so"], stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(so)
    lib.ora_sfx_load.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    lib.ora_sfx_load.restype = ctypes.c_int
    lib.ora_sfx_free.argtypes = [ctypes.c_void_p]
    lib.ora_sfx_from_memory.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                        ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
    lib.ora_sfx_from_memory.restype = ctypes.c_int
    lib.ora_align_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(OraParams), ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                    ctypes.POINTER(OraCounters), ctypes.c_int]
    lib.ora_align_batch.restype = ctypes.c_int
    lib.ora_align_batch_multi.argtypes = [ctypes.c_void_p, ctypes.POINTER(OraParams), ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.POINTER(OraCounters), ctypes.c_int]
    lib.ora_align_batch_multi.restype = ctypes.c_int
    lib.ora_align_batch_ex.argtypes = [ctypes.c_void_p, ctypes.POINTER(OraParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(OraCounters), ctypes.c_int]
    lib.ora_align_batch_ex.restype = ctypes.c_int
    lib.ora_align_batch_ex2.argtypes = [ctypes.c_void_p, ctypes.POINTER(OraParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(OraCounters), ctypes.c_int]
    lib.ora_align_batch_ex2.restype = ctypes.c_int
    lib.ora_process_paired_ends.argtypes = [ctypes.c_void_p, ctypes.POINTER(OraParams), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                            ctypes.c_void_p]
    lib.ora_process_paired_ends.restype = ctypes.c_int
    lib.ora_process_paired_ends_ex.argtypes = [ctypes.c_void_p, ctypes.POINTER(OraParams), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                               ctypes.c_void_p]
    lib.ora_process_paired_ends_ex.restype = ctypes.c_int
    lib.ora_process_paired_ends_filt.argtypes = [ctypes.c_void_p, ctypes.POINTER(OraParams), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    lib.ora_process_paired_ends_filt.restype = ctypes.c_int
    lib.ora_snp_chrom_sites.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
                                        ctypes.c_double, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.ora_snp_chrom_sites.restype = ctypes.c_int64
    lib.ora_min_core_len.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ora_min_core_len.restype = ctypes.c_int
    lib.ora_locate_first_exact.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                           ctypes.c_int64, ctypes.c_void_p]
    lib.ora_locate_first_exact.restype = ctypes.c_int64
    lib.ora_locate_last_exact.argtypes = lib.ora_locate_first_exact.argtypes
    lib.ora_locate_last_exact.restype = ctypes.c_int64
    lib.ora_locate_cores.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.ora_locate_cores.restype = None
    lib.ora_sa_element.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    lib.ora_sa_element.restype = ctypes.c_int64
    lib.ora_adaptive_trim.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.ora_adaptive_trim.restype = ctypes.c_int
    _oracle = lib
    return lib


_devtest = None


def devtest_lib():
    """biokanga_amd/lib/libbk_devtest.so: test-only kernels around the device helpers (tests/hip/devtest.hip), built by
    biokanga_amd/csrc/Makefile with everything else.  A missing library is an error.  Every launcher takes raw device pointers
    (torch tensors' data_ptr()) and returns the hipError_t."""
    global _devtest
    if _devtest is not None:
        return _devtest
    so = os.path.join(ROOT, "biokanga_amd", "lib", "libbk_devtest.so")
    if not os.path.exists(so):
        raise RuntimeError(f"{so} is missing: build it (make -C biokanga_amd/csrc)")
    lib = ctypes.CDLL(so)
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    lib.bkdt_consts.argtypes = [ctypes.POINTER(u32)]
    lib.bkdt_consts.restype = None
    for name, args in (("bkdt_lset_bucket", [vp, u32, vp]),
                       ("bkdt_lset_rounds", [vp, vp, u32, vp, vp]),
                       ("bkdt_htab_rounds", [vp, u32, u32, vp, vp, vp, u32, vp]),
                       ("bkdt_same_key", [vp, vp, u32, vp]),
                       ("bkdt_window2i", [i32, i32, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp]),
                       ("bkdt_window_rare", [i32, vp, u32, i32, vp, vp, vp, u32, vp, vp, vp, vp]),
                       ("bkdt_adaptive_trim", [i32, vp, u32, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]),
                       ("bkdt_pe_window", [i32, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]),
                       ("bkdt_search_bits", [vp, vp, vp, vp, u32, vp]),
                       ("bkdt_search_cmp", [vp, vp, vp, vp, u32, vp]),
                       ("bkdt_search_ktab", [vp, vp, vp, vp, vp, vp, vp, ctypes.c_uint64, i32, vp, u32, vp]),
                       ("bkdt_search_core", [vp, vp, vp, vp, vp, ctypes.c_uint64, i32, vp, vp, vp, u32, vp]),
                       ("bkdt_search_k2", [vp, vp, ctypes.c_uint64, vp, u32, vp]),
                       ("bkdt_search_entries", [vp, vp, vp, u32, vp, vp, u32, vp])):
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    lib.bkdt_k2_layout.argtypes = [ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    lib.bkdt_k2_layout.restype = None
    c = (u32 * 4)()
    lib.bkdt_consts(c)
    lib.kLdsSet, lib.kLdsSetFill, lib.kLdsEmpty, lib.kTombBit = (int(x) for x in c)
    _devtest = lib
    return lib


_indextest = None


def indextest_lib():
    """biokanga_amd/lib/libbk_indextest.so: the index set-up kernels of bk_index.hip under test-only entry points (tests/hip/indextest.hip),
    built by biokanga_amd/csrc/Makefile with everything else.  A missing library is an error.  Every entry point takes raw device
    pointers (torch tensors' data_ptr()) with the sizes of the buffers behind them and returns the hipError_t."""
    global _indextest
    if _indextest is not None:
        return _indextest
    so = os.path.join(ROOT, "biokanga_amd", "lib", "libbk_indextest.so")
    if not os.path.exists(so):
        raise RuntimeError(f"{so} is missing: build it (make -C biokanga_amd/csrc)")
    lib = ctypes.CDLL(so)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    for name, args in (("bkit_pack_target", [vp, u64, vp, u64]),
                       ("bkit_pack_target2", [vp, u64, vp, u64, vp, u64, i32]),
                       ("bkit_split_sa5", [vp, u64, vp, vp]),
                       ("bkit_build_ktab", [vp, u64, vp, vp, u64, vp, u64, i32, i32, i32, u64, u64, vp, u64]),
                       ("bkit_build_k2", [vp, u64, vp, vp, u64, i32, vp, vp, vp, u64, vp, u64, u64, i32]),
                       ("bkit_build_k2_levels", [vp, u64, u64]),
                       ("bkit_make_ktab2", [vp, vp, u64, u64, vp, vp]),
                       ("bkit_fill_ktab2_y", [vp, vp, u64, vp]),
                       ("bkit_pack_ktab64", [vp, u64, vp, vp, u64, vp]),
                       ("bkit_build_isa", [vp, u64, vp, u64, u64]),
                       ("bkit_count_nonzero", [vp, u64, vp]),
                       ("bkit_build_swin", [vp, u64, vp, vp, u64, vp, u64, i32]),
                       ("bkit_swin_fill", [vp, u64, vp, vp, u64, vp, u64, vp, u64, i32, u64, u64]),
                       ("bkit_swin_map", [vp, vp, u64, u32, vp, vp]),
                       ("bkit_swin_breaks", [vp, vp, u64, vp, u64, i32, vp, vp, vp, vp, u64, i32, ctypes.POINTER(i32), i32, vp, u64, u64, u64, u64, vp, u64]),
                       ("bkit_swin_cover", [vp, u64, u64, u32, u32, vp, u64, i32])):
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    lib.bkit_consts.argtypes = [ctypes.POINTER(u32)]
    lib.bkit_consts.restype = None
    c = (u32 * 10)()
    lib.bkit_consts(c)
    (lib.kSwBlkShift, lib.kSwMinRun, lib.kSwHead, lib.kSwLevels, lib.kTab2BitmapMax, lib.kK2Levels, lib.kK2Bases, lib.kSwPre3, lib.kSwPre5,
     lib.kMaxReadLenAbs) = (int(x) for x in c)
    _indextest = lib
    return lib


_preptest = None


class PrepBatch(ctypes.Structure):
    """bkpt_batch of tests/hip/preptest.hip: device pointers (0 = null) and the sizes of the buffers behind them"""
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("bases", "bases_bytes", "pk_words", "pk_words_n", "pk_exc", "pk_nexc", "pk_read0", "offs", "lens", "rd4", "rd4_words", "rd2", "rd2_words",
                 "rmeta", "rmeta_words", "out", "out_recs", "plan", "plan_rows", "plan_stride", "plan_n", "wpr", "n_reads", "nw")]


def preptest_lib():
    """biokanga_amd/lib/libbk_preptest.so: the read preparation kernels of bk_prep.hip under test-only entry points (tests/hip/preptest.hip),
    built by biokanga_amd/csrc/Makefile with everything else.  A missing library is an error.  Every entry point takes raw device
    pointers (torch tensors' data_ptr()) with the sizes of the buffers behind them and returns the hipError_t."""
    global _preptest
    if _preptest is not None:
        return _preptest
    so = os.path.join(ROOT, "biokanga_amd", "lib", "libbk_preptest.so")
    if not os.path.exists(so):
        raise RuntimeError(f"{so} is missing: build it (make -C biokanga_amd/csrc)")
    lib = ctypes.CDLL(so)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    pb, pi, pu64 = ctypes.POINTER(PrepBatch), ctypes.POINTER(i32), ctypes.POINTER(u64)
    for name, args in (("bkpt_plan_fill", [pi, i32, i32, vp]),
                       ("bkpt_prep", [pb, pi, vp, u64, vp, vp, vp, u64, vp, u64]),
                       ("bkpt_pack_rows", [pb, vp, u64]),
                       ("bkpt_expand_rd4", [pb, vp, u64]),
                       ("bkpt_compact", [pu64, u64, u32, vp, u64, pu64, pu64, pu64, i32, vp]),
                       ("bkpt_widen_lens", [vp, u64, vp, u64, vp, u64]),
                       ("bkpt_packed_extent", [vp, vp, u64, vp]),
                       ("bkpt_check_exc", [vp, u64, vp, u32, vp]),
                       ("bkpt_max_len", [vp, u64, vp])):
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    lib.bkpt_consts.argtypes = [ctypes.POINTER(u32)]
    lib.bkpt_consts.restype = None
    c = (u32 * 8)()
    lib.bkpt_consts(c)
    (lib.kListStripes, lib.kNwLong, lib.kNwLongest, lib.kPackedPadWords, lib.kMaxCoresFast, lib.kReadHasN, lib.kMaxReadLenAbs,
     lib.sizeof_hit) = (int(x) for x in c)
    _preptest = lib
    return lib


class OracleSfx:
    def __init__(self, path=None, *, seq=None, sa=None, el_size=4, entries=None):
        """path: a .sfx file; or seq (uint8, 1 B/base incl. EOS) + sa (raw little-endian element bytes or
        uint32 array) + entries [(entry_id, seq_len, start_ofs, end_ofs)] held in host memory."""
        self.lib = oracle_lib()
        h = ctypes.c_void_p()
        if path is not None:
            rc = self.lib.ora_sfx_load(path.encode(), ctypes.byref(h))
            if rc != 0:
                raise RuntimeError(f"ora_sfx_load({path}) failed: {rc}")
        else:
            self._seq = np.ascontiguousarray(seq, dtype=np.uint8)
            self._sa = np.ascontiguousarray(sa)
            self._ent = np.ascontiguousarray(np.array(entries, dtype=np.uint64).reshape(-1, 4))
            rc = self.lib.ora_sfx_from_memory(self._seq.ctypes.data, self._sa.ctypes.data, len(self._seq), el_size,
                                              self._ent.ctypes.data, len(self._ent), ctypes.byref(h))
            if rc != 0:
                raise RuntimeError(f"ora_sfx_from_memory failed: {rc}")
        self.h = h

    def close(self):
        if self.h:
            self.lib.ora_sfx_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def align(self, bases, offs, lens, params, nthreads=4):
        """bases: uint8 array (1 B/base), offs uint64, lens uint32 -> (hits structured array, counters)"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n = len(lens)
        out = np.zeros(n, dtype=HIT_DTYPE)
        ctr = OraCounters()
        rc = self.lib.ora_align_batch(self.h, ctypes.byref(params), bases.ctypes.data, offs.ctypes.data,
                                      lens.ctypes.data, n, out.ctypes.data, ctypes.byref(ctr), nthreads)
        if rc != 0:
            raise RuntimeError(f"ora_align_batch failed: {rc}")
        return out, ctr


LOCI_DTYPE = np.dtype([("chrom_id", "<u4"), ("match_loci", "<u4"), ("match_len", "<u2"), ("strand", "u1"), ("mismatches", "u1")])


def oracle_align_multi(osfx, bases, offs, lens, params, nthreads=4):
    """Multi-loci form (params.max_ml > 1) -> (hits, offs[n+1], loci) in the layout bk_batch_loci() returns."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n = len(lens)
    ml = max(1, params.max_ml)
    out = np.zeros(n, dtype=HIT_DTYPE)
    dense = np.zeros((n, ml), dtype=LOCI_DTYPE)
    ctr = OraCounters()
    rc = osfx.lib.ora_align_batch_multi(osfx.h, ctypes.byref(params), bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, n,
                                        out.ctypes.data, dense.ctypes.data, ctypes.byref(ctr), nthreads)
    if rc != 0:
        raise RuntimeError(f"ora_align_batch_multi failed: {rc}")
    cnt = np.where(out["rslt"] == 1, out["low_hit_instances"].astype(np.int64), 0)
    if params.clamp_ml:
        cnt = np.where(out["rslt"] == 3, ml, cnt)
    lo = np.zeros(n + 1, dtype=np.uint64)
    lo[1:] = np.cumsum(cnt)
    mask = np.arange(ml)[None, :] < cnt[:, None]
    return out, lo, dense[mask]


SEG2_DTYPE = np.dtype([("match_loci", "<u4"), ("match_len", "<u2"), ("read_ofs", "<u2"), ("mismatches", "u1"), ("flags", "u1"), ("score", "<u2")])


def oracle_align_indel(osfx, bases, offs, lens, params, nthreads=4):
    """params.micro_indel_len > 0 -> (hits, seg2): seg2[i].flags != 0 marks a read aligned with a microInDel"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n = len(lens)
    out = np.zeros(n, dtype=HIT_DTYPE)
    seg2 = np.zeros(n, dtype=SEG2_DTYPE)
    ctr = OraCounters()
    rc = osfx.lib.ora_align_batch_ex(osfx.h, ctypes.byref(params), bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, n,
                                     out.ctypes.data, None, seg2.ctypes.data, ctypes.byref(ctr), nthreads)
    if rc != 0:
        raise RuntimeError(f"ora_align_batch_ex failed: {rc}")
    return out, seg2


def oracle_align_multi_indel(osfx, bases, offs, lens, params, nthreads=4):
    """-r modes together with -a / -A: (hits, offs[n+1], loci, seg2) - AlignReads with MaxHits > 1 and its microInDel / splice branches"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n = len(lens)
    ml = max(1, params.max_ml)
    out = np.zeros(n, dtype=HIT_DTYPE)
    dense = np.zeros((n, ml), dtype=LOCI_DTYPE)
    seg2 = np.zeros(n, dtype=SEG2_DTYPE)
    ctr = OraCounters()
    rc = osfx.lib.ora_align_batch_ex(osfx.h, ctypes.byref(params), bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, n,
                                     out.ctypes.data, dense.ctypes.data, seg2.ctypes.data, ctypes.byref(ctr), nthreads)
    if rc != 0:
        raise RuntimeError(f"ora_align_batch_ex failed: {rc}")
    cnt = np.where(out["rslt"] == 1, out["low_hit_instances"].astype(np.int64), 0)
    if params.clamp_ml:
        cnt = np.where(out["rslt"] == 3, ml, cnt)
    lo = np.zeros(n + 1, dtype=np.uint64)
    lo[1:] = np.cumsum(cnt)
    mask = np.arange(ml)[None, :] < cnt[:, None]
    return out, lo, dense[mask], seg2


TRIMS_DTYPE = np.dtype([("left", "<u2"), ("right", "<u2"), ("chimeric", "u1"), ("reserved", "u1")])


def oracle_align_multi_chimeric(osfx, bases, offs, lens, params, nthreads=4):
    """-r modes together with -c: (hits, offs[n+1], loci, trims, seg2) - every locus of a list with its own end trims (TRIMS_DTYPE, read
    orientation; chimeric = the placement came from the chimeric call)"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n = len(lens)
    ml = max(1, params.max_ml)
    out = np.zeros(n, dtype=HIT_DTYPE)
    dense = np.zeros((n, ml), dtype=LOCI_DTYPE)
    trims = np.zeros((n, ml), dtype=TRIMS_DTYPE)
    seg2 = np.zeros(n, dtype=SEG2_DTYPE)
    ctr = OraCounters()
    rc = osfx.lib.ora_align_batch_ex2(osfx.h, ctypes.byref(params), bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, n,
                                      out.ctypes.data, dense.ctypes.data, seg2.ctypes.data, trims.ctypes.data, ctypes.byref(ctr), nthreads)
    if rc != 0:
        raise RuntimeError(f"ora_align_batch_ex2 failed: {rc}")
    cnt = np.where(out["rslt"] == 1, out["low_hit_instances"].astype(np.int64), 0)
    if params.clamp_ml:
        cnt = np.where(out["rslt"] == 3, ml, cnt)
    lo = np.zeros(n + 1, dtype=np.uint64)
    lo[1:] = np.cumsum(cnt)
    mask = np.arange(ml)[None, :] < cnt[:, None]
    return out, lo, dense[mask], trims[mask], seg2


def remove_orphan_splices(hits, seg2):
    """CAligner::RemoveOrphanSpliceJuncts (Aligner.cpp:2287-2380): same rule as for microInDels, NAR 7 (OJ).  In place."""
    return _remove_orphans(hits, seg2, 4, 7)


def remove_orphan_indels(hits, seg2):
    return _remove_orphans(hits, seg2, 1, 8)


def _remove_orphans(hits, seg2, flag, nar):
    """CAligner::RemoveOrphanMicroInDels (Aligner.cpp:2382-2470): a microInDel placement stands only if another read has its
    junction within 3 bases on both sides; the others become NAR 8 (OM).  In place."""
    idx = [i for i in range(len(hits)) if hits["nar"][i] == 1 and (seg2["flags"][i] & flag)]
    j = sorted((int(hits["chrom_id"][i]), int(hits["match_loci"][i]) + int(hits["match_len"][i]) - 1, int(seg2["match_loci"][i]), i) for i in idx)
    keep = set()
    if len(j) > 1:
        for a, b in zip(j, j[1:]):
            if a[0] == b[0] and abs(a[1] - b[1]) <= 3 and abs(a[2] - b[2]) <= 3:
                keep.add(a[3]); keep.add(b[3])
    for i in idx:
        if i not in keep:
            hits["nar"][i] = nar
            hits["num_hits"][i] = 0
            hits["low_hit_instances"][i] = 0
    return hits


def chrom_accept_table(names, exclude=(), include=()):
    """CAligner::AcceptThisChromID (Aligner.cpp:2651-2715) as a table by sequence id (1-based; entry 0 unused): a sequence passes unless an
    exclude expression matches its name and - with include expressions - only if one of those does (POSIX extended, case-insensitive)"""
    import re
    t = np.ones(len(names) + 1, dtype=np.uint8)
    for i, nm in enumerate(names):
        ok = not any(re.search(e, nm, re.I) for e in exclude)
        if ok and include:
            ok = any(re.search(e, nm, re.I) for e in include)
        t[i + 1] = 1 if ok else 0
    return t


def oracle_process_pe(osfx, params, pe_mode, min_len, max_len, pair_strand, bases, offs, lens, hits, seg2=None, accept=None):
    """in-place PE association on `hits` (PE1/PE2 interleaved); flags bit 7 = FlgPEAligned.  seg2 (one entry per read, from
    oracle_align_indel with params.min_chimeric_len set): -c together with -U, trims of recovered partners are written there.
    accept (chrom_accept_table): the -Z / -z filters, which the reference consults inside its pair rules"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    assert len(hits) % 2 == 0 and hits.flags["C_CONTIGUOUS"]
    if accept is not None:
        accept = np.ascontiguousarray(accept, dtype=np.uint8)
        assert seg2 is None or (seg2.flags["C_CONTIGUOUS"] and len(seg2) == len(hits))
        rc = osfx.lib.ora_process_paired_ends_filt(osfx.h, ctypes.byref(params), pe_mode, min_len, max_len, 1 if pair_strand else 0,
                                                   bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(hits) // 2, hits.ctypes.data,
                                                   None if seg2 is None else seg2.ctypes.data, accept.ctypes.data, len(accept))
        if rc != 0:
            raise RuntimeError(f"ora_process_paired_ends_filt failed: {rc}")
        return hits
    if seg2 is not None:
        assert seg2.flags["C_CONTIGUOUS"] and len(seg2) == len(hits)
        rc = osfx.lib.ora_process_paired_ends_ex(osfx.h, ctypes.byref(params), pe_mode, min_len, max_len, 1 if pair_strand else 0,
                                                 bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(hits) // 2, hits.ctypes.data,
                                                 seg2.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"ora_process_paired_ends_ex failed: {rc}")
        return hits
    rc = osfx.lib.ora_process_paired_ends(osfx.h, ctypes.byref(params), pe_mode, min_len, max_len, 1 if pair_strand else 0,
                                          bases.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(hits) // 2, hits.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"ora_process_paired_ends failed: {rc}")
    return hits


def interleave_pe(path1, path2, min_len=50, max_len=500):
    """reads PE1/PE2 files and interleaves accepted pairs (both mates must pass the length filter,
    CAligner::LoadRawReads Aligner.cpp:11080-11130) -> names, bases, offs, lens"""
    n1, b1, o1, l1 = read_fasta_reads(path1)
    n2, b2, o2, l2 = read_fasta_reads(path2)
    assert len(n1) == len(n2)
    names, chunks, lens = [], [], []
    for i in range(len(n1)):
        if not (min_len <= l1[i] <= max_len and min_len <= l2[i] <= max_len):
            continue
        names += [n1[i], n2[i]]
        chunks += [b1[int(o1[i]):int(o1[i]) + int(l1[i])], b2[int(o2[i]):int(o2[i]) + int(l2[i])]]
        lens += [int(l1[i]), int(l2[i])]
    lens = np.array(lens, dtype=np.uint32)
    offs = np.zeros(len(lens), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return names, np.concatenate(chunks), offs, lens


def _adj(h, g):
    """(AdjStartLoci, AdjHitLen, clip5, clip3) of a record whose end trims, if any, sit in its seg2 entry (flags bit 3)"""
    tl = tr = 0
    if g is not None and (int(g["flags"]) & 8):
        tl, tr = int(g["match_len"]), int(g["read_ofs"])
    plus = h["strand"] == ord("+")
    return int(h["match_loci"]) + (tl if plus else tr), int(h["match_len"]) - tl - tr, (tl if plus else tr), (tr if plus else tl)


def expected_pe_sam_fields(hits, i, seg2=None):
    """(flag, pos1, rnext, pnext, tlen) of read i per CAligner::ReportBAMread (Aligner.cpp:5864-5924,6036-6054); with seg2 the
    loci are the end-trimmed ones and a sixth value, the CIGAR, follows"""
    h = hits[i]
    first = i % 2 == 0
    m = hits[i + 1] if first else hits[i - 1]
    if seg2 is not None:
        mi = i + 1 if first else i - 1
        flag = 0x1 | 0x2 | (0x40 if first else 0x80)
        acc = h["nar"] == 1
        flag |= (0x10 if h["strand"] != ord("+") else 0) if acc else 0x4
        pe = bool(h["flags"] & 0x80) and bool(m["flags"] & 0x80) and m["nar"] == 1
        rnext, pnext, tlen = "*", 0, 0
        hs, hl, c5, c3 = _adj(h, seg2[i])
        if pe:
            flag |= 0x20 if m["strand"] != ord("+") else 0
            if acc:
                ms, ml, _, _ = _adj(m, seg2[mi])
                rnext, pnext = "=", ms + 1
                tlen = (ms - hs) + ml if hs <= ms else (hs - ms) + hl
        else:
            flag |= 0x8
        cigar = (f"{c5}S" if c5 else "") + f"{hl}M" + (f"{c3}S" if c3 else "") if acc else None
        return flag, (hs + 1 if acc else 0), rnext, pnext, tlen, cigar
    flag = 0x1 | 0x2 | (0x40 if first else 0x80)
    acc = h["nar"] == 1
    if acc:
        flag |= 0x10 if h["strand"] != ord("+") else 0
    else:
        flag |= 0x4
    pe = bool(h["flags"] & 0x80) and bool(m["flags"] & 0x80) and m["nar"] == 1
    rnext, pnext, tlen = "*", 0, 0
    if pe:
        flag |= 0x20 if m["strand"] != ord("+") else 0
        if acc:
            rnext = "="
            pnext = int(m["match_loci"]) + 1
            s, e = int(h["match_loci"]), int(m["match_loci"])
            tlen = (e - s) + int(m["match_len"]) if s <= e else (s - e) + int(h["match_len"])
    else:
        flag |= 0x8
    pos = int(h["match_loci"]) + 1 if acc else 0
    return flag, pos, rnext, pnext, tlen


# ------------------------------------------------------------------------------------------------
_A2S = np.full(256, 4, dtype=np.uint8)          # CFasta::Ascii2Sense (Fasta.cpp:1518): anything else -> N
for ch, v in (("a", 0), ("c", 1), ("g", 2), ("t", 3), ("u", 3)):
    _A2S[ord(ch)] = v | 0x08                    # lower case carries cRptMskFlg
    _A2S[ord(ch.upper())] = v
_A2S[ord("-")] = 6


def read_name(descr, sim=False):
    """Descriptor rule of CAligner::LoadRawReads (Aligner.cpp:10967-10974,11296-11307): if the FIRST
    descriptor of the file starts lcl|usimreads| / lcr|usimreads| every descriptor is kept whole,
    otherwise each is cut at the first whitespace (and at cMaxDescrIDLen-1 = 79 chars)."""
    if sim:
        return descr
    for i, c in enumerate(descr[:79]):
        if c.isspace():
            return descr[:i]
    return descr[:79]


def read_fasta_reads(path):
    """-> (names, bases uint8 (1 B/base), offs uint64, lens uint32); non-alpha (except '-') sloughed."""
    op = gzip.open if path.endswith(".gz") else open
    names, seqs = [], []
    cur = None
    sim = None
    with op(path, "rt") as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if cur is not None:
                    seqs.append("".join(cur))
                if sim is None:
                    sim = line[1:].startswith("lcl|usimreads|") or line[1:].startswith("lcr|usimreads|")
                names.append(read_name(line[1:], sim))
                cur = []
            elif cur is not None:
                cur.append("".join(c for c in line if c.isalpha() or c == "-"))
    if cur is not None:
        seqs.append("".join(cur))
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    offs = np.zeros(len(seqs), dtype=np.uint64)
    if len(seqs):
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    raw = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    bases = _A2S[raw]
    return names, bases, offs, lens


def filter_reads_by_len(names, bases, offs, lens, min_len=50, max_len=500):
    """default -l50 -L500 read-length acceptance (Aligner.h:92-93); under-length reads are never loaded."""
    keep = [i for i in range(len(lens)) if min_len <= lens[i] <= max_len]
    return keep


# ------------------------------------------------------------------------------------------------
def gunzip_to(src_gz, dst):
    with gzip.open(src_gz, "rb") as f, open(dst, "wb") as g:
        shutil.copyfileobj(f, g)
    return dst


def parse_sam(path):
    """-> (header lines, list of dict records)"""
    op = gzip.open if path.endswith(".gz") else open
    hdr, recs = [], []
    with op(path, "rt") as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("@"):
                hdr.append(line)
                continue
            t = line.split("\t")
            rec = dict(qname=t[0], flag=int(t[1]), rname=t[2], pos=int(t[3]), mapq=int(t[4]), cigar=t[5],
                       rnext=t[6], pnext=int(t[7]), tlen=int(t[8]), seq=t[9], qual=t[10], tags=t[11:], raw=line)
            nar = "AA"
            for tg in t[11:]:
                if tg.startswith("YU:Z:"):
                    nar = tg[5:]
            rec["nar"] = nar
            recs.append(rec)
    return hdr, recs


def parse_m0_csv(path):
    """-M0 CSV (Aligner.cpp:6380-6620): ReadID,"ar",dataset,chrom,start,end,len,strand,?,?,NumReads,mismatches,bsmap,name"""
    op = gzip.open if path.endswith(".gz") else open
    out = {}
    with op(path, "rt") as f:
        for line in f:
            t = line.rstrip("\n").split(",")
            if len(t) < 14:
                continue
            out[t[13].strip('"')] = dict(read_id=int(t[0]), chrom=t[3].strip('"'), start=int(t[4]), end=int(t[5]),
                                         length=int(t[6]), strand=t[7].strip('"'), mismatches=int(t[11]))
    return out


def gen_hash16(name):
    """CUtility::GenHash16 (libbiokanga/Utility.cpp:17-37)"""
    if not name:
        return 0
    h = 19937
    for ch in name:
        h = ((h ^ ord(ch.lower())) * 3119) & 0xFFFFFFFF
        if h & 0x80000000:
            h -= 1 << 32
        h ^= (h >> 13)
        h &= 0xFFFF
    return h or 19937


def write_sfx(path, dataset, entries, seq, sa, el_size=4):
    """Test-side writer of the reference .sfx layout (header 1224 B pack(4), block 20 B + bases + SA,
    entries 8 B + 111 B each; SfxArrayV2.h:79-104,174-187).  entries: [(name, seq_len)], seq already
    concatenated with EOS terminators, sa uint32 (el_size 4) or uint64 values (el_size 5)."""
    import struct
    n = len(seq)
    hdr = bytearray(1224)
    hdr[0:4] = b"sfx5"
    struct.pack_into("<iI", hdr, 4, 5, 0)
    blk_size = 20 + n + n * el_size
    ent_size = 8 + 111 * len(entries)
    file_len = 1224 + blk_size + ent_size
    struct.pack_into("<QQIIQQ", hdr, 12, file_len, 1224 + blk_size, ent_size, 1, blk_size, 1224)
    ds = dataset.encode()[:80]
    hdr[52:52 + len(ds)] = ds
    with open(path, "wb") as f:
        f.write(hdr)
        f.write(struct.pack("<IIQI", 1, len(entries), n, el_size))
        f.write(np.ascontiguousarray(seq, dtype=np.uint8).tobytes())
        if el_size == 4:
            f.write(np.ascontiguousarray(sa, dtype="<u4").tobytes())
        else:
            v = np.ascontiguousarray(sa, dtype="<u8")
            b = v.view(np.uint8).reshape(-1, 8)[:, :5]
            f.write(np.ascontiguousarray(b).tobytes())
        f.write(struct.pack("<II", len(entries), len(entries)))
        ofs = 0
        for i, (name, slen) in enumerate(entries):
            nm = name.encode()[:80]
            rec = struct.pack("<II", i + 1, 1) + nm + b"\0" * (81 - len(nm)) + \
                struct.pack("<HIQQ", gen_hash16(name), slen, ofs, ofs + slen - 1)
            assert len(rec) == 111
            f.write(rec)
            ofs += slen + 1


def oracle_snp_sites(sfx, bases, offs, alns, chrom_id, min_reads, min_nonref_prop, max_sites=1 << 20):
    """ora_snp_chrom_sites: (sites as SNP_SITE_DTYPE, totals[4]) of one sequence"""
    from biokanga_amd.binding import SNP_ALN_DTYPE, SNP_SITE_DTYPE
    lib = oracle_lib()
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    alns = np.ascontiguousarray(alns, dtype=SNP_ALN_DTYPE)
    sites = np.zeros(max_sites, dtype=SNP_SITE_DTYPE)
    tot = np.zeros(4, dtype=np.uint64)
    n = lib.ora_snp_chrom_sites(sfx, bases.ctypes.data, offs.ctypes.data, alns.ctypes.data, len(alns), chrom_id, min_reads, float(min_nonref_prop),
                                sites.ctypes.data, max_sites, tot.ctypes.data)
    assert 0 <= n <= max_sites, n
    return sites[:n].copy(), tot


# ------------------------------------------------------------------------------------------------
def write_big_genome(path, big_len=537_000_000, small_len=1_000_000, seed=5377):
    """FASTA with one sequence beyond the 512 Mbp a BAI index can address ("big") and a small one: i.i.d. bases from a seeded
    numpy generator, 70 columns.  Used by tests/golden/make_golden.py (reference run, here) and by the GPU test of the CSI
    index (regenerated there: the file is far too large to commit).  Returns {name: uint8 array of ASCII bases}."""
    rng = np.random.default_rng(seed)
    out = {}
    with open(path, "wb") as f:
        for name, n in (("big", big_len), ("small", small_len)):
            seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n, dtype=np.uint8)]
            out[name] = seq
            f.write(f">{name}\n".encode())
            full = n // 70
            rows = np.empty((full, 71), dtype=np.uint8)
            rows[:, :70] = seq[: full * 70].reshape(full, 70)
            rows[:, 70] = 10
            f.write(memoryview(rows))
            if n % 70:
                f.write(seq[full * 70:].tobytes() + b"\n")
    return out


# ------------------------------------------------------------------------------------------------
# tests/golden/indeledge (tests/golden/make_golden_indel_edges.py): microInDel / splice junction edge cases, some of its runs on the
# tests/golden/repeat genome
def indel_edge_params(flags):
    """the reference's flags of a run in cases.json -> (make_params / AlignParams keywords, min read length, max read length)"""
    kw, lo, hi = {}, 50, 500
    keys = {"-s": "max_subs", "-a": "micro_indel_len", "-A": "splice_junct_len", "-Q": "align_strand", "-R": "max_ml", "-c": "min_chimeric_len"}
    for f in flags:
        if f[:2] in keys:
            kw[keys[f[:2]]] = int(f[2:])
        elif f[:2] == "-l":
            lo = int(f[2:])
        elif f[:2] == "-L":
            hi = int(f[2:])
        else:
            assert f[:2] == "-r", f
    return kw, lo, hi


def indel_edge_fixture(dst):
    """unpacks the fixture into dst -> (cases.json, {genome: .sfx path}, {reads file: (names, bases, offs, lens)})"""
    import json
    src = os.path.join(GOLDEN, "indeledge")
    with open(os.path.join(src, "cases.json")) as f:
        cases = json.load(f)
    sfx = {"indeledge": gunzip_to(os.path.join(src, "genome.sfx.gz"), os.path.join(dst, "indeledge.sfx")),
           "repeat": gunzip_to(os.path.join(GOLDEN, "repeat", "genome.sfx.gz"), os.path.join(dst, "repeat.sfx"))}
    reads = {n: read_fasta_reads(os.path.join(src, n)) for n in ("reads.fa.gz", "reads_repeat.fa.gz")}
    return cases, sfx, reads


def read_sfx(path):
    """(bases incl. EOS, suffix array, [(name, seq_len)]) of a one-block .sfx file with 4-byte elements (the layout write_sfx writes; a
    .gz is read through gzip)"""
    import struct
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as f:
        raw = f.read()
    _, n_ent, n, el = struct.unpack_from("<IIQI", raw, 1224)
    assert el == 4
    seq = np.frombuffer(raw, dtype=np.uint8, count=n, offset=1244).copy()
    sa = np.frombuffer(raw, dtype="<u4", count=n, offset=1244 + n).copy()
    at = 1244 + 5 * n + 8
    ents = []
    for i in range(n_ent):
        rec = raw[at + 111 * i:at + 111 * (i + 1)]
        ents.append((rec[8:89].split(b"\0")[0].decode(), struct.unpack_from("<I", rec, 91)[0]))
    return seq, sa, ents


def rewrite_sfx_5byte(src, dst, dataset="wide"):
    """the sequences and suffix array of a .sfx file (one block, 4-byte elements) written again with 5-byte elements"""
    seq, sa, ents = read_sfx(src)
    write_sfx(dst, dataset, ents, seq, sa.astype(np.uint64), el_size=5)
    return dst
