"""GPU unit tests of the read preparation kernels (biokanga_amd/csrc/bk_prep.hip) through their launchers under the test-only entry
points of tests/hip/preptest.hip.  The references are those of tests/prep_ref.py - plain numpy over the reads' bytes, base by base,
nothing a kernel made - and every comparison is exact.  tests/test_prep_ref_cpu.py checks the references and that the batches hold the
cases named here.  torch only carries the buffers to the device and back: every comparison is numpy's, on the host.

Every buffer a kernel writes is filled with 0xA5 before the call and followed by a guard of 256 such bytes, which must come back
untouched; where the contract says "not written" the poison must still be there.  Active lists are compared sorted (the order within a
block goes by which wave's atomic lands first), everything else byte for byte.

The same rows come out of four routes - k_prep_fused<NW, PACKED> in 8 instantiations (and there through the LDS transpose or through
direct stores), k_pack_reads + k_init_reads, k_exc_rows + k_apply_exc, k_expand_rd4 - and are compared with ONE reference.

What a packed batch's 2-bit rows hold under an exception (observed, and what the header's "ignored" allows): the field as submitted in
the forward row, its complement in the reverse row - so with zero fields an N reads A forward and T reverse, where a batch of bytes
gives A on both strands.  No kernel reads those fields: a read with an exception is flagged kReadHasN and read through its 4-bit rows,
into which k_apply_exc writes the codes.  The tests state it that way: with zero fields the 2-bit rows are compared in full with "the
fields as submitted and their reverse complement", with random fields outside the exception positions only; the 4-bit rows always in
full."""
import ctypes

import numpy as np
import pytest

import helpers
import prep_ref as ref

pytestmark = pytest.mark.gpu

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
INVALID = 1                       # hipErrorInvalidValue
GUARD = 256
NWS = (8, 16, ref.NW_LONG, ref.NW_LONGEST)


class Buf:
    """a device buffer holding a numpy array's bytes, followed by a guard of poison that get() checks"""

    def __init__(self, a):
        import torch
        a = np.ascontiguousarray(a)
        self.dtype, self.shape, self.nbytes = a.dtype, a.shape, a.nbytes
        host = np.concatenate([a.reshape(-1).view(U8), np.full(GUARD, 0xA5, dtype=U8)])
        self.t = torch.from_numpy(host).to("cuda")

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        h = self.t.cpu().numpy()
        assert (h[self.nbytes:] == 0xA5).all(), "guard behind the buffer was written"
        return h[:self.nbytes].view(self.dtype).reshape(self.shape)


def out_buf(count, dtype):
    return Buf(ref.poison(max(count, 1), dtype))


def ptr(b):
    return 0 if b is None else b.ptr


def ok(rc):
    if rc not in (0, INVALID):            # a launch that failed or faulted: nothing more is started on this device
        pytest.exit(f"hipError_t {rc} from a launcher of bk_prep.hip", returncode=3)
    assert rc == 0, f"hipError_t {rc}"


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if got.dtype.names:
        got, exp = got.view(U8).reshape(len(got), -1), exp.view(U8).reshape(len(exp), -1)
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} entries differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]:#x}, expected {exp[tuple(bad[0])]:#x}")


@pytest.fixture(scope="module")
def lib():
    import torch                  # (first: the library then shares the HIP runtime torch brings, and the tensors' pointers are its own)
    assert torch.cuda.is_available()
    lib = helpers.preptest_lib()
    assert (lib.kListStripes, lib.kNwLong, lib.kNwLongest, lib.kPackedPadWords, lib.kMaxCoresFast, lib.kReadHasN, lib.kMaxReadLenAbs, lib.sizeof_hit) == \
        (ref.LIST_STRIPES, ref.NW_LONG, ref.NW_LONGEST, ref.PACKED_PAD_WORDS, ref.MAX_CORES_FAST, ref.READ_HAS_N, ref.MAX_READ_LEN, ref.HIT_DTYPE.itemsize)
    return lib


_plans = {}


def plan_table(lib, maxlen, max_ns):
    """[rows][maxlen + 1][2]: plan_table_fill's table for reads of up to maxlen bases under the configuration that goes with max_ns"""
    key = (maxlen, ref.mm_delta_for(max_ns))
    if key not in _plans:
        cfg = (ctypes.c_int * 9)(*ref.cfg_array(max_ns))
        rows = lib.bkpt_plan_fill(cfg, maxlen, 0, None)
        assert rows >= 2
        t = np.zeros((rows, maxlen + 1, 2), dtype=U32)
        assert lib.bkpt_plan_fill(cfg, maxlen, rows, t.ctypes.data) == 0
        _plans[key] = t
    return _plans[key]


# ------------------------------------------------------------------------------------------------
# expected values of a batch, made once

_expected = {}


class Expected:
    def __init__(self, b, wpr, words2):
        self.words2 = words2
        self.rd4 = ref.rows4_plain(b, wpr)
        self.rd2 = ref.rows2_plain(b, words2) if words2 else None
        self.hasn = ref.has_n_plain(b)
        self.refused = {m: ref.refused_plain(b, m) for m in ref.MAX_NS}
        self.packed = {}

    def pack(self, b, random_fields):
        """the packed form, and the 2-bit rows of the fields as submitted with the mask of those under an exception"""
        if random_fields not in self.packed:
            words, woffs, _, exc = ref.pack_plain(b, np.random.default_rng(11) if random_fields else None)
            rd2 = ref.rows2_plain(b, self.words2, ref.packed_fields(b, words, woffs)) if self.words2 else None
            self.packed[random_fields] = (words, woffs, exc, rd2, ref.exc_mask2(b, self.words2) if self.words2 else None)
        return self.packed[random_fields]


def expected(key, b, wpr, words2):
    k = (key, wpr, words2)
    if k not in _expected:
        _expected[k] = Expected(b, wpr, words2)
    return _expected[k]


# ------------------------------------------------------------------------------------------------
class Run:
    """the buffers of one batch on the device, as bk_engine.cpp sizes them, and the calls on them"""

    def __init__(self, lib, b, inp, nw, lean, wpr, exp, random_fields=False, plan_maxlen=None, packed=None):
        self.lib, self.b, self.nw, self.lean, self.wpr, self.inp = lib, b, nw, lean, wpr, inp
        n = b.n
        a = helpers.PrepBatch()
        self.lens = Buf(b.lens)
        self.exc = None
        if inp == "bytes":
            self.src, self.offs = Buf(b.bases), Buf(b.offs)
            a.bases, a.bases_bytes = self.src.ptr, len(b.bases)
        else:
            words, woffs, exc, self.rd2_sub, self.mask2 = packed or exp.pack(b, random_fields)
            self.src, self.offs = Buf(np.concatenate([words, ref.poison(ref.PACKED_PAD_WORDS, U32)])), Buf(woffs)     # (what lies behind a read is masked off)
            a.pk_words, a.pk_words_n = self.src.ptr, len(words) + ref.PACKED_PAD_WORDS
            if len(exc):
                self.exc = Buf(exc)
                a.pk_exc, a.pk_nexc = self.exc.ptr, len(exc)
        a.offs, a.lens = self.offs.ptr, self.lens.ptr
        self.rd4 = out_buf(n * 2 * wpr, U64)
        a.rd4, a.rd4_words = self.rd4.ptr, n * 2 * wpr
        self.rd2 = out_buf(n * nw, U64) if lean else None
        if lean:
            a.rd2, a.rd2_words = self.rd2.ptr, n * nw
        self.rmeta_words = (n + 1) & ~1
        self.rmeta, self.out = out_buf(self.rmeta_words, U32), out_buf(n, ref.HIT_DTYPE)
        a.rmeta, a.rmeta_words, a.out, a.out_recs = self.rmeta.ptr, self.rmeta_words, self.out.ptr, n
        self.plan_maxlen = plan_maxlen or max(16 * nw, b.maxlen)
        a.wpr, a.n_reads, a.nw = wpr, n, nw
        self.a = a

    def set_plan(self, max_ns):
        a = self.a
        self.plan_host = plan_table(self.lib, self.plan_maxlen, max_ns)
        if self.nw:                                    # the table as bk_engine.cpp hands it on: rows of its longest read, of which this batch's are staged
            self.plan = Buf(self.plan_host)
            a.plan, a.plan_rows, a.plan_stride, a.plan_n = self.plan.ptr, self.plan_host.shape[0], self.plan_maxlen + 1, self.b.maxlen + 1

    def prep(self, max_ns):
        n = self.b.n
        self.set_plan(max_ns)
        self.act, self.cnt2 = out_buf(n, U32), Buf(np.zeros(2, dtype=U32))                     # cnt2: the list's count and cmax, as PhaseCtl holds them
        stage_words = n + (ref.LIST_STRIPES + 2) * 1024
        self.stage, self.stripe_cnt = out_buf(stage_words, U32), Buf(np.zeros(2 * ref.LIST_STRIPES * 16, dtype=U32))
        cfg = (ctypes.c_int * 9)(*ref.cfg_array(max_ns))
        ok(self.lib.bkpt_prep(ctypes.byref(self.a), cfg, self.act.ptr, n, self.cnt2.ptr, self.cnt2.ptr + 4, self.stage.ptr, stage_words, self.stripe_cnt.ptr,
                              2 * ref.LIST_STRIPES * 16))

    def check_lists(self, exp, max_ns, what):
        """rmeta, the result records, the active list with its count and cmax, the stripe counters"""
        b, n = self.b, self.b.n
        refused = exp.refused[max_ns]
        rmeta = self.rmeta.get()
        same(rmeta[:n], ref.rmeta_ref(b.lens, exp.hasn), what + " rmeta")
        if n & 1:
            assert rmeta[n] in ((0,) if self.inp == "packed" and self.nw else (0xA5A5A5A5,)), what     # (the clearing of a packed batch goes by 8-byte words)
        same(self.out.get(), ref.hits_ref(refused), what + " out")
        act_exp, cmax_exp = ref.active_ref(b.lens, refused, self.plan_host[0])
        cnt, cmax = (int(x) for x in self.cnt2.get())
        act = self.act.get()
        assert cnt == len(act_exp), (what, cnt, len(act_exp))
        same(np.sort(act[:cnt]), act_exp, what + " active list")
        assert (act[cnt:] == 0xA5A5A5A5).all(), what
        assert cmax == cmax_exp, (what, cmax, cmax_exp)
        assert not self.stripe_cnt.get().any(), what + ": stripe counters not back at zero"
        self.stage.get()
        return refused

    def rd4_lean_expected(self, exp):
        e = ref.poison(self.b.n * 2 * self.wpr, U64).reshape(self.b.n, 2, self.wpr)
        e[exp.hasn] = exp.rd4[exp.hasn]
        return e

    def check_rows(self, exp, what, random_fields=False):
        n = self.b.n
        rd4 = self.rd4.get().reshape(n, 2, self.wpr)
        same(rd4, self.rd4_lean_expected(exp) if self.lean else exp.rd4, what + " rd4")
        if self.lean:
            rd2 = self.rd2.get().reshape(n, 2, self.nw // 2)
            if self.inp == "bytes":
                same(rd2, exp.rd2, what + " rd2")
            elif not random_fields:
                same(rd2, self.rd2_sub, what + " rd2 (fields as submitted)")
                same(rd2 & ~self.mask2, exp.rd2 & ~self.mask2, what + " rd2 outside the exceptions")
            else:
                same(rd2 & ~self.mask2, exp.rd2 & ~self.mask2, what + " rd2 outside the exceptions")
        return rd4


def fused_once(lib, key, b, nw, inp, lean, random_fields=False, max_ns_list=ref.MAX_NS):
    wpr = ref.words_per_read(b.maxlen if key in ("max100", "max32") else 16 * nw)
    exp = expected(key, b, wpr, nw // 2)
    for max_ns in max_ns_list:
        what = f"{key} nw={nw} {inp} {'lean' if lean else 'full'} max_ns={max_ns}"
        r = Run(lib, b, inp, nw, lean, wpr, exp, random_fields)
        r.prep(max_ns)
        refused = r.check_lists(exp, max_ns, what)
        r.check_rows(exp, what, random_fields)
        assert 0 < refused.sum() < b.n


# ------------------------------------------------------------------------------------------------
# (a) the fused path

@pytest.mark.parametrize("lean", [False, True], ids=["full", "lean"])
@pytest.mark.parametrize("inp", ["bytes", "packed"])
@pytest.mark.parametrize("nw", NWS)
def test_fused(lib, nw, inp, lean):
    """every length 1 .. 16 nw, N runs at the word boundaries of both strands, a read of nothing but N, codes 5..7, the N limit at and one
    beyond MaxNsSeq for max_ns 0, 1 and 5"""
    fused_once(lib, f"fused{nw}", ref.fused_case(nw).batch, nw, inp, lean)


@pytest.mark.parametrize("lean", [False, True], ids=["full", "lean"])
@pytest.mark.parametrize("nw", NWS)
def test_fused_packed_random_fields(lib, nw, lean):
    """the fields under the exceptions hold anything: the 4-bit rows, the flags and the decisions do not depend on them"""
    fused_once(lib, f"fused{nw}", ref.fused_case(nw).batch, nw, "packed", lean, random_fields=True, max_ns_list=(1,))


@pytest.mark.parametrize("lean", [False, True], ids=["full", "lean"])
@pytest.mark.parametrize("inp", ["bytes", "packed"])
@pytest.mark.parametrize("kind", ref.FUSED_VARIANTS)
def test_fused_nw8_counts_and_widths(lib, kind, inp, lean):
    """nw = 8: read counts that are a multiple of 256, 64 k + 1 and 64 k + 63 - full waves leave through the LDS transpose, the partial one
    by direct stores, in one launch; batches of wpr 8 and of wpr 4, whose rows are shorter than the register window"""
    fused_once(lib, kind, ref.fused_variant(kind), 8, inp, lean, max_ns_list=(1,))


class BigExpected:
    """(g): the references of the one large batch, from the vectorised forms"""

    def __init__(self, n):
        bases, offs, lens = ref.big_lens_bases(n)
        b = ref.Batch.__new__(ref.Batch)
        b.n, b.lens, b.offs, b.bases, b.maxlen = n, lens, offs, bases, int(lens.max())
        self.b, self.wpr = b, ref.words_per_read(128)
        self.rd4, self.rd2, ns, bad = ref.rows_vec(bases, offs, lens, self.wpr, 4)
        self.hasn = bad | (ns > 0)
        self.refused = {1: ref.refused_vec(lens, ns, bad, 1)}
        words, woffs, exc = ref.pack_vec(bases, offs, lens, self.rd2[:, 0])
        # the reverse rows' fields under an exception (single N): base pos of the read is base len - 1 - pos of its reverse complement
        j = lens[exc["read"]].astype(np.int64) - 1 - exc["pos"]
        self.rmask = np.zeros((n, 4), dtype=U64)
        self.rmask[exc["read"], j // 32] = U64(3) << (62 - 2 * (j % 32)).astype(U64)
        self.packed = (words, woffs, exc, None, None)


def big_case(lib, inp):
    """(g) three times as many blocks as the device holds at once, and every row, flag and record of every one of them looked at (a
    miscompiled revcomp2 once gave wrong rows only in the blocks that did not start on a freshly zeroed register file)"""
    import torch
    n = 3 * torch.cuda.get_device_properties(0).multi_processor_count * 2048
    if "big" not in _expected:
        _expected["big"] = BigExpected(n)
    e = _expected["big"]
    b = e.b
    assert b.n == n and 0.005 * n < e.hasn.sum() < 0.015 * n and not e.refused[1].any()
    r = Run(lib, b, inp, 8, True, e.wpr, e, packed=e.packed)
    r.prep(1)
    r.check_lists(e, 1, f"big {inp}")
    same(r.rd4.get().reshape(n, 2, e.wpr), r.rd4_lean_expected(e), f"big {inp} rd4")
    rd2 = r.rd2.get().reshape(n, 2, 4)
    same(rd2[:, 0], e.rd2[:, 0], f"big {inp} rd2 forward")
    if inp == "bytes":
        same(rd2[:, 1], e.rd2[:, 1], f"big {inp} rd2 reverse")
    else:                                   # (zero fields as submitted: T where the reverse complement has the N, see the module's comment)
        same(rd2[:, 1] & ~e.rmask, e.rd2[:, 1], f"big {inp} rd2 reverse outside the exceptions")
        same(rd2[:, 1] & e.rmask, e.rmask, f"big {inp} rd2 reverse under the exceptions")


@pytest.mark.parametrize("inp", ["bytes", "packed"])
def test_later_generations_of_blocks(lib, inp):
    big_case(lib, inp)


# ------------------------------------------------------------------------------------------------
# (b) the unfused path

@pytest.mark.parametrize("inp", ["bytes", "packed"])
def test_unfused(lib, inp):
    """k_pack_reads + k_init_reads (+ k_apply_exc): reads of up to 2000 bases, the lengths around a word, around the register windows and
    the longest; an N run of 300 bases, two exception entries"""
    b = ref.unfused_case().batch
    wpr = ref.words_per_read(ref.MAX_READ_LEN)
    exp = expected("unfused", b, wpr, 0)
    for max_ns in ref.MAX_NS:
        what = f"unfused {inp} max_ns={max_ns}"
        r = Run(lib, b, inp, 0, False, wpr, exp)
        r.prep(max_ns)
        r.check_lists(exp, max_ns, what)
        r.check_rows(exp, what)


@pytest.mark.parametrize("inp", ["bytes", "packed"])
def test_unfused_equals_fused(lib, inp):
    """a batch of (a) through both paths: the same rd4, rmeta, out, active set and cmax (both equal the reference; asserted directly, so
    that a failure names the disagreement)"""
    nw = ref.NW_LONGEST
    b = ref.fused_case(nw).batch
    wpr = ref.words_per_read(16 * nw)
    exp = expected(f"fused{nw}", b, wpr, nw // 2)
    f = Run(lib, b, inp, nw, False, wpr, exp)
    u = Run(lib, b, inp, 0, False, wpr, exp, plan_maxlen=16 * nw)
    for r in (f, u):
        r.prep(5)
        r.check_lists(exp, 5, f"{inp} nw={r.nw}")
        r.check_rows(exp, f"{inp} nw={r.nw}")
    for name in ("rd4", "out"):
        same(getattr(f, name).get(), getattr(u, name).get(), name)
    same(f.rmeta.get()[:b.n], u.rmeta.get()[:b.n], "rmeta")
    fc, uc = f.cnt2.get(), u.cnt2.get()
    same(fc, uc, "count and cmax")
    same(np.sort(f.act.get()[:fc[0]]), np.sort(u.act.get()[:uc[0]]), "active set")


# ------------------------------------------------------------------------------------------------
# (c) launch_pack_rows with a list of pairs

def _mark4(codes, wpr):
    """masks of the nibbles of both strands that lie under an exception, and those nibbles' codes"""
    m = [15 if c > 3 else 0 for c in codes]
    v = [c if c > 3 else 0 for c in codes]
    return (np.array([ref.row4(m, wpr), ref.row4(list(reversed(m)), wpr)], dtype=U64), np.array([ref.row4(v, wpr), ref.row4(list(reversed(v)), wpr)], dtype=U64))


@pytest.mark.parametrize("inp", ["bytes", "packed"])
@pytest.mark.parametrize("which", ["empty", "one", "all", "third"])
def test_pack_rows_pairs(lib, which, inp):
    """the rows of the listed pairs' reads are written, in both strands; the others are not.
    Observed contract of a packed batch: k_apply_exc runs over the WHOLE exception list whatever the pairs listed, so a read that is not
    listed and has an exception gets that exception's codes written into its (otherwise untouched) rows - over poison here, over whatever
    the rows held in the library, where those are the rows the read preparation wrote for a read with an N: the same codes in the same
    places.  An empty list launches nothing, the exceptions included."""
    b = ref.fused_variant("n512")
    wpr = ref.words_per_read(128)
    exp = expected("n512", b, wpr, 4)
    n_pairs = b.n // 2
    pair_n = exp.hasn[0::2] | exp.hasn[1::2]
    rng = np.random.default_rng(5)
    pairs = {"empty": np.zeros(0, dtype=U32), "one": np.flatnonzero(pair_n)[3:4].astype(U32), "all": rng.permutation(n_pairs).astype(U32),
             "third": rng.permutation(n_pairs)[:n_pairs // 3].astype(U32)}[which]
    listed = np.zeros(b.n, dtype=bool)
    listed[2 * pairs.astype(np.int64)] = listed[2 * pairs.astype(np.int64) + 1] = True
    if which in ("one", "third"):
        assert (exp.hasn & listed).any() and (exp.hasn & ~listed).any()         # exceptions inside and outside the listed pairs
    r = Run(lib, b, inp, 0, False, wpr, exp)
    d_pairs = Buf(pairs if len(pairs) else np.zeros(1, dtype=U32))
    ok(lib.bkpt_pack_rows(ctypes.byref(r.a), d_pairs.ptr, len(pairs)))
    e = ref.poison(b.n * 2 * wpr, U64).reshape(b.n, 2, wpr)
    e[listed] = exp.rd4[listed]
    if inp == "packed" and len(pairs):
        for i in np.flatnonzero(exp.hasn & ~listed):
            m, v = _mark4(b.codes()[i], wpr)
            e[i] = (e[i] & ~m) | v
    same(r.rd4.get().reshape(b.n, 2, wpr), e, f"pairs {which} {inp}")
    beyond = Buf(np.array([n_pairs], dtype=U32))
    assert lib.bkpt_pack_rows(ctypes.byref(r.a), beyond.ptr, 1) == INVALID          # a pair beyond the batch


# ------------------------------------------------------------------------------------------------
# (d) k_expand_rd4

@pytest.mark.parametrize("inp", ["bytes", "packed"])
@pytest.mark.parametrize("nw", [8, 16])
def test_expand_rd4(lib, nw, inp):
    """after a lean read preparation: the listed reads without an N get their 4-bit rows, widened from the 2-bit rows and zero from nw to
    wpr; those with an N keep what the preparation wrote; the rows of reads not listed stay unwritten"""
    b = ref.fused_case(nw).batch
    wpr = ref.words_per_read(16 * nw)
    exp = expected(f"fused{nw}", b, wpr, nw // 2)
    perm = np.random.default_rng(9).permutation(b.n).astype(U32)
    lists = [(None, 1), (None, 255), (None, 257), (None, b.n), (perm[:b.n // 3], b.n // 3)]
    assert exp.hasn[perm[:b.n // 3]].any() and not exp.hasn[perm[:b.n // 3]].all()
    for lst, n_list in lists:
        r = Run(lib, b, inp, nw, True, wpr, exp)
        r.prep(1)
        d_list = None if lst is None else Buf(lst)
        ok(lib.bkpt_expand_rd4(ctypes.byref(r.a), ptr(d_list), n_list))
        listed = np.zeros(b.n, dtype=bool)
        listed[np.arange(n_list) if lst is None else lst] = True
        e = r.rd4_lean_expected(exp)
        todo = listed & ~exp.hasn
        e[todo] = exp.rd4[todo]
        assert (e[todo][:, :, nw:] == 0).all()
        same(r.rd4.get().reshape(b.n, 2, wpr), e, f"expand nw={nw} {inp} n_list={n_list}")
        r.rd2.get(), r.rmeta.get()
    assert lib.bkpt_expand_rd4(ctypes.byref(r.a), None, b.n + 1) == INVALID


# ------------------------------------------------------------------------------------------------
# (e) launch_compact

@pytest.mark.parametrize("pattern", ["empty", "last_only", "one_full", "random"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_compact(lib, n, pattern):
    """stripes -> dense lists behind what the lists hold; the sizes added to the totals; the maximum folded into max_out; the lines of
    lists 0..2 and the maximum lines cleared (those of the lists beyond n too, which the launch does not compact); stage unchanged"""
    S, cap = ref.LIST_STRIPES, 300
    rng = np.random.default_rng(100 * n + len(pattern))
    sizes = np.zeros((S, 3), dtype=U32)
    if pattern == "last_only":
        sizes[S - 1, :] = 1
    elif pattern == "one_full":
        sizes[17, :] = cap
    elif pattern == "random":
        sizes[:] = rng.integers(0, cap + 1, (S, 3))
        sizes[rng.random((S, 3)) < 0.3] = 0
        assert (sizes[:, :n] == 0).any() and (sizes[:, :n] == 0).sum() < S * n
    stage_host = [rng.integers(0, 1 << 32, S * cap, dtype=np.uint64).astype(U32) for _ in range(n)]
    maxima = rng.integers(1, 1000, S).astype(U32) if pattern != "empty" else np.zeros(S, dtype=U32)
    for old_tot, max_in in ((0, None), (37, 0), (37, 5000)):
        cnt_host = rng.integers(1, 1 << 32, 2 * S * 16, dtype=np.uint64).astype(U32).reshape(2 * S, 16)      # (words no kernel looks at hold anything)
        cnt_host[:S, :3] = sizes
        cnt_host[S:, 0] = maxima
        totals = [old_tot + 5 * li if old_tot else 0 for li in range(n)]
        dense_words = [totals[li] + int(sizes[:, li].sum()) for li in range(n)]
        stage = [Buf(s) for s in stage_host]
        cnt = Buf(cnt_host)
        dense = [out_buf(w, U32) for w in dense_words]
        total = [Buf(np.array([t], dtype=U32)) for t in totals]
        max_out = None if max_in is None else Buf(np.array([max_in], dtype=U32))
        arr = lambda v: (ctypes.c_uint64 * 3)(*(list(v) + [0] * (3 - len(v))))
        ok(lib.bkpt_compact(arr([s.ptr for s in stage]), S * cap, cap, cnt.ptr, 2 * S * 16, arr([d.ptr for d in dense]), arr(dense_words),
                            arr([t.ptr for t in total]), n, ptr(max_out)))
        what = f"compact n={n} {pattern} old={old_tot} max_in={max_in}"
        exp_d, exp_t = ref.compact_ref(stage_host, cap, sizes, [ref.poison(max(w, 1), U32) for w in dense_words], totals)
        for li in range(n):
            same(dense[li].get(), exp_d[li], f"{what} list {li}")
            assert int(total[li].get()[0]) == exp_t[li], what
            same(stage[li].get(), stage_host[li], f"{what} stage {li}")
        if max_out is not None:
            assert int(max_out.get()[0]) == max(max_in, int(maxima.max())), what
        cnt_exp = cnt_host.copy()
        cnt_exp[:S, :3] = 0
        cnt_exp[S:, 0] = 0
        same(cnt.get(), cnt_exp, what + " counters")
    # a stripe that claims more than its region holds, a list that would outgrow its buffer
    cnt_host[:S, :3] = sizes
    cnt_host[3, 0] = cap + 1
    over = Buf(cnt_host)
    assert lib.bkpt_compact(arr([s.ptr for s in stage]), S * cap, cap, over.ptr, 2 * S * 16, arr([d.ptr for d in dense]), arr(dense_words),
                            arr([t.ptr for t in total]), n, None) == INVALID


# ------------------------------------------------------------------------------------------------
# (f) the checks of a packed batch

@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_widen_lens(lib, n):
    lens16 = np.random.default_rng(n).integers(0, ref.MAX_READ_LEN + 1, n).astype(U16)
    lens16[0] = ref.MAX_READ_LEN
    d_lens16, lens32, nwords = Buf(lens16), out_buf(n, U32), out_buf(n, U64)
    ok(lib.bkpt_widen_lens(d_lens16.ptr, n, lens32.ptr, n, nwords.ptr, n))
    same(lens32.get(), lens16.astype(U32), "lens32")
    same(nwords.get(), np.array([(int(x) + 15) // 16 for x in lens16], dtype=U64), "words per read")
    assert lib.bkpt_widen_lens(d_lens16.ptr, n, lens32.ptr, n - 1, nwords.ptr, n) == INVALID


BIG_N = 2048 * 256 + 5              # beyond the 2048 blocks of the largest grid: the grid-stride loop runs


@pytest.mark.parametrize("n", [1, 257, BIG_N])
def test_packed_extent_and_max_len(lib, n):
    """the maxima whichever thread meets them: in the first read, in the last, in a lane other than 0 of a wave, beyond the first pass of the
    grid; folded into what the words held"""
    rng = np.random.default_rng(n)
    places = sorted({0, n - 1, min(n - 1, 64 * 3 + 17), min(n - 1, 2048 * 256 + 3)})
    for at in places:
        lens = rng.integers(1, 1000, n).astype(U32)
        offs = rng.integers(0, 1 << 40, n, dtype=np.uint64)
        lens[at] = 1999
        offs[(at + n // 2) % n] = (1 << 41) + 12345
        d_lens, d_offs = Buf(lens), Buf(offs)
        end = int((offs + ((lens.astype(U64) + U64(15)) >> U64(4))).max())
        for start in ((0, 0), (1 << 50, 1500), (5, 2000)):
            ext, mx = Buf(np.array(start, dtype=U64)), Buf(np.array([start[1]], dtype=U32))
            ok(lib.bkpt_packed_extent(d_offs.ptr, d_lens.ptr, n, ext.ptr))
            ok(lib.bkpt_max_len(d_lens.ptr, n, mx.ptr))
            assert [int(x) for x in ext.get()] == [max(start[0], end), max(start[1], 1999)], (n, at, start)
            assert int(mx.get()[0]) == max(start[1], 1999), (n, at, start)


def test_check_exc(lib):
    """k_check_exc counts the entries that break the list's rule; a valid list - adjacent runs and a run that ends on a read's last base
    among them - counts none"""
    b = ref.unfused_case().batch
    _, _, _, exc = ref.pack_plain(b)
    lens = b.lens
    assert len(exc) > 50
    same_read = exc["read"][1:] == exc["read"][:-1]
    adjacent = same_read & (exc["pos"][:-1].astype(np.int64) + exc["run"][:-1] + 1 == exc["pos"][1:])
    assert adjacent.any() and (exc["pos"].astype(np.int64) + exc["run"] + 1 == lens[exc["read"]]).any()
    d_lens = Buf(lens)

    def count(e, start=0):
        bad, d_exc = Buf(np.array([start], dtype=U32)), Buf(e)
        ok(lib.bkpt_check_exc(d_exc.ptr, len(e), d_lens.ptr, b.n, bad.ptr))
        return int(bad.get()[0]) - start

    assert ref.check_exc_ref(exc, lens) == 0 and count(exc) == 0 and count(exc, 7) == 0
    k = int(np.flatnonzero(same_read)[0]) + 1               # an entry with one of its read in front of it
    q = exc[k - 1]
    plant = {"code 3": (k, dict(code=3)), "code 8": (k, dict(code=8)), "read == n_reads": (len(exc) - 1, dict(read=b.n)),
             "pos + run == len": (k, dict(pos=int(lens[exc["read"][k]]) - 1 - int(exc["run"][k]) + 1)),
             "duplicate": (k, dict(pos=int(q["pos"]), run=int(q["run"]))),
             "overlap by one base": (k, dict(pos=int(q["pos"]) + int(q["run"]))),
             "descending read": (len(exc) // 2, dict(read=int(exc["read"][len(exc) // 2 + 1]) + 1, pos=0, run=0))}          # (the entry behind it descends)
    everything = exc.copy()
    for name, (at, change) in plant.items():
        e = exc.copy()
        for f, v in change.items():
            e[f][at] = v
            if name in ("code 3", "read == n_reads", "descending read"):
                everything[f][at] = v
        want = ref.check_exc_ref(e, lens)
        assert want >= 1, name
        assert count(e) == want, name
    want = ref.check_exc_ref(everything, lens)
    assert want >= 3 and count(everything, 2) == want
    # more than one block of entries, the violation in the last
    many = np.zeros(1000, dtype=ref.NBASE_DTYPE)
    many["read"], many["pos"], many["code"] = np.arange(1000) // 4, (np.arange(1000) % 4) * 2, 4
    ln = np.full(250, 8, dtype=U32)
    many["run"][999] = 2                                    # (its last base would be base 8 of a read of 8)
    assert ref.check_exc_ref(many, ln) == 1
    bad, d_many, d_ln = Buf(np.zeros(1, dtype=U32)), Buf(many), Buf(ln)
    ok(lib.bkpt_check_exc(d_many.ptr, 1000, d_ln.ptr, 250, bad.ptr))
    assert int(bad.get()[0]) == 1


# ------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_would_leave_a_buffer(lib):
    b = ref.fused_variant("max32")
    exp = expected("max32", b, 4, 4)

    def refused(change, inp="bytes", lean=True):
        r = Run(lib, b, inp, 8, lean, 4, exp)
        r.set_plan(1)
        change(r.a)
        n = b.n
        act, cnt2 = out_buf(n, U32), Buf(np.zeros(2, dtype=U32))
        words = n + (ref.LIST_STRIPES + 2) * 1024
        stage, sc = out_buf(words, U32), Buf(np.zeros(2 * ref.LIST_STRIPES * 16, dtype=U32))
        cfg = (ctypes.c_int * 9)(*ref.cfg_array(1))
        rc = lib.bkpt_prep(ctypes.byref(r.a), cfg, act.ptr, n, cnt2.ptr, cnt2.ptr + 4, stage.ptr, words, sc.ptr, 2 * ref.LIST_STRIPES * 16)
        if rc == INVALID:                                          # .. and nothing was launched
            assert (act.get() == 0xA5A5A5A5).all() and (r.rd4.get() == 0xA5A5A5A5A5A5A5A5).all() and (r.out.get().view(U8) == 0xA5).all()
        else:
            ok(rc)
        return rc == INVALID

    def setter(**kw):
        def f(a):
            for k, v in kw.items():
                setattr(a, k, v(a) if callable(v) else v)
        return f

    assert not refused(setter())
    for kw in (dict(nw=12), dict(wpr=3), dict(wpr=1), dict(rd4_words=lambda a: a.rd4_words - 1), dict(rd2_words=lambda a: a.rd2_words - 1),
               dict(rmeta_words=b.n if b.n & 1 else b.n - 1), dict(out_recs=b.n - 1), dict(plan_n=lambda a: a.plan_stride + 1), dict(plan_n=16 * 8 + 2, plan_stride=200),
               dict(bases_bytes=lambda a: a.bases_bytes - 1), dict(n_reads=0)):
        assert refused(setter(**kw)), kw
    assert refused(setter(pk_words_n=lambda a: a.pk_words_n - 1), inp="packed")
    assert refused(setter(nw=16), lean=True)                                    # (rd2 too small for rows of 16 words)
    long_b = ref.fused_variant("max100")
    r = Run(lib, long_b, "bytes", 8, False, 6, expected("max100", long_b, 8, 4))          # wpr below ceil(100 / 16)
    assert lib.bkpt_pack_rows(ctypes.byref(r.a), None, 0) == INVALID


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inp", ["bytes", "packed"])
def test_later_generations_of_blocks_again(lib, inp):
    """(g) a second time in this process, after everything else has run"""
    big_case(lib, inp)
