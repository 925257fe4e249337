"""References of the read preparation (biokanga_amd/csrc/bk_prep.hip) in plain numpy, base by base: what the rows, the N decision, the
result record, the active list, the packed form, the list compaction and the exception check ARE, not how the kernels get there.
tests/test_prep_ref_cpu.py checks the references themselves (against bk.pack_reads, against the CPU oracle's N decision, the vectorised
row forms against the plain ones) and that the generated batches hold the cases tests/test_gpu_prep.py names.

Layouts (biokanga_amd/csrc/bk_device.h, include/biokanga_amd.h):
  4-bit row  16 bases per 64-bit word, first base in the top nibble, zero beyond the read's end, wpr words
  2-bit row  32 bases per 64-bit word, first base in the top bits, the low two bits of each nibble (N held as A), zero beyond the end
  forward    nibble j = byte j & 7 (bits 3..7 of a byte are quality and mask flags)
  reverse    nibble j = complement of base len-1-j: 3 - c for c < 4, codes 4..7 as they are (SeqTrans.cpp:458-512)"""
import functools

import numpy as np

U32, U64 = np.uint32, np.uint64

LIST_STRIPES = 64              # kListStripes
NW_LONG, NW_LONGEST = 20, 32   # kNwLong, kNwLongest
PACKED_PAD_WORDS = 32          # kPackedPadWords
MAX_CORES_FAST = 16            # kMaxCoresFast
READ_HAS_N = 1 << 15           # kReadHasN
MAX_READ_LEN = 2000            # kMaxReadLenAbs
NAR_NS, NAR_NOHIT = 2, 3       # BK_NAR_NS, BK_NAR_NOHIT
N = 4                          # eBaseN

HIT_DTYPE = np.dtype([("chrom_id", "<u4"), ("match_loci", "<u4"), ("match_len", "<u2"), ("low_hit_instances", "<i2"), ("rslt", "u1"), ("nar", "u1"),
                      ("strand", "u1"), ("low_mm", "i1"), ("nxt_low_mm", "i1"), ("num_hits", "u1"), ("mismatches", "u1"), ("flags", "u1")])
NBASE_DTYPE = np.dtype([("read", "<u4"), ("pos", "<u2"), ("code", "u1"), ("run", "u1")])
assert HIT_DTYPE.itemsize == 20 and NBASE_DTYPE.itemsize == 8

# DevAlignCfg in its field order: max_subs, mm_delta, align_strand, max_ns, max_hits, min_core_len, slides_per100, max_iter, heavy_thresh
# (what derive_cfg makes of the default options over a genome of less than 500 kb)
CFG = dict(max_subs=10, mm_delta=1, align_strand=0, max_ns=1, max_hits=1, min_core_len=6, slides_per100=8, max_iter=2000, heavy_thresh=64)
MAX_NS = (0, 1, 5)


def mm_delta_for(max_ns):
    """the tests' second setting: with -d 2 phase 0 has two cores a strand, with the default one - cmax is not the same number throughout"""
    return 2 if max_ns == 5 else 1


def cfg_array(max_ns):
    return [dict(CFG, max_ns=max_ns, mm_delta=mm_delta_for(max_ns))[k] for k in ("max_subs", "mm_delta", "align_strand", "max_ns", "max_hits", "min_core_len", "slides_per100", "max_iter",
                                                  "heavy_thresh")]


def words_per_read(maxlen):
    """bk_engine_int.h: 16-base words of a 4-bit row, even, at least one word of zeros behind the longest read"""
    return ((maxlen + 15) // 16 + 2) & ~1


def poison(count, dtype):
    return np.frombuffer(b"\xA5" * (count * np.dtype(dtype).itemsize), dtype=dtype).copy()


# ------------------------------------------------------------------------------------------------
# the plain forms: one base at a time

def fwd_codes(read):
    return [int(b) & 7 for b in read]


def rev_codes(codes):
    return [3 - c if c < 4 else c for c in reversed(codes)]


def row4(codes, wpr):
    w = [0] * wpr
    for j, c in enumerate(codes):
        w[j // 16] |= c << (60 - 4 * (j % 16))
    return w


def row2(codes, words):
    w = [0] * words
    for j, c in enumerate(codes):
        w[j // 32] |= (c & 3) << (62 - 2 * (j % 32))
    return w


def max_ns_seq(length, max_ns):
    """Aligner.cpp:9041-9043"""
    return max(length * max_ns // 100, max_ns) if max_ns else 0


def refused(codes, max_ns):
    """Aligner.cpp:9045-9063: the scan stops at a code above N, or at the N that is one too many; a scan that stopped refuses the read"""
    allowed, seen = max_ns_seq(len(codes), max_ns), 0
    for c in codes:
        if c > N:
            return True
        if c == N:
            seen += 1
            if seen > allowed:
                return True
    return False


def has_n(codes):
    return any(c >= N for c in codes)


# ------------------------------------------------------------------------------------------------
class Batch:
    """reads in the 1 byte/base form: a list of uint8 arrays -> bases (back to back), offs, lens"""

    def __init__(self, reads):
        self.reads = [np.ascontiguousarray(r, dtype=np.uint8) for r in reads]
        self.n = len(self.reads)
        self.lens = np.array([len(r) for r in self.reads], dtype=U32)
        self.offs = np.zeros(self.n, dtype=U64)
        self.offs[1:] = np.cumsum(self.lens[:-1], dtype=U64)
        self.bases = np.concatenate(self.reads) if self.n else np.zeros(0, dtype=np.uint8)
        self.maxlen = int(self.lens.max())
        self._codes = None

    def codes(self):
        if self._codes is None:
            self._codes = [fwd_codes(r) for r in self.reads]
        return self._codes

    def take(self, idx):
        return Batch([self.reads[i] for i in idx])


def rows4_plain(batch, wpr):
    """[read][strand][wpr]"""
    out = np.zeros((batch.n, 2, wpr), dtype=U64)
    for i, c in enumerate(batch.codes()):
        out[i, 0] = np.array(row4(c, wpr), dtype=U64)
        out[i, 1] = np.array(row4(rev_codes(c), wpr), dtype=U64)
    return out


def rows2_plain(batch, words, codes=None):
    """[read][strand][words]; codes: other forward codes than the batch's own (packed input: the fields as submitted)"""
    out = np.zeros((batch.n, 2, words), dtype=U64)
    for i, c in enumerate(batch.codes() if codes is None else codes):
        out[i, 0] = np.array(row2(c, words), dtype=U64)
        out[i, 1] = np.array(row2(rev_codes(c), words), dtype=U64)
    return out


def n_counts(batch):
    """per read: bases of code N, and whether a code above N occurs"""
    cs = batch.codes()
    return np.array([sum(1 for x in c if x == N) for c in cs], dtype=np.int64), np.array([any(x > N for x in c) for c in cs], dtype=bool)


def refused_plain(batch, max_ns):
    return np.array([refused(c, max_ns) for c in batch.codes()], dtype=bool)


def has_n_plain(batch):
    return np.array([has_n(c) for c in batch.codes()], dtype=bool)


def rmeta_ref(lens, hasn):
    return (lens.astype(U32) | np.where(hasn, READ_HAS_N, 0).astype(U32)).astype(U32)


def hits_ref(ref):
    """the default result record: all zero except nar and strand"""
    h = np.zeros(len(ref), dtype=HIT_DTYPE)
    h["nar"] = np.where(ref, NAR_NS, NAR_NOHIT)
    h["strand"] = ord("?")
    return h


# ---- the plan table's row of phase 0 (bk_plan_table.h): x = cl | cd << 11 | nc << 22, y = mm | n_phases << 6 | max_slides << 13
def plan_nc(row):
    return (row[:, 0] >> 22).astype(np.int64)


def plan_n_phases(row):
    return ((row[:, 1] >> 6) & 127).astype(np.int64)


def active_ref(lens, ref, plan_row0):
    """(sorted read numbers of the first active list, cmax): the reads not refused whose n_phases > 0; cmax = the most cores any of them has
    among those of at most MAX_CORES_FAST"""
    nph, nc = plan_n_phases(plan_row0)[lens], plan_nc(plan_row0)[lens]
    on = ~ref & (nph > 0)
    fast = nc[on & (nc <= MAX_CORES_FAST)]
    return np.flatnonzero(on).astype(U32), int(fast.max()) if len(fast) else 0


# ------------------------------------------------------------------------------------------------
# the packed form (include/biokanga_amd.h)

def pack_plain(batch, rng=None):
    """-> words, word offsets, lens16, exceptions.  A base whose code is not 0..3 leaves its field zero (rng: a random field - the header
    calls those fields ignored) and joins the exception run in front of it if that has the same code, ends right before it and holds
    fewer than 256 bases; bits past a read's end are zero."""
    words, woffs, exc = [], [], []
    for i, codes in enumerate(batch.codes()):
        woffs.append(len(words))
        w = [0] * ((len(codes) + 15) // 16)
        for j, c in enumerate(codes):
            if c > 3:
                last = exc[-1] if exc else None
                if last and last[0] == i and last[2] == c and last[1] + last[3] + 1 == j and last[3] < 255:
                    last[3] += 1
                else:
                    exc.append([i, j, c, 0])
                c = int(rng.integers(0, 4)) if rng is not None else 0
            w[j // 16] |= c << (30 - 2 * (j % 16))
        words += w
    e = np.zeros(len(exc), dtype=NBASE_DTYPE)
    for k, (r, p, c, run) in enumerate(exc):
        e[k] = (r, p, c, run)
    return np.array(words, dtype=U32), np.array(woffs, dtype=U64), batch.lens.astype(np.uint16), e


def packed_fields(batch, words, woffs):
    """the 2-bit fields as submitted, per read: what the 2-bit rows of a packed batch are made of"""
    out = []
    for i in range(batch.n):
        o = int(woffs[i])
        out.append([(int(words[o + j // 16]) >> (30 - 2 * (j % 16))) & 3 for j in range(int(batch.lens[i]))])
    return out


def exc_mask2(batch, words2):
    """[read][strand][words2] masks of the 2-bit fields that lie under an exception, in both strands' coordinates"""
    out = np.zeros((batch.n, 2, words2), dtype=U64)
    for i, c in enumerate(batch.codes()):
        m = [3 if x > 3 else 0 for x in c]
        out[i, 0] = np.array(row2(m, words2), dtype=U64)
        out[i, 1] = np.array(row2(list(reversed(m)), words2), dtype=U64)
    return out


def check_exc_ref(exc, lens):
    """k_check_exc's rule, as include/biokanga_amd.h states the list: an entry counts as bad unless its code is 4..7, its read exists, its
    run ends inside the read, and it lies strictly behind the entry in front of it - a later read, or the same read from beyond that
    entry's last base on"""
    bad = 0
    for k in range(len(exc)):
        r, p, c, run = (int(exc[k][f]) for f in ("read", "pos", "code", "run"))
        good = 4 <= c <= 7 and r < len(lens) and p + run < int(lens[r])
        if good and k > 0:
            qr, qp, qrun = (int(exc[k - 1][f]) for f in ("read", "pos", "run"))
            good = qr < r or (qr == r and qp + qrun < p)
        bad += not good
    return bad


# ------------------------------------------------------------------------------------------------
def compact_ref(stage, cap, sizes, dense, totals):
    """launch_compact: per list, stripes 0 .. LIST_STRIPES - 1 one behind the other, appended behind what the list holds.
    stage[li]: LIST_STRIPES regions of cap entries; sizes[s][li]; dense[li] arrays; totals[li] -> new dense arrays and totals"""
    out_d, out_t = [], []
    for li in range(len(dense)):
        d = dense[li].copy()
        at = int(totals[li])
        for s in range(LIST_STRIPES):
            k = int(sizes[s][li])
            d[at:at + k] = stage[li][s * cap:s * cap + k]
            at += k
        out_d.append(d)
        out_t.append(at)
    return out_d, out_t


# ------------------------------------------------------------------------------------------------
# the vectorised forms of the rows, the N counts and the flags, for batches too large for the plain ones

def _code_matrix(codes, at, lens, width):
    """[read][width]: read i = codes[at[i] : at[i] + lens[i]], zero beyond its end"""
    ln = lens.astype(np.int64)
    first = np.cumsum(ln) - ln                                     # where a read's bases start among those of all the reads
    k = np.arange(int(ln.sum()), dtype=np.int64)
    m = np.zeros((len(ln), width), dtype=np.uint8)
    m.reshape(-1)[np.repeat(np.arange(len(ln)) * width - first, ln) + k] = codes[np.repeat(at - first, ln) + k]
    return m


def _pack_rows(m, bits):
    """[read][bases] values below 2^bits, first base on top -> [read][words] of 64 bits"""
    per = 8 // bits
    n, width = m.shape
    b = np.zeros((n, width // per), dtype=np.uint8)
    for k in range(per):
        b |= (m[:, k::per] << (8 - bits * (k + 1))).astype(np.uint8)
    return np.ascontiguousarray(b).view(">u8").astype(U64)


def rows_vec(bases, offs, lens, wpr, words2, chunk=1 << 16):
    """-> rd4 [read][strand][wpr], rd2 [read][strand][words2] (None if words2 == 0), N count and above-N flag per read.
    The reverse strand: the whole array of bases turned round and complemented holds every read's reverse complement, read i's from
    total - offs[i] - lens[i] on"""
    n = len(lens)
    width = (int(lens.max()) + 31) // 32 * 32
    assert width <= 16 * wpr + 16 and (not words2 or width <= 32 * words2)
    c = bases & 7
    strands = ((c, offs.astype(np.int64)), (np.where(c < 4, 3 - c, c).astype(np.uint8)[::-1], len(bases) - offs.astype(np.int64) - lens.astype(np.int64)))
    rd4 = np.zeros((n, 2, wpr), dtype=U64)
    rd2 = np.zeros((n, 2, words2), dtype=U64) if words2 else None
    ns, bad = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for a in range(0, n, chunk):
        e = min(n, a + chunk)
        for st, (src, at) in enumerate(strands):
            m = _code_matrix(src, at[a:e], lens[a:e], width)
            if st == 0:
                ns[a:e] = (m == N).sum(axis=1)
                bad[a:e] = (m > N).any(axis=1)
            rd4[a:e, st, :min(wpr, width // 16)] = _pack_rows(m, 4)[:, :wpr]
            if words2:
                rd2[a:e, st, :width // 32] = _pack_rows(m & 3, 2)
    return rd4, rd2, ns, bad


def refused_vec(lens, ns, bad, max_ns):
    ln = lens.astype(np.int64)
    allowed = np.maximum(ln * max_ns // 100, max_ns) if max_ns else np.zeros(len(ln), dtype=np.int64)
    return bad | (ns > allowed)


# ------------------------------------------------------------------------------------------------
# the batches of tests/test_gpu_prep.py

N_STARTS = ("0", "15", "16", "17", "31", "32", "33", "len-17", "len-16", "len-1")
N_RUNS = (1, 2, 17, 33)


def _start(name, length):
    return length + int(name[3:]) if name.startswith("len") else int(name)


def _random_read(rng, length):
    """codes a, c, g, t under random upper bits 3..7"""
    return (rng.integers(0, 4, length) | (rng.integers(0, 32, length) << 3)).astype(np.uint8)


def _set_code(read, at, count, code):
    read[at:at + count] = (read[at:at + count] & 0xF8) | code


def plant_runs(reads, rng, share=0.2):
    """every (start, run length) of N_STARTS x N_RUNS in turn into about `share` of the reads, where the read is long enough to hold
    the start (a run is cut at the read's end); -> the plantings made: (read, start name, run length, start, bases planted)"""
    made, k = [], 0
    for i in np.flatnonzero(rng.random(len(reads)) < share):
        length = len(reads[i])
        for _ in range(len(N_STARTS) * len(N_RUNS)):             # the next combination this read can hold
            name, run = N_STARTS[k % len(N_STARTS)], N_RUNS[(k // len(N_STARTS)) % len(N_RUNS)]
            k += 1
            at = _start(name, length)
            if 0 <= at < length:
                cnt = min(run, length - at)
                _set_code(reads[i], at, cnt, N)
                made.append((int(i), name, run, at, cnt))
                break
    return made


def special_reads(rng, maxlen):
    """-> reads, {label: position in the list}: a read of nothing but N; codes 5, 6, 7 in the first, a middle and the last base; for
    max_ns 0, 1 and 5, reads with exactly MaxNsSeq and MaxNsSeq + 1 single N at lengths where len * max_ns / 100 is below, equal to and
    above max_ns (as far as reads of up to maxlen bases get there)"""
    reads, labels = [], {}

    def add(label, r):
        labels[label] = len(reads)
        reads.append(r)

    r = _random_read(rng, min(maxlen, 77))
    _set_code(r, 0, len(r), N)
    add("all_n", r)
    for code in (5, 6, 7):
        for where in ("first", "middle", "last"):
            r = _random_read(rng, min(maxlen, 90))
            _set_code(r, {"first": 0, "middle": len(r) // 2, "last": len(r) - 1}[where], 1, code)
            add(f"code{code}_{where}", r)
    for max_ns in MAX_NS:
        for rel, length in (("below", 60), ("equal", 100 if max_ns != 5 else 110), ("above", 250 if max_ns != 5 else 125)):
            if length > maxlen:
                length = maxlen
            if max_ns and {"below": length * max_ns // 100 >= max_ns, "equal": length * max_ns // 100 != max_ns, "above": length * max_ns // 100 <= max_ns}[rel]:
                continue                                                        # (no read this short gets there)
            for extra in (0, 1):
                count = max_ns_seq(length, max_ns) + extra
                r = _random_read(rng, length)
                for at in rng.choice(length, count, replace=False):
                    _set_code(r, int(at), 1, N)
                add(f"ns{max_ns}_{rel}_{'over' if extra else 'at'}", r)
    return reads, labels


class Case:
    """a batch with what was planted into it"""

    def __init__(self, batch, runs, labels):
        self.batch, self.runs, self.labels = batch, runs, labels


@functools.lru_cache(maxsize=None)
def fused_case(nw):
    """(a): every length 1 .. 16 nw five times, the special reads, N runs in about a fifth; shuffled"""
    rng = np.random.default_rng(1000 + nw)
    maxlen = 16 * nw
    reads = [_random_read(rng, length) for length in range(1, maxlen + 1) for _ in range(5)]
    runs = plant_runs(reads, rng)
    sp, labels = special_reads(rng, maxlen)
    order = rng.permutation(len(reads) + len(sp))
    allr = reads + sp
    where = np.empty(len(order), dtype=np.int64)
    where[order] = np.arange(len(order))                       # read k of allr is read where[k] of the batch
    runs = [(int(where[i]), name, run, at, cnt) for i, name, run, at, cnt in runs]
    labels = {k: int(where[len(reads) + v]) for k, v in labels.items()}
    return Case(Batch([allr[k] for k in order]), runs, labels)


def fused_variant(kind):
    """nw = 8: the first n reads of the batch, n a multiple of 256, 64 k + 1 and 64 k + 63 (full and partial waves in one launch); the reads of
    at most 100 bases (wpr 8) and of at most 32 (wpr 4: rows shorter than the register window)"""
    b = fused_case(8).batch
    if kind in ("n512", "n577", "n639"):
        return b.take(range(int(kind[1:])))
    top = {"max100": 100, "max32": 32}[kind]
    return b.take([i for i in range(b.n) if b.lens[i] <= top])


FUSED_VARIANTS = ("n512", "n577", "n639", "max100", "max32")
UNFUSED_LENS = (1, 15, 16, 17, 31, 32, 33, 100, 128, 129, 256, 257, 512, 513, 600, 1999, 2000)


@functools.lru_cache(maxsize=None)
def unfused_case():
    """(b): the lengths at which k_pack_reads and k_init_reads change their path, three reads of each, and 200 random ones; the planting of
    (a) and a run of 300 N, which takes two exception entries"""
    rng = np.random.default_rng(77)
    reads = [_random_read(rng, length) for length in UNFUSED_LENS for _ in range(3)]
    reads += [_random_read(rng, int(length)) for length in rng.integers(1, MAX_READ_LEN + 1, 200)]
    runs = plant_runs(reads, rng)
    sp, labels = special_reads(rng, MAX_READ_LEN)
    labels = {k: len(reads) + v for k, v in labels.items()}
    reads += sp
    r = _random_read(rng, 700)
    _set_code(r, 123, 300, N)
    labels["long_run"] = len(reads)
    reads.append(r)
    return Case(Batch(reads), runs, labels)


def big_lens_bases(n, seed=5):
    """(g): lengths 20 .. 128, one read in a hundred with one N; -> bases, offs, lens"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 129, n).astype(U32)
    offs = np.zeros(n, dtype=U64)
    offs[1:] = np.cumsum(lens[:-1], dtype=U64)
    total = int(lens.sum())
    bases = rng.integers(0, 4, total, dtype=np.uint8) | (rng.integers(0, 32, total, dtype=np.uint8) << 3)
    withn = np.flatnonzero(rng.random(n) < 0.01)
    at = offs[withn].astype(np.int64) + (rng.random(len(withn)) * lens[withn]).astype(np.int64)
    bases[at] = (bases[at] & 0xF8) | N
    return bases, offs, lens


def pack_vec(bases, offs, lens, fwd2):
    """the packed form of a batch whose exceptions are single N (big_lens_bases), from its forward 2-bit rows fwd2 [read][words] - a
    read's packed words are the 16-base halves of that row, N as a zero field: words, word offsets, exceptions"""
    nwords = (lens.astype(np.int64) + 15) // 16
    woffs = np.zeros(len(lens), dtype=U64)
    woffs[1:] = np.cumsum(nwords[:-1])
    halves = np.stack([(fwd2 >> U64(32)).astype(U32), (fwd2 & U64(0xFFFFFFFF)).astype(U32)], axis=2).reshape(len(lens), -1)
    words = halves[np.arange(halves.shape[1])[None, :] < nwords[:, None]]
    at = np.flatnonzero((bases & 7) > 3)
    rd = np.searchsorted(offs, at.astype(U64), side="right") - 1
    e = np.zeros(len(at), dtype=NBASE_DTYPE)
    e["read"], e["pos"], e["code"] = rd, at - offs[rd].astype(np.int64), bases[at] & 7
    return words, woffs, e
