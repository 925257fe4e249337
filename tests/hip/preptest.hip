// preptest.hip - the read preparation kernels of biokanga_amd/csrc/bk_prep.hip under test-only entry points: the file is included as it
// stands (with bk_index.hip beside it, for launch_fill_u64), nothing of the library is linked in.  Built as
// biokanga_amd/lib/libbk_preptest.so (csrc/Makefile); tests/helpers.py preptest_lib() loads it.  Every entry point takes raw device
// pointers with the sizes of the buffers behind them, fills a DevBatch / DevAlignCfg with the fields its launcher reads and nothing else,
// calls the LAUNCHER on the null stream with the arguments bk_engine.cpp gives it, synchronises and returns the hipError_t.  Arguments
// that would let a kernel leave its buffers are answered with hipErrorInvalidValue and no launch: the lists a kernel indexes by (offsets,
// lengths, exceptions, pairs, read lists, stripe counters, totals) are read back first and checked against the sizes STATED, nothing else.
#include <vector>

#include "../../biokanga_amd/csrc/bk_index.hip"
#include "../../biokanga_amd/csrc/bk_prep.hip"

using namespace bk;

namespace {

constexpr int kBad = (int)hipErrorInvalidValue;

int finish()
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}

template <typename T>
bool fetch(std::vector<T> &h, const void *d, uint64_t n)
{
    h.resize(n);
    return n == 0 || hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
}

}  // namespace

extern "C" {

// a batch as the caller states it: device pointers (0 = null) and the sizes of the buffers behind them, in the units named
struct bkpt_batch {
    uint64_t bases, bases_bytes;            // 1 byte/base reads, or null ..
    uint64_t pk_words, pk_words_n;          // .. and the packed words: pk_words_n 32-bit words, the kPackedPadWords behind the last read's among them
    uint64_t pk_exc, pk_nexc, pk_read0;
    uint64_t offs, lens;                    // n_reads entries each
    uint64_t rd4, rd4_words;
    uint64_t rd2, rd2_words;                // null: every read gets 4-bit rows
    uint64_t rmeta, rmeta_words;
    uint64_t out, out_recs;
    uint64_t plan, plan_rows, plan_stride, plan_n;      // plan: plan_rows * plan_stride entries
    uint64_t wpr, n_reads, nw;
};

}  // extern "C"

namespace {

bool nw_ok(uint64_t nw) { return nw == 0 || nw == 8 || nw == 16 || nw == (uint64_t)kNwLong || nw == (uint64_t)kNwLongest; }

// what every launcher that walks the reads relies on.  lens receives the lengths
bool batch_ok(const bkpt_batch &a, std::vector<uint32_t> &lens)
{
    if (a.n_reads == 0 || a.n_reads > 0x7FFFFFFFu || !a.offs || !a.lens || !a.rd4 || (a.rd4 & 15) || (a.rd2 & 15)) return false;
    if ((a.bases != 0) == (a.pk_words != 0)) return false;
    if ((a.wpr & 1) || a.wpr < 2 || 2 * a.wpr > 256 || a.rd4_words / (2 * a.wpr) < a.n_reads) return false;
    std::vector<uint64_t> offs;
    if (!fetch(offs, (const void *)a.offs, a.n_reads) || !fetch(lens, (const void *)a.lens, a.n_reads)) return false;
    for (uint64_t i = 0; i < a.n_reads; i++) {
        const uint64_t len = lens[i], words = (len + 15) >> 4;
        if (len > (uint64_t)kMaxReadLenAbs || words > a.wpr) return false;
        if (a.bases ? (offs[i] > a.bases_bytes || len > a.bases_bytes - offs[i])
                    : (offs[i] > a.pk_words_n || words + kPackedPadWords > a.pk_words_n - offs[i]))
            return false;
    }
    if (a.pk_words && a.pk_nexc) {
        // k_apply_exc walks the words of a run on both strands: the run must end inside its read
        if (!a.pk_exc) return false;
        std::vector<bk_nbase> exc;
        if (!fetch(exc, (const void *)a.pk_exc, a.pk_nexc)) return false;
        for (const bk_nbase &e : exc) {
            const uint32_t rr = e.read - (uint32_t)a.pk_read0;
            if (rr < a.n_reads && (uint32_t)e.pos + e.run >= lens[rr]) return false;
        }
    }
    return true;
}

DevBatch dev_batch(const bkpt_batch &a)
{
    DevBatch b{};
    b.bases = (const uint8_t *)a.bases; b.offs = (const uint64_t *)a.offs; b.lens = (const uint32_t *)a.lens;
    b.pk_words = (const uint32_t *)a.pk_words; b.pk_exc = (const bk_nbase *)a.pk_exc; b.pk_nexc = a.pk_words ? a.pk_nexc : 0; b.pk_read0 = (uint32_t)a.pk_read0;
    b.rd4 = (uint64_t *)a.rd4; b.rd2 = (uint64_t *)a.rd2; b.rmeta = (uint32_t *)a.rmeta; b.out = (bk_hit *)a.out;
    b.wpr = (uint32_t)a.wpr; b.n_reads = (uint32_t)a.n_reads; b.nw = (uint32_t)a.nw;
    b.plan = (const uint2 *)a.plan; b.plan_stride = (uint32_t)a.plan_stride; b.plan_n = (uint32_t)a.plan_n;
    return b;
}

DevAlignCfg dev_cfg(const int *c)
{
    DevAlignCfg g{};
    g.max_subs = c[0]; g.mm_delta = c[1]; g.align_strand = c[2]; g.max_ns = c[3]; g.max_hits = c[4];
    g.min_core_len = c[5]; g.slides_per100 = c[6]; g.max_iter = c[7]; g.heavy_thresh = c[8];
    return g;
}

bool cfg_ok(const int *c) { return c[0] >= 0 && c[0] <= 25 && (c[1] == 1 || c[1] == 2) && c[3] >= 0 && c[3] <= 5 && c[5] >= 1 && c[6] >= 1 && c[6] <= 9; }

}  // namespace

extern "C" {

// kListStripes, kNwLong, kNwLongest, kPackedPadWords, kMaxCoresFast, kReadHasN, kMaxReadLenAbs, sizeof(bk_hit)
void bkpt_consts(uint32_t *out8)
{
    out8[0] = (uint32_t)kListStripes; out8[1] = (uint32_t)kNwLong; out8[2] = (uint32_t)kNwLongest; out8[3] = (uint32_t)kPackedPadWords;
    out8[4] = (uint32_t)kMaxCoresFast; out8[5] = kReadHasN; out8[6] = (uint32_t)kMaxReadLenAbs; out8[7] = (uint32_t)sizeof(bk_hit);
}

// cfg: the nine fields of DevAlignCfg in their order.  rows = 0: returns plan_table_rows(cfg, maxlen) and writes nothing; else fills
// out (HOST memory, rows * (maxlen + 1) entries of two words) and returns 0, or -1 where a value does not fit its field
int bkpt_plan_fill(const int *cfg, int maxlen, int rows, uint32_t *out)
{
    if (!cfg_ok(cfg) || maxlen < 1 || maxlen > kMaxReadLenAbs || rows < 0) return -2;
    const DevAlignCfg g = dev_cfg(cfg);
    if (rows == 0) return plan_table_rows(g, maxlen);
    return plan_table_fill(g, maxlen, rows, reinterpret_cast<uint2 *>(out)) ? 0 : -1;
}

// act: act_words entries, of which *act_cnt are taken; act_cnt, cmax: one word each; stage: stage_words entries; stripe_cnt: stripe_words
// words, zero.  nw = 0 selects the unfused path
int bkpt_prep(const bkpt_batch *a, const int *cfg, uint32_t *act, uint64_t act_words, uint32_t *act_cnt, uint32_t *cmax, uint32_t *stage, uint64_t stage_words,
              uint32_t *stripe_cnt, uint64_t stripe_words)
{
    std::vector<uint32_t> lens;
    if (!cfg_ok(cfg) || !nw_ok(a->nw) || !batch_ok(*a, lens)) return kBad;
    if (!act || !act_cnt || !cmax || !a->rmeta || (a->rmeta & 7) || !a->out || a->out_recs < a->n_reads) return kBad;
    if (a->rmeta_words < ((a->n_reads + 1) & ~1ULL)) return kBad;                         // (cleared in 8-byte words)
    if (a->rd2 && (a->nw == 0 || a->rd2_words / a->nw < a->n_reads)) return kBad;
    uint32_t taken = 0;
    if (hipMemcpy(&taken, act_cnt, 4, hipMemcpyDeviceToHost) != hipSuccess || (uint64_t)taken + a->n_reads > act_words) return kBad;
    if (a->nw) {
        for (uint32_t l : lens)
            if (l > 16 * a->nw) return kBad;
        if (!a->plan || a->plan_rows < 1 || a->plan_n < 1 || a->plan_n > a->plan_stride || a->plan_n > 16 * a->nw + 1) return kBad;
        if (!stage || stage_words < a->n_reads + (uint64_t)(kListStripes + 2) * 1024 || !stripe_cnt || stripe_words < 2ULL * kListStripes * 16) return kBad;
        std::vector<uint32_t> cnt;
        if (!fetch(cnt, stripe_cnt, 2ULL * kListStripes * 16)) return kBad;
        for (uint32_t v : cnt)
            if (v) return kBad;
    }
    launch_prep(dev_cfg(cfg), dev_batch(*a), act, act_cnt, cmax, stage, stripe_cnt, 0);
    return finish();
}

// pairs: null (every read) or n_pairs pair numbers, each below n_reads / 2
int bkpt_pack_rows(const bkpt_batch *a, const uint32_t *pairs, uint64_t n_pairs)
{
    std::vector<uint32_t> lens, p;
    if (!batch_ok(*a, lens) || n_pairs > a->n_reads / 2 + 1 || !fetch(p, pairs, pairs ? n_pairs : 0)) return kBad;
    for (uint32_t v : p)
        if (2ULL * v + 1 >= a->n_reads) return kBad;
    launch_pack_rows(dev_batch(*a), 0, pairs, (uint32_t)n_pairs);
    return finish();
}

// list: null (reads 0 .. n_list - 1) or n_list read numbers
int bkpt_expand_rd4(const bkpt_batch *a, const uint32_t *list, uint64_t n_list)
{
    if (a->n_reads == 0 || !nw_ok(a->nw) || a->nw == 0 || !a->rd4 || !a->rd2 || !a->rmeta || (a->wpr & 1) || a->wpr < 2 || 2 * a->wpr > 256) return kBad;
    if (a->rd4_words / (2 * a->wpr) < a->n_reads || a->rd2_words / a->nw < a->n_reads || a->rmeta_words < a->n_reads || n_list > 0xFFFFFFFFu) return kBad;
    std::vector<uint32_t> l;
    if (!fetch(l, list, list ? n_list : 0) || (!list && n_list > a->n_reads)) return kBad;
    for (uint32_t v : l)
        if (v >= a->n_reads) return kBad;
    expand_rd4(dev_batch(*a), list, (uint32_t)n_list, 0);
    return finish();
}

// stage: three pointers (HOST array) to stage_words entries each, stripe s of a list at s * cap; cnt: cnt_words words; dense, total: n
// pointers (HOST arrays); dense_words: n sizes.  The stripes' sizes and the totals are read back: what they add up to must fit
int bkpt_compact(const uint64_t *stage, uint64_t stage_words, uint32_t cap, uint32_t *cnt, uint64_t cnt_words, const uint64_t *dense, const uint64_t *dense_words,
                 const uint64_t *total, int n, uint32_t *max_out)
{
    if (n < 1 || n > 3 || !cnt || cnt_words < 2ULL * kListStripes * 16 || (uint64_t)cap * kListStripes > stage_words) return kBad;
    std::vector<uint32_t> c;
    if (!fetch(c, cnt, 2ULL * kListStripes * 16)) return kBad;
    StripeSet set{};
    set.cnt = cnt; set.cap = cap;
    uint32_t *d[3] = {nullptr, nullptr, nullptr}, *t[3] = {nullptr, nullptr, nullptr};
    for (int li = 0; li < 3; li++) set.stage[li] = (uint32_t *)stage[li < n ? li : 0];
    for (int li = 0; li < n; li++) {
        if (!stage[li] || !dense[li] || !total[li]) return kBad;
        uint64_t sum = 0;
        for (int s = 0; s < kListStripes; s++) {
            if (c[s * 16 + li] > cap) return kBad;
            sum += c[s * 16 + li];
        }
        uint32_t old = 0;
        if (hipMemcpy(&old, (const void *)total[li], 4, hipMemcpyDeviceToHost) != hipSuccess || old + sum > dense_words[li]) return kBad;
        d[li] = (uint32_t *)dense[li]; t[li] = (uint32_t *)total[li];
    }
    launch_compact(set, d, t, n, max_out, 0);
    return finish();
}

int bkpt_widen_lens(const uint16_t *lens16, uint64_t n, uint32_t *lens32, uint64_t lens32_n, unsigned long long *nwords, uint64_t nwords_n)
{
    if (n == 0 || n > 0xFFFFFFFFu || n > lens32_n || n > nwords_n) return kBad;
    launch_widen_lens(lens16, (uint32_t)n, lens32, nwords, 0);
    return finish();
}

// out: two 8-byte words, which the kernel folds its maxima into
int bkpt_packed_extent(const uint64_t *offs, const uint32_t *lens, uint64_t n, unsigned long long *out)
{
    if (n == 0 || n > 0xFFFFFFFFu || !out) return kBad;
    launch_packed_extent(offs, lens, (uint32_t)n, out, 0);
    return finish();
}

// lens: n_reads entries; bad: one word, which the kernel adds to
int bkpt_check_exc(const bk_nbase *exc, uint64_t n_exc, const uint32_t *lens, uint32_t n_reads, uint32_t *bad)
{
    if (n_exc == 0 || n_exc > 0xFFFFFFFFu || !exc || !lens || !bad) return kBad;
    launch_check_exc(exc, n_exc, lens, n_reads, bad, 0);
    return finish();
}

// out: one word, which the kernel folds its maximum into
int bkpt_max_len(const uint32_t *lens, uint64_t n, uint32_t *out)
{
    if (n == 0 || n > 0xFFFFFFFFu || !out) return kBad;
    launch_max_len(lens, (uint32_t)n, out, 0);
    return finish();
}

}  // extern "C"
