// devtest.hip - test-only kernels around the device helpers of biokanga_amd/csrc (bk_dev_sets.h, bk_dev_window.h, bk_dev_trim.h, and the search
// primitives of bk_dev_util.h and bk_dev_k2.h), included as they stand.  Built as biokanga_amd/lib/libbk_devtest.so (csrc/Makefile); tests/helpers.py devtest_lib() loads it.  Every launcher takes raw
// device pointers, launches on the null stream, synchronises and returns the hipError_t.  The helpers' probe loops end only at a free
// slot: the caller keeps an LDS set within kLdsSetFill keys and an HBM table at most half full (tombstones counted), epochs in
// [1, kTombBit).
#include "../../biokanga_amd/csrc/bk_dev_sets.h"
#include "../../biokanga_amd/csrc/bk_dev_window.h"
#include "../../biokanga_amd/csrc/bk_dev_trim.h"
#include "../../biokanga_amd/csrc/bk_dev_k2.h"
#include "dev_search_eval.h"

using namespace bk;

namespace {

constexpr uint8_t kLook = 1, kInsert = 2;                                      // lset rounds: flag bits of a lane
constexpr uint8_t kOpContains = 1, kOpInsert = 2, kOpFind = 3, kOpFindRetract = 4;   // htab rounds: what a lane does

__global__ void __launch_bounds__(64) k_lset_bucket(const uint32_t *__restrict__ keys, uint32_t n, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = lset_bucket(keys[i]);
}

// k_wave's order: every lane looks up, wave barrier, every lane inserts, wave barrier
__global__ void __launch_bounds__(64) k_lset_rounds(const uint32_t *__restrict__ keys, const uint8_t *__restrict__ flags, uint32_t rounds,
                                                    uint8_t *__restrict__ found, uint32_t *__restrict__ set_out)
{
    __shared__ __attribute__((aligned(16))) uint32_t lset[kLdsSet];
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < kLdsSet; i += 64) lset[i] = kLdsEmpty;
    __builtin_amdgcn_wave_barrier();
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t key = keys[r * 64 + lane];
        const uint8_t f = flags[r * 64 + lane];
        found[r * 64 + lane] = (f & kLook) ? (lset_contains(lset, key) ? 1 : 0) : 0;
        __builtin_amdgcn_wave_barrier();
        if (f & kInsert) lset_insert(lset, key);
        __builtin_amdgcn_wave_barrier();
    }
    for (uint32_t i = lane; i < kLdsSet; i += 64) set_out[i] = lset[i];
}

// one wave per block, block b on its own table slice (tab + b * tab_size) with its own rounds, as wave_slot in k_wave / k_heavy.
// A round: contains / find_or_insert of every lane, wave barrier, insert / retract of every lane, wave barrier
__global__ void __launch_bounds__(64) k_htab_rounds(unsigned long long *__restrict__ tabs, uint32_t tab_size, const uint32_t *__restrict__ keys,
                                                    const uint8_t *__restrict__ ops, const uint32_t *__restrict__ epochs, uint32_t rounds,
                                                    uint8_t *__restrict__ out)
{
    unsigned long long *tab = tabs + (uint64_t)blockIdx.x * tab_size;
    const uint32_t mask = tab_size - 1, lane = threadIdx.x;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint64_t at = ((uint64_t)blockIdx.x * rounds + r) * 64 + lane;
        const uint32_t key = keys[at], epoch = epochs[(uint64_t)blockIdx.x * rounds + r];
        const uint8_t op = ops[at];
        uint32_t slot = 0xFFFFFFFFu;
        bool res = false;
        if (op == kOpContains) res = htab_contains(tab, mask, epoch, key);
        else if (op == kOpFind || op == kOpFindRetract) res = htab_find_or_insert(tab, mask, epoch, key, slot);
        out[at] = res ? 1 : 0;
        __builtin_amdgcn_wave_barrier();
        if (op == kOpInsert) htab_insert(tab, mask, epoch, key);
        else if (op == kOpFindRetract && slot != 0xFFFFFFFFu) htab_retract(tab, slot, epoch);
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ void __launch_bounds__(64) k_same_key(const uint32_t *__restrict__ keys, const uint8_t *__restrict__ cand, uint32_t rounds,
                                                 uint8_t *__restrict__ out)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t r = 0; r < rounds; r++)
        out[r * 64 + lane] = same_key_earlier_in_round(cand[r * 64 + lane] != 0, keys[r * 64 + lane], (int)lane) ? 1 : 0;
}

// one candidate per lane: rows r2w[n][NW / 2], rni[n][NW / 4]; results im[n][NW / 4], mm[n], eos[n]
template <int NW, bool WIDE>
__global__ void __launch_bounds__(64) k_window2i(const uint64_t *__restrict__ r2w_all, const uint64_t *__restrict__ rni_all, const int *__restrict__ len,
                                                 const uint64_t *__restrict__ t, const uint64_t *__restrict__ tgt2, const uint64_t *__restrict__ tgt2s, uint32_t n,
                                                 uint64_t *__restrict__ im, int *__restrict__ mm, uint8_t *__restrict__ eos)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint64_t r2w[NW / 2], rni[NW / 4];
    load_read_words2<NW>(r2w_all + (uint64_t)i * (NW / 2), r2w);
#pragma unroll
    for (int k = 0; k < NW / 4; k++) rni[k] = rni_all[(uint64_t)i * (NW / 4) + k];
    IWindow<NW> w;
    eval_window2i<NW, WIDE>(r2w, rni, len[i], tgt2, tgt2s, t[i], w);
#pragma unroll
    for (int k = 0; k < NW / 4; k++) im[(uint64_t)i * (NW / 4) + k] = w.im[k];
    mm[i] = w.mm;
    eos[i] = w.eos ? 1 : 0;
}

// rows[n][row_words]: 4 bit/base words (four) or 2 bit/base words; results: the Window (bm, mm, eos) and window_to_iwindow of it (im)
template <int NW>
__global__ void __launch_bounds__(64) k_window_rare(const uint64_t *__restrict__ rows, uint32_t row_words, int four, const int *__restrict__ len,
                                                    const uint64_t *__restrict__ t, const uint64_t *__restrict__ tgt4, uint32_t n,
                                                    uint64_t *__restrict__ bm, uint64_t *__restrict__ im, int *__restrict__ mm, uint8_t *__restrict__ eos)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    RdRow row;
    row.p = rows + (uint64_t)i * row_words;
    row.four = four != 0;
    Window<NW> w4;
    eval_window_rare<NW>(row, len[i], tgt4, t[i], w4);
    IWindow<NW> w;
    window_to_iwindow<NW>(w4, w);
#pragma unroll
    for (int k = 0; k < NW / 4; k++) { bm[(uint64_t)i * (NW / 4) + k] = w4.bm[k]; im[(uint64_t)i * (NW / 4) + k] = w.im[k]; }
    mm[i] = (w.mm == w4.mm && w.eos == w4.eos) ? w.mm : -1;
    eos[i] = w4.eos ? 1 : 0;
}

// one candidate per lane, every lane with its own length and parameters (the run loops diverge inside a wave, as in k_heavy):
// rows[n][row_words] 4 bit/base words
template <int ATW>
__global__ void __launch_bounds__(64) k_adaptive_trim(const uint64_t *__restrict__ rows, uint32_t row_words, const int *__restrict__ len,
                                                      const uint64_t *__restrict__ t, const uint64_t *__restrict__ tgt4, const int *__restrict__ min_trim,
                                                      const int *__restrict__ max_mm, const int *__restrict__ min_flank, uint32_t n, int *__restrict__ out_len,
                                                      int *__restrict__ out_mm, int *__restrict__ out_t5, int *__restrict__ out_t3)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    int mm, t5, t3;
    out_len[i] = adaptive_trim_dev<ATW>(rows + (uint64_t)i * row_words, tgt4, t[i], len[i], min_trim[i], max_mm[i], min_flank[i], mm, t5, t3);
    out_mm[i] = mm; out_t5[i] = t5; out_t3[i] = t3;
}

// pe_window_key<ATW> of one candidate window per lane; ATW == 0: pe_window_ok's own result and mismatch count as well
template <int ATW>
__global__ void __launch_bounds__(64) k_pe_window(const uint64_t *__restrict__ rows, uint32_t row_words, const int *__restrict__ len,
                                                  const uint64_t *__restrict__ t, const uint64_t *__restrict__ tgt4, const int *__restrict__ max_mm,
                                                  const int *__restrict__ min_put, const unsigned long long *__restrict__ order, uint32_t n,
                                                  unsigned long long *__restrict__ key_out, int *__restrict__ out_t5, int *__restrict__ out_t3,
                                                  uint8_t *__restrict__ ok_out, int *__restrict__ mm_out)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint64_t *rdw = rows + (uint64_t)i * row_words;
    int t5, t3;
    key_out[i] = pe_window_key<ATW>(rdw, len[i], tgt4, t[i], max_mm[i], min_put[i], order[i], t5, t3);
    out_t5[i] = t5; out_t3[i] = t3;
    if constexpr (ATW == 0) {
        int mm;
        ok_out[i] = pe_window_ok(rdw, len[i], tgt4, t[i], max_mm[i], mm) ? 1 : 0;
        mm_out[i] = mm;
    }
}

// the search primitives (tests/test_gpu_dev_search.py): one case per lane - dev_search_eval.h turns a case into the call of the function under
// test, the same text the CPU twin runs - neighbouring lanes with other functions, lengths, offsets and caps, so the loops diverge inside a wave
__global__ void __launch_bounds__(64) k_search_bits(bkt::CtxA x, const bkt::Case *__restrict__ cs, uint32_t n, bkt::Res *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = bkt::eval_a(x, cs[i]);
}
__global__ void __launch_bounds__(64) k_search_cmp(bkt::CtxB x, const bkt::Case *__restrict__ cs, uint32_t n, bkt::Res *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = bkt::eval_b(x, cs[i]);
}
__global__ void __launch_bounds__(64) k_search_ktab(bkt::CtxC x, const bkt::Case *__restrict__ cs, uint32_t n, bkt::Res *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = bkt::eval_c(x, cs[i]);
}
__global__ void __launch_bounds__(64) k_search_core(bkt::CtxD x, const bkt::Case *__restrict__ cs, uint32_t n, bkt::Res *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = bkt::eval_d(x, cs[i]);
}
__global__ void __launch_bounds__(64) k_search_k2(bkt::CtxE x, const bkt::Case *__restrict__ cs, uint32_t n, bkt::Res *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = bkt::eval_e(x, cs[i]);
}
// the entry table goes to LDS as in the kernels that look entries up (every lane of the block reaches lds_entries_load's barrier)
__global__ void __launch_bounds__(64) k_find_entry(bkt::CtxF x, const bkt::Case *__restrict__ cs, uint32_t n, bkt::Res *__restrict__ out)
{
    __shared__ LdsEntries le;
    lds_entries_load(le, x.ix);
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) out[i] = bkt::eval_f(x, le, cs[i], i);
}

int finish()
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return (int)e;
}

}  // namespace

extern "C" {

// {kLdsSet, kLdsSetFill, kLdsEmpty, kTombBit}: the caps and special values the tests stay within
void bkdt_consts(uint32_t *out4)
{
    out4[0] = kLdsSet; out4[1] = kLdsSetFill; out4[2] = kLdsEmpty; out4[3] = kTombBit;
}

int bkdt_lset_bucket(const uint32_t *keys, uint32_t n, uint32_t *out)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_lset_bucket, dim3((n + 63) / 64), dim3(64), 0, 0, keys, n, out);
    return finish();
}

// keys, flags (bit 0 look up, bit 1 insert), found: rounds * 64; set_out: kLdsSet words
int bkdt_lset_rounds(const uint32_t *keys, const uint8_t *flags, uint32_t rounds, uint8_t *found, uint32_t *set_out)
{
    hipLaunchKernelGGL(k_lset_rounds, dim3(1), dim3(64), 0, 0, keys, flags, rounds, found, set_out);
    return finish();
}

// tabs: blocks * tab_size entries (tab_size a power of two); keys, ops (1 contains, 2 insert, 3 find_or_insert, 4 find_or_insert and
// retract the slot it took), out: blocks * rounds * 64; epochs: blocks * rounds
int bkdt_htab_rounds(unsigned long long *tabs, uint32_t tab_size, uint32_t blocks, const uint32_t *keys, const uint8_t *ops, const uint32_t *epochs,
                     uint32_t rounds, uint8_t *out)
{
    if (blocks == 0 || tab_size == 0 || (tab_size & (tab_size - 1))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_htab_rounds, dim3(blocks), dim3(64), 0, 0, tabs, tab_size, keys, ops, epochs, rounds, out);
    return finish();
}

int bkdt_same_key(const uint32_t *keys, const uint8_t *cand, uint32_t rounds, uint8_t *out)
{
    hipLaunchKernelGGL(k_same_key, dim3(1), dim3(64), 0, 0, keys, cand, rounds, out);
    return finish();
}

int bkdt_window2i(int nw, int wide, const uint64_t *r2w, const uint64_t *rni, const int *len, const uint64_t *t, const uint64_t *tgt2, const uint64_t *tgt2s,
                  uint32_t n, uint64_t *im, int *mm, uint8_t *eos)
{
    if (n == 0) return 0;
    const dim3 grid((n + 63) / 64), block(64);
    if (nw == 8 && !wide) hipLaunchKernelGGL((k_window2i<8, false>), grid, block, 0, 0, r2w, rni, len, t, tgt2, tgt2s, n, im, mm, eos);
    else if (nw == 8) hipLaunchKernelGGL((k_window2i<8, true>), grid, block, 0, 0, r2w, rni, len, t, tgt2, tgt2s, n, im, mm, eos);
    else if (nw == 16 && !wide) hipLaunchKernelGGL((k_window2i<16, false>), grid, block, 0, 0, r2w, rni, len, t, tgt2, tgt2s, n, im, mm, eos);
    else if (nw == 16) hipLaunchKernelGGL((k_window2i<16, true>), grid, block, 0, 0, r2w, rni, len, t, tgt2, tgt2s, n, im, mm, eos);
    else return (int)hipErrorInvalidValue;
    return finish();
}

int bkdt_window_rare(int nw, const uint64_t *rows, uint32_t row_words, int four, const int *len, const uint64_t *t, const uint64_t *tgt4, uint32_t n,
                     uint64_t *bm, uint64_t *im, int *mm, uint8_t *eos)
{
    if (n == 0) return 0;
    const dim3 grid((n + 63) / 64), block(64);
    if (nw == 8) hipLaunchKernelGGL((k_window_rare<8>), grid, block, 0, 0, rows, row_words, four, len, t, tgt4, n, bm, im, mm, eos);
    else if (nw == 16) hipLaunchKernelGGL((k_window_rare<16>), grid, block, 0, 0, rows, row_words, four, len, t, tgt4, n, bm, im, mm, eos);
    else return (int)hipErrorInvalidValue;
    return finish();
}

// rows: n rows of row_words 4 bit/base words, row_words >= 4 atw + 1 (a read of 64 atw bases and the word nib16 loads behind it); tgt4 is
// followed by a word of padding as well.  atw = 8 or 32 (the instantiations of k_heavy)
int bkdt_adaptive_trim(int atw, const uint64_t *rows, uint32_t row_words, const int *len, const uint64_t *t, const uint64_t *tgt4, const int *min_trim,
                       const int *max_mm, const int *min_flank, uint32_t n, int *out_len, int *out_mm, int *out_t5, int *out_t3)
{
    if ((atw != 8 && atw != 32) || row_words < 4u * (uint32_t)atw + 1) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const dim3 grid((n + 63) / 64), block(64);
    if (atw == 8) hipLaunchKernelGGL((k_adaptive_trim<8>), grid, block, 0, 0, rows, row_words, len, t, tgt4, min_trim, max_mm, min_flank, n, out_len, out_mm, out_t5, out_t3);
    else hipLaunchKernelGGL((k_adaptive_trim<32>), grid, block, 0, 0, rows, row_words, len, t, tgt4, min_trim, max_mm, min_flank, n, out_len, out_mm, out_t5, out_t3);
    return finish();
}

// the inputs of bkdt_adaptive_trim that pe_window_key takes (its flanks are 3, min_put is its min_trim) and the window's scan order.
// atw = 0 (the read whole: pe_window_ok, whose result and mismatch count go to ok_out / mm_out - left alone otherwise), 8 or 32.
// pe_window_ok reads the whole row before it looks at the length: with atw = 0 every len must be at most 16 (row_words - 1)
int bkdt_pe_window(int atw, const uint64_t *rows, uint32_t row_words, const int *len, const uint64_t *t, const uint64_t *tgt4, const int *max_mm, uint32_t n,
                   const int *min_put, const unsigned long long *order, unsigned long long *key_out, int *t5, int *t3, uint8_t *ok_out, int *mm_out)
{
    if ((atw != 0 && atw != 8 && atw != 32) || row_words < 4u * (uint32_t)atw + 1 || row_words < 2) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    const dim3 grid((n + 63) / 64), block(64);
    if (atw == 0) hipLaunchKernelGGL((k_pe_window<0>), grid, block, 0, 0, rows, row_words, len, t, tgt4, max_mm, min_put, order, n, key_out, t5, t3, ok_out, mm_out);
    else if (atw == 8) hipLaunchKernelGGL((k_pe_window<8>), grid, block, 0, 0, rows, row_words, len, t, tgt4, max_mm, min_put, order, n, key_out, t5, t3, ok_out, mm_out);
    else hipLaunchKernelGGL((k_pe_window<32>), grid, block, 0, 0, rows, row_words, len, t, tgt4, max_mm, min_put, order, n, key_out, t5, t3, ok_out, mm_out);
    return finish();
}

// ---- the search primitives.  cases: n records of bkt::Case, out: n of bkt::Res (dev_search_eval.h says what a case's fields mean per group).
// Every array is as long as the CPU twin's (tests/cpp/dev_search_host.cpp `dump`), its padding words included.
int bkdt_search_bits(const uint64_t *w, const uint64_t *rd4, const uint64_t *rd2, const void *cases, uint32_t n, void *out)
{
    if (n == 0) return 0;
    const bkt::CtxA x{w, rd4, rd2};
    hipLaunchKernelGGL(k_search_bits, dim3((n + 63) / 64), dim3(64), 0, 0, x, (const bkt::Case *)cases, n, (bkt::Res *)out);
    return finish();
}

int bkdt_search_cmp(const uint64_t *rd4, const uint64_t *rd2, const uint64_t *tgt4, const void *cases, uint32_t n, void *out)
{
    if (n == 0) return 0;
    const bkt::CtxB x{rd4, rd2, tgt4};
    hipLaunchKernelGGL(k_search_cmp, dim3((n + 63) / 64), dim3(64), 0, 0, x, (const bkt::Case *)cases, n, (bkt::Res *)out);
    return finish();
}

// one table of order k (4^k + 1 entries) in its four forms - 32-bit starts, 64-bit starts, ktab_hi + offsets, {start, anything} pairs - each
// under a DevIndex of its own with everything else zero, and the index without a table
int bkdt_search_ktab(const uint32_t *tab32, const uint64_t *tab64, const uint64_t *pk_hi, const uint32_t *pk_lo, const void *tab2, const uint32_t *sa_lo,
                     const uint8_t *sa_hi, uint64_t n_index, int k, const void *cases, uint32_t n, void *out)
{
    if (n == 0) return 0;
    bkt::CtxC x;
    bkt::index_views(x, tab32, tab64, pk_hi, pk_lo, (const uint2 *)tab2, sa_lo, sa_hi, n_index, k);
    hipLaunchKernelGGL(k_search_ktab, dim3((n + 63) / 64), dim3(64), 0, 0, x, (const bkt::Case *)cases, n, (bkt::Res *)out);
    return finish();
}

// tgt4 is followed by sequence-end words; tab32 or tab64 (or neither, k = 0)
int bkdt_search_core(const uint64_t *tgt4, const uint32_t *sa_lo, const uint8_t *sa_hi, const uint32_t *tab32, const uint64_t *tab64, uint64_t n_index, int k,
                     const uint64_t *rd4, const uint64_t *rd2, const void *cases, uint32_t n, void *out)
{
    if (n == 0) return 0;
    bkt::CtxD x;
    bkt::index_search(x, tgt4, sa_lo, sa_hi, tab32, tab64, n_index, k, rd4, rd2);
    hipLaunchKernelGGL(k_search_core, dim3((n + 63) / 64), dim3(64), 0, 0, x, (const bkt::Case *)cases, n, (bkt::Res *)out);
    return finish();
}

// k2: the n_keys keys and their sampled levels, k2s_start(n_keys, kK2Levels + 1) words
int bkdt_search_k2(const uint64_t *tgt4, const uint32_t *k2, uint64_t n_keys, const void *cases, uint32_t n, void *out)
{
    if (n == 0) return 0;
    bkt::CtxE x;
    bkt::k2_ctx(x, tgt4, k2, n_keys);
    hipLaunchKernelGGL(k_search_k2, dim3((n + 63) / 64), dim3(64), 0, 0, x, (const bkt::Case *)cases, n, (bkt::Res *)out);
    return finish();
}

// hits: n records of bk_hit, where write_result puts case i's record
int bkdt_search_entries(const uint64_t *ent_start, const uint64_t *ent_end, const uint32_t *ent_id, uint32_t n_ent, void *hits, const void *cases, uint32_t n,
                        void *out)
{
    if (n == 0) return 0;
    bkt::CtxF x;
    bkt::index_entries(x, ent_start, ent_end, ent_id, n_ent, (bk_hit *)hits);
    hipLaunchKernelGGL(k_find_entry, dim3((n + 63) / 64), dim3(64), 0, 0, x, (const bkt::Case *)cases, n, (bkt::Res *)out);
    return finish();
}

// {kK2Levels, words of a key array of n keys with its levels}
void bkdt_k2_layout(uint64_t n, uint64_t *out2)
{
    out2[0] = kK2Levels; out2[1] = k2s_start(n, kK2Levels + 1);
}

}  // extern "C"
