// bk_contam.hip - contaminant (adaptor) overlaps of raw reads, `biokanga align -H` (CContaminants::MatchContaminants, libbiokanga/Contaminants.cpp:1227-1309,
// as CAligner::LoadRawReads calls it, biokanga/Aligner.cpp:11036-11076).  The reference walks a trie once per overlap length per read end; its
// outcome is a closed form, and that is what runs here:
//   for a read of 20..2000 bases and a use type (5' PE1, 5' PE2, 3' PE1, 3' PE2) with entries, the LARGEST L, trim + 1 <= L <= min(read, longest
//   entry), for which an entry of at least L bases has at most ONE mismatching position between the read's first L bases and the entry's last L
//   (5') or the read's last L and the entry's first L (3'); a position mismatches when the read's base is N, or the entry's base is not N and
//   differs.  Reported: L - trim (0 without such an L).
// One wave per read.  The wave packs the at most 200 bases of either read end that can overlap anything into LDS at 2 bit/base (plus a mask of
// the N and one of the other non-a,c,g,t bases), the entries are held the same way, and a (overlap length, entry) pair is XOR / popcount over
// 64-bit words of 32 bases with an exit at the second mismatch: a clean read fails almost every pair in its first word.  The pairs are dealt to
// the lanes longest overlap first, so the lowest lane of a ballot holds the answer.
// The set lives in LDS while it fits kContamLdsBudget (32 KB: 238 entries - every adaptor file in practice - and four blocks of 256 threads still
// share a CU's 160 KB); a larger one, up to the reference's 1600 entries of 200 bases (211 KB), is read through the caches.
// gfx950 build: 48 VGPRs with the set in LDS, 52 without, no scratch, 3456 bytes of LDS + the set; 8 waves per SIMD by registers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "../../include/biokanga_amd.h"
#include "bk_cpus.h"
#include "bk_devbuf.h"

namespace {

typedef unsigned long long u64;

constexpr int kMaxEntryLen = 200, kMinEntryLen = 4, kMaxEntries = 1600, kMinReadLen = 20, kMaxReadLen = 2000;
constexpr int kEntryWords = 16;                        // 8 words of 32 bases (200 bases + a word the funnel shift may touch), 8 of their N mask
constexpr int kWaves = 4;                              // per block
constexpr u64 kLow = 0x5555555555555555ull;            // the low bit of every base's pair: where the masks keep their flag
constexpr uint32_t kContamLdsBudget = 32u << 10;
// one chunk in flight per slot: at most this much of the reads on the device at a time
constexpr uint64_t kChunkBases = 64ull << 20;
constexpr uint32_t kChunkReads = 1u << 20;
constexpr int kSlots = 2;

// the set as the device sees it: header, lengths, then kEntryWords words per entry; entries of a type lie together, longest first
struct SetHdr {
    uint32_t n[4], first[4], maxlen[4], n_total, lens_at, words_at, bytes;      // (offsets in bytes from the header's start)
    uint16_t cnt[4][kMaxEntryLen + 8];                 // cnt[t][L]: entries of type t with at least L bases - a prefix of the type's list
};

// 32 bases from base `off` on of a packed array (the word behind the last one holding bases must exist)
template <class P>
__device__ __forceinline__ u64 fetch32(P w, int off)
{
    const int k = off >> 5, s = (off & 31) * 2;
    const u64 lo = w[k] >> s;
    return s ? (lo | (w[k + 1] << (64 - s))) : lo;
}

// At most one mismatch over L bases?  `five`: the read window's first L against the entry's last L, else the window's last L (the window
// ends where the read ends) against the entry's first L.
template <class P, class Q>
__device__ __forceinline__ bool overlaps(bool five, int L, int elen, int win, P ebits, P emask, Q rbits, Q rn, Q ro)
{
    const int eoff = five ? elen - L : 0, roff = five ? 0 : win - L;
    int mism = 0;
    for (int at = 0; at < L; at += 32) {
        const u64 c = fetch32(ebits, eoff + at), cn = fetch32(emask, eoff + at);
        const u64 r = fetch32(rbits, roff + at), n = fetch32(rn, roff + at), o = fetch32(ro, roff + at);
        const u64 x = r ^ c, d = (x | (x >> 1)) & kLow;
        u64 m = n | (~cn & (o | d) & kLow);
        const int left = L - at;
        if (left < 32) m &= (1ull << (2 * left)) - 1;
        mism += __popcll(m);
        if (mism > 1) return false;
    }
    return true;
}

// The largest accepted overlap of one read end, by the whole wave (every lane returns it).
template <class P, class Q>
__device__ __forceinline__ int best_overlap(bool five, int type, int min_overlap, int win, const SetHdr *h, const uint16_t *elens, P ewords, Q rbits,
                                            Q rn, Q ro, int lane)
{
    const int nt = (int)h->n[type];
    if (nt == 0 || win < min_overlap) return 0;
    int G = 1;
    while (G < nt && G < 64) G <<= 1;                  // lanes per overlap length
    const int rows = 64 / G, row = lane / G, col = lane % G;
    const int first = (int)h->first[type];
    for (int top = win; top >= min_overlap; top -= rows) {
        const int L = top - row;
        bool hit = false;
        if (L >= min_overlap) {
            const int live = (int)h->cnt[type][L];
            for (int e = col; e < live && !hit; e += G) {
                P w = ewords + (size_t)(first + e) * kEntryWords;
                hit = overlaps(five, L, (int)elens[first + e], win, w, w + 8, rbits, rn, ro);
            }
        }
        const u64 b = __ballot(hit);
        if (b) return top - (__ffsll((long long)b) - 1) / G;
    }
    return 0;
}

template <bool kSetInLds>
__global__ void __launch_bounds__(64 * kWaves)
k_contam(const uint8_t *__restrict__ bases, const uint32_t *__restrict__ offs, const uint32_t *__restrict__ lens, const uint8_t *__restrict__ pe2,
         int pe2_all, uint32_t nreads, int trim5, int trim3, const SetHdr *__restrict__ set, uint16_t *__restrict__ out)
{
    extern __shared__ u64 lds_set[];                   // the set (kSetInLds), as the host laid it out
    __shared__ u64 win[kWaves][2][3][9];               // per wave, per end: bits, N mask, other-base mask; 256 bases + the funnel shift's word
    __shared__ SetHdr hdr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        const uint32_t *src = (const uint32_t *)set;
        uint32_t *dst = (uint32_t *)&hdr;
        for (uint32_t i = threadIdx.x; i < sizeof(SetHdr) / 4; i += blockDim.x) dst[i] = src[i];
        if (kSetInLds) {
            const u64 *s8 = (const u64 *)set;
            const uint32_t n8 = set->bytes / 8;
            for (uint32_t i = threadIdx.x; i < n8; i += blockDim.x) lds_set[i] = s8[i];
        }
    }
    __syncthreads();
    const uint16_t *elens_g = (const uint16_t *)((const char *)set + hdr.lens_at);
    const u64 *ewords_g = (const u64 *)((const char *)set + hdr.words_at);
    const uint16_t *elens_l = (const uint16_t *)((const char *)lds_set + hdr.lens_at);
    const u64 *ewords_l = (const u64 *)((const char *)lds_set + hdr.words_at);
    if (lane == 0)
        for (int e = 0; e < 2; e++)
            for (int a = 0; a < 3; a++) win[wave][e][a][8] = 0;
    for (uint32_t r = blockIdx.x * kWaves + wave; r < nreads; r += gridDim.x * kWaves) {
        const int n = (int)lens[r];
        int res5 = 0, res3 = 0;
        if (n >= kMinReadLen && n <= kMaxReadLen) {
            const int second = pe2 ? (pe2[r] != 0) : pe2_all;
            const int t5 = second ? 1 : 0, t3 = second ? 3 : 2;
            const int w5 = min(n, (int)hdr.maxlen[t5]), w3 = min(n, (int)hdr.maxlen[t3]);
            const uint8_t *rd = bases + offs[r];
            // lane j packs window bases 4j .. 4j+3 of either end into one byte of each array (bytes of a little-endian word)
            for (int e = 0; e < 2; e++) {
                const int w = e ? w3 : w5, from = e ? n - w3 : 0;
                uint32_t bits = 0, nm = 0, om = 0;
                for (int k = 0; k < 4; k++) {
                    const int i = 4 * lane + k;
                    if (i < w) {
                        const uint32_t b = rd[from + i] & 7u;
                        bits |= (b & 3u) << (2 * k);
                        nm |= (uint32_t)(b == 4u) << (2 * k);
                        om |= (uint32_t)(b > 4u) << (2 * k);
                    }
                }
                ((uint8_t *)win[wave][e][0])[lane] = (uint8_t)bits;
                ((uint8_t *)win[wave][e][1])[lane] = (uint8_t)nm;
                ((uint8_t *)win[wave][e][2])[lane] = (uint8_t)om;
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const u64 *b5 = win[wave][0][0], *n5 = win[wave][0][1], *o5 = win[wave][0][2];
            const u64 *b3 = win[wave][1][0], *n3 = win[wave][1][1], *o3 = win[wave][1][2];
            int L5, L3;
            if (kSetInLds) {
                L5 = best_overlap(true, t5, trim5 + 1, w5, &hdr, elens_l, ewords_l, b5, n5, o5, lane);
                L3 = best_overlap(false, t3, trim3 + 1, w3, &hdr, elens_l, ewords_l, b3, n3, o3, lane);
            } else {
                L5 = best_overlap(true, t5, trim5 + 1, w5, &hdr, elens_g, ewords_g, b5, n5, o5, lane);
                L3 = best_overlap(false, t3, trim3 + 1, w3, &hdr, elens_g, ewords_g, b3, n3, o3, lane);
            }
            res5 = L5 > trim5 ? L5 - trim5 : 0;
            res3 = L3 > trim3 ? L3 - trim3 : 0;
            __builtin_amdgcn_wave_barrier();           // (the windows are rewritten for the wave's next read)
        }
        if (lane == 0) { out[2 * (size_t)r] = (uint16_t)res5; out[2 * (size_t)r + 1] = (uint16_t)res3; }
    }
}

struct Slot {
    bk::PinBuf<uint8_t> h_bases, h_pe2;
    bk::PinBuf<uint32_t> h_offs, h_lens;
    bk::PinBuf<uint16_t> h_out;                        // two per read
    bk::DevBuf<uint8_t> d_bases, d_pe2;
    bk::DevBuf<uint32_t> d_offs, d_lens;
    bk::DevBuf<uint16_t> d_out;
    hipEvent_t done = nullptr;
    uint64_t first = 0;                                // the chunk in flight: reads [first, first + n)
    uint32_t n = 0;
};

}  // namespace

struct bk_contam {
    int device = 0;
    hipStream_t stream = nullptr;
    bk::DevBuf<uint8_t> d_set;
    uint32_t set_bytes = 0;
    bool in_lds = false;
    int blocks = 0;
    Slot slot[kSlots];
    bool have_slots = false;
};

namespace {

void free_all(bk_contam *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (Slot &s : c->slot)
        if (s.done) (void)hipEventDestroy(s.done);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                          // (the buffers go with their owners, while the device is current)
}

// the staging and device buffers of the chunks, made at the first match call: kSlots x (64 MB of bases + 13 bytes per read of 2^20) on either side
bool make_slots(bk_contam *c)
{
    if (c->have_slots) return true;
    for (Slot &s : c->slot) {
        // (the first failure ends it; a later call finds what was made and goes on from there)
        if (s.h_bases.ensure(kChunkBases) || s.h_pe2.ensure(kChunkReads) || s.h_offs.ensure(kChunkReads) || s.h_lens.ensure(kChunkReads) || s.h_out.ensure(2ull * kChunkReads) ||
            s.d_bases.ensure(kChunkBases) || s.d_pe2.ensure(kChunkReads) || s.d_offs.ensure(kChunkReads) || s.d_lens.ensure(kChunkReads) || s.d_out.ensure(2ull * kChunkReads))
            return false;
        if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) return false;
    }
    c->have_slots = true;
    return true;
}

template <class Fn>
void par(size_t n, int nthreads, Fn fn)
{
    const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)nthreads, n / 16384));
    if (nt <= 1) { fn((size_t)0, n); return; }
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; t++) th.emplace_back([&fn, n, nt, t]() { fn(n * t / nt, n * (t + 1) / nt); });
    fn((size_t)0, n / nt);
    for (auto &x : th) x.join();
}

}  // namespace

extern "C" int bk_contam_create(bk_contam **out, int device_id, const bk_contam_entry *entries, uint32_t n_entries)
{
    if (!out) return BK_ERR_PARAMS;
    *out = nullptr;
    if (!entries || n_entries < 1 || n_entries > (uint32_t)kMaxEntries || device_id < 0) return BK_ERR_PARAMS;
    for (uint32_t i = 0; i < n_entries; i++) {
        const bk_contam_entry &e = entries[i];
        if (!e.bases || e.len < (uint32_t)kMinEntryLen || e.len > (uint32_t)kMaxEntryLen || e.use < 1 || e.use > 4) return BK_ERR_PARAMS;
        for (uint32_t k = 0; k < e.len; k++)
            if (e.bases[k] > 4) return BK_ERR_PARAMS;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return BK_ERR_NODEVICE;
    if (device_id >= ndev) return BK_ERR_PARAMS;
    // the image: entries of a type together, longest first (a stable order: nothing reports which entry matched)
    std::vector<uint32_t> order(n_entries);
    for (uint32_t i = 0; i < n_entries; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (entries[a].use != entries[b].use) return entries[a].use < entries[b].use;
        return entries[a].len > entries[b].len;
    });
    const uint32_t lens_at = (uint32_t)sizeof(SetHdr), words_at = (lens_at + 2 * n_entries + 7) & ~7u;
    const uint32_t bytes = words_at + n_entries * kEntryWords * 8;
    std::vector<u64> img((bytes + 7) / 8, 0);
    SetHdr *h = (SetHdr *)img.data();
    uint16_t *elens = (uint16_t *)((char *)img.data() + lens_at);
    u64 *words = (u64 *)((char *)img.data() + words_at);
    h->n_total = n_entries; h->lens_at = lens_at; h->words_at = words_at; h->bytes = bytes;
    for (uint32_t k = 0; k < n_entries; k++) {
        const bk_contam_entry &e = entries[order[k]];
        const int t = (int)e.use - 1;
        if (h->n[t]++ == 0) { h->first[t] = k; h->maxlen[t] = e.len; }
        for (uint32_t L = 1; L <= e.len; L++) h->cnt[t][L]++;
        elens[k] = (uint16_t)e.len;
        u64 *w = words + (size_t)k * kEntryWords;
        for (uint32_t i = 0; i < e.len; i++) {
            const u64 b = e.bases[i];
            w[i >> 5] |= (b & 3) << (2 * (i & 31));
            if (b == 4) w[8 + (i >> 5)] |= 1ull << (2 * (i & 31));
        }
    }
    bk_contam *c = new (std::nothrow) bk_contam;
    if (!c) return BK_ERR_MEM;
    c->device = device_id;
    c->set_bytes = bytes;
    c->in_lds = bytes <= kContamLdsBudget;
    hipDeviceProp_t prop;
    if (hipSetDevice(device_id) != hipSuccess || hipGetDeviceProperties(&prop, device_id) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || c->d_set.ensure(img.size() * 8) != hipSuccess ||
        hipMemcpy(c->d_set.get(), img.data(), img.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
        free_all(c);
        return BK_ERR_MEM;
    }
    c->blocks = std::max(1, prop.multiProcessorCount) * 8;
    *out = c;
    return BK_OK;
}

extern "C" void bk_contam_destroy(bk_contam *c) { free_all(c); }

extern "C" int bk_contam_match(bk_contam *c, const uint8_t *bases, const uint64_t *offs, const uint32_t *lens, uint64_t nreads, const uint8_t *is_pe2,
                               int all_pe2, int trim5, int trim3, uint16_t *out)
{
    if (!c || trim5 < 0 || trim3 < 0 || trim5 > 0xffff || trim3 > 0xffff || (all_pe2 != 0 && all_pe2 != 1)) return BK_ERR_PARAMS;
    if (nreads == 0) return BK_OK;
    if (!bases || !lens || !out) return BK_ERR_PARAMS;
    if (hipSetDevice(c->device) != hipSuccess) return BK_ERR_NODEVICE;
    if (!make_slots(c)) return BK_ERR_MEM;
    const int nthreads = std::max(1, std::min(8, bk::effective_cpus()));
    auto collect = [&](Slot &s) -> int {               // the results of the slot's chunk, once it is through
        if (!s.n) return BK_OK;
        if (hipEventSynchronize(s.done) != hipSuccess) return BK_ERR_INTERNAL;
        memcpy(out + 2 * s.first, s.h_out.get(), 4ull * s.n);
        s.n = 0;
        return BK_OK;
    };
    int rc = BK_OK;
    uint64_t at = 0, src = 0;                          // next read; where it starts when the reads lie back to back (offs == NULL)
    for (int k = 0; at < nreads && rc == BK_OK; k ^= 1) {
        Slot &s = c->slot[k];
        if ((rc = collect(s)) != BK_OK) break;
        // the chunk: reads while they fit; only what can overlap anything travels - a read outside 20..2000 bases goes as length 0
        uint32_t n = 0;
        uint64_t nb = 0, src_first = src;
        while (at + n < nreads && n < kChunkReads) {
            const uint32_t len = lens[at + n];
            const uint32_t take = (len >= (uint32_t)kMinReadLen && len <= (uint32_t)kMaxReadLen) ? len : 0;
            if (nb + take > kChunkBases) break;
            s.h_offs.get()[n] = (uint32_t)nb;
            s.h_lens.get()[n] = take;
            nb += take;
            src += len;
            n++;
        }
        {
            // (the copy, by a few threads: each finds where its range of back-to-back reads starts)
            const uint64_t first = at;
            par(n, nthreads, [&](size_t lo, size_t hi) {
                uint64_t from = src_first;
                if (!offs) for (size_t i = 0; i < lo; i++) from += lens[first + i];
                for (size_t i = lo; i < hi; i++) {
                    const uint32_t len = lens[first + i];
                    if (s.h_lens.get()[i]) memcpy(s.h_bases.get() + s.h_offs.get()[i], bases + (offs ? offs[first + i] : from), len);
                    from += len;
                    s.h_pe2.get()[i] = is_pe2 ? (uint8_t)(is_pe2[first + i] != 0) : (uint8_t)all_pe2;
                }
            });
        }
        s.first = at;
        s.n = n;
        at += n;
        bool ok = (nb == 0 || hipMemcpyAsync(s.d_bases.get(), s.h_bases.get(), nb, hipMemcpyHostToDevice, c->stream) == hipSuccess) &&
                  hipMemcpyAsync(s.d_offs.get(), s.h_offs.get(), 4ull * n, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
                  hipMemcpyAsync(s.d_lens.get(), s.h_lens.get(), 4ull * n, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
                  hipMemcpyAsync(s.d_pe2.get(), s.h_pe2.get(), n, hipMemcpyHostToDevice, c->stream) == hipSuccess;
        if (ok) {
            const int blocks = (int)std::min<uint64_t>((uint64_t)c->blocks, (n + kWaves - 1) / kWaves);
            if (c->in_lds)
                hipLaunchKernelGGL(k_contam<true>, dim3(blocks), dim3(64 * kWaves), c->set_bytes, c->stream, s.d_bases.get(), s.d_offs.get(), s.d_lens.get(), s.d_pe2.get(), 0, n,
                                   trim5, trim3, (const SetHdr *)c->d_set.get(), s.d_out.get());
            else
                hipLaunchKernelGGL(k_contam<false>, dim3(blocks), dim3(64 * kWaves), 0, c->stream, s.d_bases.get(), s.d_offs.get(), s.d_lens.get(), s.d_pe2.get(), 0, n, trim5,
                                   trim3, (const SetHdr *)c->d_set.get(), s.d_out.get());
            ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(s.h_out.get(), s.d_out.get(), 4ull * n, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                 hipEventRecord(s.done, c->stream) == hipSuccess;
        }
        if (!ok) { s.n = 0; rc = BK_ERR_INTERNAL; }
    }
    for (Slot &s : c->slot) {
        const int r2 = collect(s);
        if (rc == BK_OK) rc = r2;
    }
    if (rc != BK_OK) (void)hipStreamSynchronize(c->stream);
    return rc;
}
