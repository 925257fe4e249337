// bk_samtags.h - NM:i and MD:Z of a SAM record, made by a wave (gfx950 only; shared by the formatter of bk_sam.hip and the request call of
// bk_samtags.hip).  The tags are a literal walk of the line as written: POS, the CIGAR [c5 S] m M [c3 S] [gap N|I|D m2 M] and SEQ against
// the sequence as indexed (DevIndex::tgt4, the nibble & 7: a c g t n).  S and I consume SEQ, N and D the target, M both; an M base matches
// when both letters are the same one of ACGT.  NM = mismatching M bases + I bases + D bases.  MD = the match runs (always written, 0 too)
// with the target's letter at a mismatch and ^letters at a deletion; N, I and S write nothing and do not end a run.
//
// A wave takes its (up to) 64 records in turn and its lanes a record's M bases 64 at a time: lane q loads read code and target code of
// base q, __ballot gives the mismatches (NM by popcount), every mismatching lane finds the mismatch before it in the mask - or in what the
// steps before carried over - which is its run, and a prefix sum over the lanes' piece lengths places its "<run><letter>".  The deletion's
// "<run>^letters" and the closing run go the same way.  Nothing is indexed at run time but memory.
#pragma once
#include "bk_device.h"

namespace bk {

constexpr uint32_t kTagNone = 0xFFFFu;              // NM of a record without tags: its walk is malformed (or NM itself would not fit 16 bits)
constexpr uint32_t kTagNoExc = 0xFFFFFFFFu;

// where the reads of the walks lie: a byte per base (code in the low three bits), or 16 bases per 32-bit word, first base in the top bits,
// with the bases that are not a,c,g,t listed as runs sorted by (read, pos)
struct TagReads {
    const uint8_t *bases;
    const uint32_t *pk_words;
    const bk_nbase *pk_exc;
    uint64_t n_pk_exc;
};

// one record's walk, as its lane holds it
struct TagWalk {
    uint64_t rd_at;                                 // the read's first base in `bases` / first word in `pk_words`
    uint64_t g0;                                    // the first M base in the concatenated target
    uint32_t rd, efirst;                            // packed reads: the read's number and its first exception run (kTagNoExc: none)
    uint32_t len_c5, m_c3, m2_op;                   // len | c5 << 16, m | c3 << 16, m2 | gop << 16 | reversed << 24
    uint32_t gap;
    uint32_t ok;                                    // 0: no walk (the lane has no record, or tag_walk_set refused it)
};

// The CIGAR numbers of a record against its read and its sequence: false when the walk is not well formed - a number <= 0, a walk that does
// not consume exactly SEQ, or one that leaves its sequence (pos: 0-based first M base, chrom_len: the sequence's length).  Fills w's
// geometry; rd_at, g0, rd, efirst are the caller's.
__device__ __forceinline__ bool tag_walk_set(TagWalk &w, uint64_t len, uint64_t c5, uint64_t m, uint64_t c3, uint32_t gop, long gap, uint64_t m2, bool rev,
                                             uint64_t pos, uint64_t chrom_len)
{
    w.ok = 0;
    if (!len || len > 0xffffu || !m || m > len || c5 > len || c3 > len) return false;
    uint64_t seq = c5 + m + c3, tgt = pos + m;
    if (gop) {
        if ((gop != 'N' && gop != 'I' && gop != 'D') || gap <= 0 || !m2 || m2 > len) return false;
        if (gop == 'I') { if ((uint64_t)gap > len) return false; seq += (uint64_t)gap; }
        else { if ((uint64_t)gap > chrom_len) return false; tgt += (uint64_t)gap; }
        seq += m2;
        tgt += m2;
    }
    if (seq != len || tgt > chrom_len) return false;
    w.len_c5 = (uint32_t)len | (uint32_t)c5 << 16;
    w.m_c3 = (uint32_t)m | (uint32_t)c3 << 16;
    w.m2_op = (gop ? (uint32_t)m2 : 0u) | gop << 16 | (rev ? 1u << 24 : 0u);
    w.gap = gop ? (uint32_t)gap : 0u;
    w.ok = 1;
    return true;
}

__device__ __forceinline__ int tag_digits(uint32_t v)
{
    int n = 1;
    while (v >= 10) { v /= 10; n++; }
    return n;
}

__device__ __forceinline__ void tag_put_num(char *w, uint32_t v, int nd)
{
    for (int k = nd - 1; k >= 0; k--) { w[k] = (char)('0' + v % 10); v /= 10; }
}

__device__ __forceinline__ char tag_letter(uint32_t code) { return (char)((0x4E54474341ULL >> (8 * code)) & 0xff); }      // "ACGTN"

__device__ __forceinline__ uint32_t tag_tgt_code(const uint64_t *__restrict__ tgt4, uint64_t g)
{
    const uint32_t c = (uint32_t)(tgt4[g >> 4] >> (60 - 4 * (g & 15))) & 7u;
    return c > 4 ? 4u : c;
}

__device__ __forceinline__ uint64_t tag_shfl64(uint64_t v, int src)
{
    return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src);
}

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// Called by all lanes of a wave, each with its own record's walk (ok = 0: none).  nm / md_len: the lane's own record's NM (kTagNone: no
// tags) and the length of its MD text.  WRITE: the text goes to the lane's md_dst as well (md_len bytes, no terminator).
template <bool WRITE>
__device__ __forceinline__ void wave_tags(const uint64_t *__restrict__ tgt4, const TagReads &rs, const TagWalk &mine, char *md_dst, uint32_t &nm_out, uint32_t &md_len_out)
{
    const int lane = (int)(threadIdx.x & 63);
    nm_out = kTagNone;
    md_len_out = 0;
    uint64_t todo = __ballot(mine.ok != 0);
    while (todo) {
        const int rr = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        // record rr's walk, in every lane
        const uint64_t rd_at = tag_shfl64(mine.rd_at, rr), g0 = tag_shfl64(mine.g0, rr);
        const uint32_t len_c5 = (uint32_t)__shfl((int)mine.len_c5, rr), m_c3 = (uint32_t)__shfl((int)mine.m_c3, rr), m2_op = (uint32_t)__shfl((int)mine.m2_op, rr);
        const uint32_t gap = (uint32_t)__shfl((int)mine.gap, rr);
        const uint32_t len = len_c5 & 0xffffu, c5 = len_c5 >> 16, m = m_c3 & 0xffffu, c3 = m_c3 >> 16, m2 = m2_op & 0xffffu, gop = (m2_op >> 16) & 0xffu;
        const bool rev = (m2_op >> 24) & 1u;
        uint32_t rd = 0, efirst = kTagNoExc;
        if (!rs.bases) { rd = (uint32_t)__shfl((int)mine.rd, rr); efirst = (uint32_t)__shfl((int)mine.efirst, rr); }
        char *md = WRITE ? reinterpret_cast<char *>(tag_shfl64(reinterpret_cast<uint64_t>(md_dst), rr)) : nullptr;
        uint32_t nm = 0, out = 0;
        int brk = -1;                                // the last M base (counted over both M runs) that a piece has used up
        for (int seg = 0; seg < 2; seg++) {
            const uint32_t seglen = seg ? m2 : m;
            if (!seglen) continue;
            const uint32_t sofs = seg ? c5 + m + c3 + (gop == 'I' ? gap : 0u) : c5;       // the run's first base in SEQ ..
            const uint64_t tpos = g0 + (seg ? (uint64_t)m + (gop != 'I' ? gap : 0u) : 0u);      // .. and in the target
            const uint32_t cbase = seg ? m : 0u;
            if (seg && gop == 'I') nm += gap;
            if (seg && gop == 'D') {
                // <run>^<deleted target letters>; the run after it starts from nothing
                const uint32_t run = (uint32_t)((int)m - 1 - brk);
                const int nd = tag_digits(run);
                if (WRITE) {
                    if (lane == 0) { tag_put_num(md + out, run, nd); md[out + nd] = '^'; }
                    for (uint32_t q = (uint32_t)lane; q < gap; q += 64) md[out + nd + 1 + q] = tag_letter(tag_tgt_code(tgt4, g0 + m + q));
                }
                out += (uint32_t)nd + 1 + gap;
                brk = (int)m - 1;
                nm += gap;
            }
            for (uint32_t base = 0; base < seglen; base += 64) {
                const uint32_t j = base + (uint32_t)lane;
                const bool in = j < seglen;
                uint32_t rc = 4, tc = 4;
                if (in) {
                    const uint32_t s = sofs + j, idx = rev ? len - 1 - s : s;
                    if (rs.bases) { rc = rs.bases[rd_at + idx] & 7u; rc = rc > 4 ? 4u : rc; }
                    else {
                        rc = (rs.pk_words[rd_at + (idx >> 4)] >> (30 - 2 * (idx & 15))) & 3u;
                        for (uint64_t e = efirst; e < rs.n_pk_exc && rs.pk_exc[e].read == rd; e++) {       // (efirst == kTagNoExc: no turn)
                            const bk_nbase x = rs.pk_exc[e];
                            if (idx >= x.pos && idx - x.pos <= x.run) rc = 4;
                        }
                    }
                    if (rev && rc < 4) rc = 3 - rc;
                    tc = tag_tgt_code(tgt4, tpos + j);
                }
                const bool mis = in && !(rc == tc && rc < 4);
                const uint64_t mask = __ballot(mis);
                if (!mask) continue;
                nm += (uint32_t)__popcll(mask);
                const uint64_t below = mask & ((1ULL << lane) - 1);
                const int prev = below ? (int)(cbase + base) + 63 - __clzll((long long)below) : brk;
                const uint32_t run = (uint32_t)((int)(cbase + j) - 1 - prev);
                const int nd = tag_digits(run);
                const uint32_t piece = mis ? (uint32_t)nd + 1 : 0u;
                const uint32_t incl = wave_incl_sum(piece, lane);
                if (WRITE && mis) {
                    char *w = md + out + incl - piece;
                    tag_put_num(w, run, nd);
                    w[nd] = tag_letter(tc);
                }
                out += (uint32_t)__shfl((int)incl, 63);
                brk = (int)(cbase + base) + 63 - __clzll((long long)mask);
            }
        }
        const uint32_t run = (uint32_t)((int)(m + m2) - 1 - brk);
        const int nd = tag_digits(run);
        if (WRITE && lane == 0) tag_put_num(md + out, run, nd);
        out += (uint32_t)nd;
        if (lane == rr) { nm_out = nm < kTagNone ? nm : kTagNone; md_len_out = out; }
    }
}

}  // namespace bk
