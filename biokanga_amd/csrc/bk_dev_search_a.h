// bk_dev_search_a.h - pass A of the search for ONE core, stage by stage: k-mer table, small bucket out of the second-level keys, the
// record and what becomes of it.  Shared by k_search_a_ilp (bk_search.hip), which runs the stages of its ILP items one after the other so
// that a stage's loads are in flight together, and by the searching form of the read preparation (k_prep_fused<.., SEARCH0>,
// bk_prep.hip), which does phase 0's core 0 from the bases its lane holds.  The probe is the same in both: p0 = the core's first 16
// bases as nibbles, masked to the core's length, with 0x4000000000000000 set where an N among the bases behind the k-mer keeps the core
// from the 2-bit keys; q2raw = the 16 bases behind the k-mer's, 2 bits each.
#pragma once
#include "bk_dev_k2.h"

namespace bk {

constexpr uint32_t kNoIv32 = 0xFFFFFFFFu;       // DevBatch::iv32: count of an entry nobody has left an interval in

struct PassACore {
    // the probe (stage 1)
    bool on;                    // the item is a core its read has
    bool cached;                // a later phase's offset-0 core whose interval phase 0 left in iv32 (cv)
    uint2 cv;
    uint64_t p0;
    uint32_t q2raw;
    int cl;
    // stage 2
    bool have_code;
    uint64_t lo, hi;
    uint32_t key0;
    // stage 3
    uint32_t key[kInlineBucket];
    bool absent;                // the table's line says that no key of the bucket continues the way the core does
    bool carry;                 // a bucket of one suffix whose table entry carries the suffix itself: handed on as it is (kElemFlag)
    // stage 4
    uint64_t first;
    uint32_t nval;
    bool push;                  // the slot goes on pass B's work list
    uint2 leave;                // what phase 0 leaves in iv32 for this read and strand
};

__device__ __forceinline__ void pass_a_clear(PassACore &s)
{
    s.on = false; s.cached = false; s.cv = make_uint2(0, kNoIv32); s.p0 = 0; s.q2raw = 0; s.cl = 1;
    s.have_code = false; s.lo = s.hi = 0; s.key0 = kK2Above; s.first = 0; s.nval = 0; s.push = false; s.leave = make_uint2(0, kNoIv32);
}

// stage 2: k-mer table
__device__ __forceinline__ void pass_a_table(const DevIndex &ix, int k, PassACore &s)
{
    s.nval = kKindFull << kKindShift;
    s.push = s.on;
    s.have_code = s.on && !s.cached && s.cl >= k && !(s.p0 & 0x4444444444444444ULL & top_mask(k));
    s.key0 = kK2Above;
    if (s.have_code) {
        const uint64_t code = (uint64_t)(squeeze2(s.p0) >> (32 - 2 * k));
        if (ix.ktab2 != nullptr) {
            // {bucket start, second-level key of its first suffix}: a bucket of one - every second one a read of a unique region
            // meets, and a third of those its other strand runs into by chance - is settled by the line that names it
            const uint2 e0 = ix.ktab2[code], e1 = ix.ktab2[code + 1];
            s.lo = e0.x; s.hi = e1.x; s.key0 = e0.y;                // (a bucket of one: its key; a larger one: the map of its keys' first five bits)
        } else {
            ktab_get_pair(ix, code, s.lo, s.hi);
        }
    }
}

// stage 3: small buckets from the key array
// (a lane loads the keys its bucket has - one to three for most - and no more: this kernel lives on the rate at which the
// texture path takes lane requests, and sixteen keys for every lane cost a third more time than the search saved)
__device__ __forceinline__ void pass_a_keys(const DevIndex &ix, int k, int lazy, PassACore &s)
{
    const uint64_t size = s.hi - s.lo;
    const uint32_t m = k2_mask(s.cl - k);
    s.absent = s.have_code && ix.ktab2 != nullptr && size >= 2 && ktab2_absent(s.key0, m, s.q2raw & m);
    s.carry = s.have_code && lazy && ix.ktab2 != nullptr && ix.ktab2_elem && size == 1;
    const bool key_in_entry = size == 1 && ix.ktab2 != nullptr && !ix.ktab2_elem;
#pragma unroll
    for (uint32_t j = 0; j < kInlineBucket; j++)
        s.key[j] = (s.have_code && !s.absent && !s.carry && size <= kInlineBucket && j < size) ? (key_in_entry ? s.key0 : ix.k2[s.lo + j]) : kK2Above;
}

// stage 4: results
__device__ __forceinline__ void pass_a_result(int k, int lazy, PassACore &s)
{
    s.leave = make_uint2(0, kNoIv32);
    if (s.cached && (s.cv.y & kElemFlag)) {
        // phase 0 met a bucket of one suffix here and handed the suffix on: so does this phase
        s.first = s.cv.x;
        s.nval = s.cv.y;
        s.push = false;
    } else if (s.cached) {
        // the interval of the first k + 15 bases, as the bucket compare below would have produced it
        s.first = s.cv.x;
        const uint32_t cnt = s.cv.y;
        if (cnt == 0 || s.cl <= k + kK2Bases) { s.nval = cnt; s.push = false; }
        else if (lazy && cnt <= kLazyBucket) { s.nval = cnt | kLazyFlag; s.push = false; }
        else s.nval = cnt | (kKindDeep << kKindShift);
    }
    if (s.carry) {
        // (the table's line named the bucket and the suffix in it: no key line, no suffix array line - the window the extension fetches
        // says whether the core is there)
        s.first = s.key0;
        s.nval = 1u | kIvFlags;
        s.push = false;
        s.leave = make_uint2(s.key0, 1u | kIvFlags);
    } else if (s.have_code) {
        const uint64_t size = s.hi - s.lo;
        if (size == 0 || s.absent) { s.first = s.lo; s.nval = 0; s.push = false; s.leave = make_uint2((uint32_t)s.lo, 0u); }
        else if (size <= kInlineBucket) {
            const uint32_t m = k2_mask(s.cl - k), q2 = s.q2raw & m;
            uint32_t lb = 0, ub = 0;
            bool suspect = false;                          // a key of the N kind counted as equal: pass B has a look at the target
#pragma unroll
            for (uint32_t j = 0; j < kInlineBucket; j++) {
                const int cm = k2_cmp(s.key[j], m, q2);
                lb += cm < 0;
                ub += cm <= 0;
                suspect |= cm == 0 && k2_nkind(s.key[j]);
            }
            if (suspect) {
                s.first = s.lo;
                s.nval = (uint32_t)size | (kKindK2 << kKindShift);
            } else {
                s.first = s.lo + lb;
                const uint32_t cnt = ub - lb;
                s.leave = make_uint2((uint32_t)s.first, cnt);
                if (cnt == 0 || s.cl <= k + kK2Bases) { s.nval = cnt; s.push = false; }
                else if (lazy && cnt <= kLazyBucket) { s.nval = cnt | kLazyFlag; s.push = false; }
                else s.nval = cnt | (kKindDeep << kKindShift);
            }
        } else if (size < (1ULL << kKindShift)) {
            s.first = s.lo;
            s.nval = (uint32_t)size | (kKindK2 << kKindShift);        // (pass B leaves the interval in iv32 after its key bisection)
        }
    }
}

}  // namespace bk
