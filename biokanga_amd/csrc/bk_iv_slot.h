// bk_iv_slot.h - where the interval record of (read, strand, core) lies in a phase, and the way back.  Nothing of HIP here but the
// qualifiers: the arithmetic is checked on the CPU (tests/test_host_iv_slot.py).
//
// slot = (strand * iv_cores + core) * iv_stride + index.  The index is the read's POSITION in the phase's active list, so that lanes
// working on neighbouring active reads touch neighbouring words in every phase - or, where the flag says so, the read's NUMBER: phase 0
// of a batch whose read preparation searched (k_prep_fused<.., SEARCH0>) - its lanes store the records before the first active list
// has been laid out, and in that phase nearly every read is on the list anyway.  iv_stride is the chunk's read count in both forms.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BK_SLOT_HD __host__ __device__
#else
#define BK_SLOT_HD
#endif

namespace bk {

// what a slot is numbered by: the position a, or - by_read - the read r
BK_SLOT_HD inline uint32_t iv_index(uint32_t by_read, uint32_t a, uint32_t r) { return by_read ? r : a; }

BK_SLOT_HD inline uint64_t iv_slot_at(uint32_t iv_cores, uint32_t iv_stride, uint32_t index, int st, int c)
{
    return (uint64_t)(st * (int)iv_cores + c) * iv_stride + index;
}

// the way back (plain divisions; the kernels use slot_decode's reciprocals, bk_plan_table.h, which give the same three numbers)
BK_SLOT_HD inline void iv_slot_split(uint64_t slot, uint32_t iv_cores, uint32_t iv_stride, uint32_t &index, int &st, int &c)
{
    const uint64_t plane = slot / iv_stride;
    index = (uint32_t)(slot - plane * iv_stride);
    st = (int)(plane / iv_cores);
    c = (int)(plane - (uint64_t)st * iv_cores);
}

// the read a decoded index stands for: itself, or the list's entry at that position
BK_SLOT_HD inline uint32_t iv_index_read(uint32_t by_read, uint32_t index, const uint32_t *act) { return by_read ? index : act[index]; }

}  // namespace bk
