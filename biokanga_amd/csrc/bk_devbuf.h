// bk_devbuf.h - bk::DevBuf<T>: the owner of one device buffer (bk_ctx_int.h: the index image, the small fixed buffers and the batch-side
// buffers of a context; the temporaries of bk_image.cpp and of the entry points).  A pointer and a capacity in elements - the capacity IS
// the buffer's size: an image table is made by ensure() on an empty buffer, cloned by its cap(), handed on by move.  Frees in its
// destructor; a move-assignment frees what the target held on the spot.  Growing frees first and then allocates exactly what was asked
// for - no copy, no growth factor: free-before-allocate is what keeps the peak inside the HBM budget of DESIGN.md section 3.  All memory
// goes through bk::dev_malloc_bytes / bk::free_dev (bk_image.cpp: BK_POISON, BK_TIMING).
#pragma once
#include <cstddef>
#include <utility>
#include <hip/hip_runtime_api.h>

namespace bk {
hipError_t dev_malloc_bytes(void **p, size_t bytes);
void free_dev(void *p);

template <class T> class DevBuf {
    T *p_ = nullptr;
    size_t cap_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}       // (a moved-from buffer is empty)
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
        return *this;
    }
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    size_t cap() const { return cap_; }             // elements
    void reset() { free_dev(p_); p_ = nullptr; cap_ = 0; }
    // room for n elements: nothing happens when it is there; else the old memory goes first and exactly n elements are allocated (the
    // contents are not kept).  A failure leaves the buffer empty.
    hipError_t ensure(size_t n)
    {
        if (n <= cap_) return hipSuccess;
        reset();
        void *q = nullptr;
        const hipError_t e = dev_malloc_bytes(&q, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(q);
        cap_ = n;
        return hipSuccess;
    }
};
}  // namespace bk
