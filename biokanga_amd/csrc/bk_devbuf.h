// bk_devbuf.h - bk::DevBuf<T> and bk::PinBuf<T>: the owners of one device buffer and of one page-locked host buffer.  Everything the library
// allocates is one of the two: the index image, the small fixed buffers and the batch-side buffers of a context (bk_ctx_int.h), the staging
// of the request passes (bk_stage.h), the slots of the stream pipeline and of the contaminant matcher, the temporaries of bk_image.cpp, of
// the suffix array builders and of the entry points.  A pointer and a capacity in elements - the capacity IS the buffer's size: an image
// table is made by ensure() on an empty buffer, cloned by its cap(), handed on by move.  Frees in its destructor; a move-assignment frees
// what the target held on the spot.  Growing frees first and then allocates exactly what was asked for - no copy, no growth factor:
// free-before-allocate is what keeps the peak inside the HBM budget of DESIGN.md section 3.  Device memory goes through
// bk::dev_malloc_bytes / bk::free_dev (BK_POISON, BK_TIMING), page-locked memory through bk::pin_malloc_bytes / bk::free_pin (bk_image.cpp).
#pragma once
#include <cstddef>
#include <utility>
#include <hip/hip_runtime_api.h>

namespace bk {
hipError_t dev_malloc_bytes(void **p, size_t bytes);
void free_dev(void *p);
hipError_t pin_malloc_bytes(void **p, size_t bytes);      // hipHostMallocDefault: for the device that is current
void free_pin(void *p);

template <class T, hipError_t (*Alloc)(void **, size_t), void (*Free)(void *)> class OwnedBuf {
    T *p_ = nullptr;
    size_t cap_ = 0;

public:
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    OwnedBuf(OwnedBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}       // (a moved-from buffer is empty)
    OwnedBuf &operator=(OwnedBuf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
        return *this;
    }
    ~OwnedBuf() { reset(); }

    T *get() const { return p_; }
    size_t cap() const { return cap_; }             // elements
    size_t bytes() const { return cap_ * sizeof(T); }
    void reset() { Free(p_); p_ = nullptr; cap_ = 0; }
    // room for n elements: nothing happens when it is there; else the old memory goes first and exactly n elements are allocated (the
    // contents are not kept).  A failure leaves the buffer empty.
    hipError_t ensure(size_t n)
    {
        if (n <= cap_) return hipSuccess;
        reset();
        void *q = nullptr;
        const hipError_t e = Alloc(&q, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(q);
        cap_ = n;
        return hipSuccess;
    }
};
template <class T> using DevBuf = OwnedBuf<T, dev_malloc_bytes, free_dev>;
template <class T> using PinBuf = OwnedBuf<T, pin_malloc_bytes, free_pin>;
}  // namespace bk
