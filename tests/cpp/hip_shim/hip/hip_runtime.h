// hip/hip_runtime.h - host stand-in for the HIP runtime header: with tests/cpp/hip_shim on the include path bk_device.h, bk_dev_util.h and
// bk_dev_k2.h compile for the host as they stand (tests/cpp/dev_search_host.cpp).  Only what those headers use.
#pragma once
#include <cstdint>

#define __device__
#define __host__
#define __global__
#define __launch_bounds__(...)
#define __forceinline__ inline

struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
struct bk_shim_idx { unsigned x = 0, y = 0, z = 0; };
struct bk_shim_dim { unsigned x = 1, y = 1, z = 1; };
static thread_local bk_shim_idx blockIdx, threadIdx;
static thread_local bk_shim_dim blockDim, gridDim;
typedef void *hipStream_t;

template <typename T> static inline T atomicAdd(T *p, T v) { const T old = *p; *p = old + v; return old; }
template <typename T> static inline T atomicMax(T *p, T v) { const T old = *p; if (v > old) *p = v; return old; }
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline int __clzll(long long v) { return v == 0 ? 64 : __builtin_clzll((unsigned long long)v); }
static inline unsigned long long __brevll(unsigned long long v)
{
    unsigned long long r = 0;
    for (int i = 0; i < 64; i++) r |= ((v >> i) & 1ULL) << (63 - i);
    return r;
}
#define __builtin_amdgcn_readfirstlane(x) (x)
static inline void __syncthreads() {}
