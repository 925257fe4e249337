// minlentest.hip - launch_min_len of biokanga_amd/csrc/bk_prep.hip under a test-only entry point: the file is included as it stands (with
// bk_index.hip beside it, for launch_fill_u64), nothing of the library is linked in.  Built as biokanga_amd/lib/libbk_minlentest.so
// (csrc/Makefile); tests/test_gpu_min_len.py loads it.  The entry point takes raw device pointers with the size of the buffer behind the
// lengths, calls the LAUNCHER on the null stream as bk_engine.cpp does, synchronises and returns the hipError_t; arguments that would let
// the kernel leave its buffer are answered with hipErrorInvalidValue and no launch.
#include "../../biokanga_amd/csrc/bk_index.hip"
#include "../../biokanga_amd/csrc/bk_prep.hip"

using namespace bk;

extern "C" {

// out: one word, which the kernel folds the complement of its minimum into (the engine zeroes it first)
int bkml_min_len(const uint32_t *lens, uint64_t lens_words, uint64_t n, uint32_t *out)
{
    if (n == 0 || n > 0xFFFFFFFFu || n > lens_words || !lens || !out) return (int)hipErrorInvalidValue;
    launch_min_len(lens, (uint32_t)n, out, 0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}

}  // extern "C"
