"""launch_min_len (biokanga_amd/csrc/bk_prep.hip) against numpy.min, through the test-only entry point of tests/hip/minlentest.hip
(biokanga_amd/lib/libbk_minlentest.so, built by csrc/Makefile with everything else).  The kernel keeps the minimum as the maximum of the
lengths' complements over a word its caller zeroed; the host reads ~word (bk_wave_form.h: min_len_of).  Sizes: one read, one wave less
one, a wave, a wave and one, and 100 000 reads (beyond one block, several waves per block); the shortest read at the first, the last and
a middle index, and no shorter read at all."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import helpers  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(helpers.ROOT, "biokanga_amd", "lib", "libbk_minlentest.so")
    if not os.path.exists(so):
        raise RuntimeError(f"{so} is missing: build it (make -C biokanga_amd/csrc)")
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch brings, as biokanga_amd.load_library does - two runtimes in one process see no device)
    lib = ctypes.CDLL(so)
    lib.bkml_min_len.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    lib.bkml_min_len.restype = ctypes.c_int
    return lib


def _min_len(lib, lens, start=0):
    import torch
    dev = torch.device("cuda:0")
    d_lens = torch.from_numpy(lens.astype(np.uint32).view(np.int32)).to(dev)
    d_out = torch.from_numpy(np.array([start], dtype=np.uint32).view(np.int32)).to(dev)
    assert lib.bkml_min_len(d_lens.data_ptr(), len(lens), len(lens), d_out.data_ptr()) == 0
    word = int(d_out.cpu().numpy().view(np.uint32)[0])
    assert word != 0                                   # (some read was seen)
    return word ^ 0xFFFFFFFF


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100_000])
def test_min_len_is_numpys(lib, n):
    equal = np.full(n, 100, dtype=np.uint32)
    assert _min_len(lib, equal) == int(np.min(equal)) == 100
    for at in sorted({0, n - 1, n // 2}):
        lens = equal.copy()
        lens[at] = 37
        assert _min_len(lib, lens) == int(np.min(lens)), (n, at)
    rng = np.random.default_rng(n)
    lens = rng.integers(1, 2000, n).astype(np.uint32)
    assert _min_len(lib, lens) == int(np.min(lens))


def test_min_len_folds_into_what_the_word_held(lib):
    """a word that already holds a shorter read's complement keeps it; the entry point refuses more reads than the buffer holds"""
    lens = np.full(1000, 100, dtype=np.uint32)
    assert _min_len(lib, lens, start=0xFFFFFFFF ^ 50) == 50
    assert _min_len(lib, lens, start=0xFFFFFFFF ^ 150) == 100
    import torch
    d = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    assert lib.bkml_min_len(d.data_ptr(), 8, 9, d.data_ptr()) != 0
