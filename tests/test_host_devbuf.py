"""bk::DevBuf and bk::PinBuf (biokanga_amd/csrc/bk_devbuf.h), the owners of the library's device and page-locked buffers, on the host (CPU
only): tests/cpp/devbuf_host.cpp includes the header as it stands and defines the two pairs of allocator functions they go through over
malloc / free, each pair with a pool of its own that counts live allocations and fails one on request.  Built with the ROCm compiler as the host compiler and BK_TEST_CXXFLAGS as given
(ASan + UBSan where the other host tests run under them)."""
import os
import subprocess

import helpers

CSRC = os.path.join(helpers.ROOT, "biokanga_amd", "csrc")


def test_devbuf_ownership_rules_on_the_host(tmp_path):
    """ensure() that fits calls nothing; growing frees first and allocates exactly n; a failed ensure leaves an empty buffer that works
    again; moves empty their source and free what they overwrite; nothing is live at exit and nothing is freed twice - for either owner,
and memory of one kind never reaches the other kind's free"""
    exe = str(tmp_path / "devbuf_host")
    flags = os.environ.get("BK_TEST_CXXFLAGS", "-O2").split()
    # (the header takes hipError_t from the HIP headers and nothing else of HIP: no device, no runtime library)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "c++"] + flags + ["-std=c++17", "-Wall", "-I" + CSRC, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", exe,
                           os.path.join(helpers.ROOT, "tests", "cpp", "devbuf_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
