"""DevBuf and Pinned (avian_amd/csrc/avn_devbuf.h), the host side's two grow-only allocations, without a GPU: a stand-alone host program over a stub
runtime whose n-th allocation fails, under AddressSanitizer and UBSan (tests/devbuf_main.cpp holds the checks), and the compile-time guarantee
that an allocation result cannot be dropped.  No library, nothing loaded into Python."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(REPO, "avian_amd", "csrc")]


def test_devbuf_under_sanitizers(tmp_path):
    exe = str(tmp_path / "devbuf")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    *INCLUDES, os.path.join(REPO, "tests", "devbuf_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "DEVBUF_OK" in r.stdout, r.stdout + r.stderr


UNIT = """#include "avn_devbuf.h"
hipError_t device(avn::DevBuf& b) { %s }
hipError_t typed(avn::DevBuf& b, float** f) { %s }
hipError_t pinned(avn::Pinned& h) { %s }
"""
CHECKED = ("return b.ensure(64);", "return b.ensure_as(16, f);", "return h.ensure(64);")


def test_dropped_allocation_result_does_not_compile(tmp_path):
    def compiles(name, bodies):
        src = tmp_path / (name + ".cpp")
        src.write_text(UNIT % bodies)
        return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Werror=unused-result", *INCLUDES, str(src)], capture_output=True, text=True)

    r = compiles("checked", CHECKED)
    assert r.returncode == 0, r.stderr
    for i, dropped in enumerate(("b.ensure(64); return hipSuccess;", "b.ensure_as(16, f); return hipSuccess;", "h.ensure(64); return hipSuccess;")):
        bodies = list(CHECKED)
        bodies[i] = dropped
        r = compiles("dropped%d" % i, tuple(bodies))
        assert r.returncode != 0 and "unused-result" in r.stderr, "a dropped result compiled: " + dropped + "\n" + r.stderr
