"""The narrow phase's row descriptor (NpRows, np_row_args, np_row_id in avian_amd/csrc/avn_kernels.h) as a stand-alone host program under AddressSanitizer and
UBSan (tests/np_rows_main.cpp): no GPU, no library, nothing loaded into Python.

For each of the three named constructors, lanes 0 .. n-1 must map to exactly the ids of the form's definition, written out here:
  active(list, n)                          lane a -> list[a]
  dense(n_rows)                            lane a -> a
  added(list, n_list, range_base, n_range) lane a -> list[a] below n_list, range_base + (a - n_list) from there on
at the sizes 0, 1, 63, 64, 65 and 257 (around a wavefront, and more than one workgroup of the light kernel), with the two corner cases of the added form at base 0:
an empty list -- which the kernel cannot tell from the dense form and is passed as that form -- and an empty range.  The program itself compares every id with what
the three former entry points passed to the kernel; a list is allocated with exactly its length, so a read past it is a sanitizer report."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SIZES = (0, 1, 63, 64, 65, 257)
ACTIVE, DENSE, ADDED = 0, 1, 2


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("np_rows") / "np_rows_main")
    r = subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "avian_amd", "csrc"), os.path.join(REPO, "tests", "np_rows_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def cases():
    """(form, list, range_base, n_range) and the ids of the form's definition"""
    rng = np.random.default_rng(11)
    ids = lambda n: rng.integers(0, 1 << 20, n).astype(np.uint32)
    out = []
    for n in SIZES:
        lst = ids(n)
        out.append(((ACTIVE, lst, 0, 0), lst))
        out.append(((DENSE, ids(0), 0, n), np.arange(n, dtype=np.uint32)))
        for base in (0, 1000):   # base 0 holds added(list, 0, 0, n) and added(list, k, 0, 0)
            for m in SIZES:
                lst = ids(n)
                out.append(((ADDED, lst, base, m), np.concatenate([lst, base + np.arange(m, dtype=np.uint32)])))
    return out


def test_every_lane_maps_to_the_row_of_its_form_under_sanitizers(program, tmp_path):
    cs = cases()
    assert any(c[0] == ADDED and len(c[1]) == 0 and c[2] == 0 and c[3] == 257 for c, _ in cs) and any(c[0] == ADDED and len(c[1]) == 257 and c[2] == 0 and c[3] == 0 for c, _ in cs)
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "ids.bin")
    with open(fin, "wb") as f:
        f.write(np.uint32(len(cs)).tobytes())
        for (form, lst, base, n_range), _ in cs:
            f.write(np.array([form, len(lst), base, n_range], np.uint32).tobytes() + lst.tobytes())
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"NP_ROWS_OK {len(cs)}" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr[-4000:]
    got = np.fromfile(fout, np.uint32)
    at = 0
    for (form, lst, base, n_range), want in cs:
        n = int(got[at])
        assert n == len(want), (form, len(lst), base, n_range, n)
        assert np.array_equal(got[at + 1:at + 1 + n], want), (form, len(lst), base, n_range)
        at += 1 + n
    assert at == len(got)
