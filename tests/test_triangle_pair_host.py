"""avian_amd/csrc/avn_triangle_pair.h as a stand-alone host program under AddressSanitizer and UBSan (tests/triangle_pair_main.cpp): no GPU, no library,
nothing loaded into Python.  The device header compiles as plain C++ (the HIP headers define __device__ away for a non-HIP compiler), with
-ffp-contract=off so that every operation is rounded once as on the device.

The pair set of the GPU batch-query test (tests/triangle_pair_set.py) must come out equal to tests/triangle_collider_reference.py bit for bit in every
output array, in both scalars; its triangle-free rows, which that reference leaves empty and the GPU test compares with World.contact_manifolds, are only
required to be produced.  20 000 further random rows per scalar -- half of them squeezed into deep overlap, where a clip polygon grows its most corners -- are
only required to be produced without a sanitizer report."""
import os
import subprocess

import numpy as np
import pytest

import triangle_pair_set as PS
from test_triangle_collider_cpu import COMBOS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("triangle_pair") / "triangle_pair_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "avian_amd", "csrc"),
                        os.path.join(REPO, "tests", "triangle_pair_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run(program, tmp_path, p, bits):
    fin, fout = str(tmp_path / f"pairs_{bits}.bin"), str(tmp_path / f"manifolds_{bits}.bin")
    PS.write_pairs(fin, p, bits)
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TRIANGLE_PAIRS_OK" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr[-4000:]
    return PS.read_manifolds(fout, len(p["shape1"]), bits)


@pytest.mark.parametrize("bits", [32, 64])
def test_pair_set_equals_the_reference_bit_for_bit_under_sanitizers(program, tmp_path, bits):
    p, ref, ref7, spans = PS.pair_set(bits)
    for label, (got, need) in PS.coverage(p, ref, ref7, spans).items():
        print(f"{label}: {got} (at least {need})")
        assert got >= need, label
    out = run(program, tmp_path, p, bits)
    tri = (p["shape1"] == PS.TRI) | (p["shape2"] == PS.TRI)
    assert tri.sum() == len(tri) - PS.TRIANGLE_FREE_ROWS
    for name in PS.OUTPUTS + ("point",):
        bad = np.nonzero([not PS.same_bits(out[name][i], ref[name][i]) for i in np.nonzero(tri)[0]])[0]
        assert len(bad) == 0, f"{name}: {len(bad)} rows differ, first row {np.nonzero(tri)[0][bad[0]]}"


@pytest.mark.parametrize("bits", [32, 64])
def test_twenty_thousand_random_rows_leave_no_sanitizer_report(program, tmp_path, bits):
    dt = np.float32 if bits == 32 else np.float64
    rng = np.random.default_rng(77 + bits)
    batches = []
    for k, (k1, k2) in enumerate(COMBOS):
        n = 3334 if k < 2 else 3333
        b = list(PS.random_flag_pairs(rng, k1, k2, n))
        deep = np.arange(n) % 2 == 0   # every other row: the two shapes almost concentric, random orientations
        b[6] = np.where(deep[:, None], b[2] + (b[6] - b[2]) * 0.05, b[6])
        batches.append(tuple(b))
    p = PS.concat(batches, dt)
    assert len(p["shape1"]) == 20000
    out = run(program, tmp_path, p, bits)
    assert out["point_count"].max() <= 8 and (out["point_count"] > 0).sum() > 5000
    assert (out["point_count"] >= 5).sum() > 100, "deep overlaps reach the many-cornered polygons"
