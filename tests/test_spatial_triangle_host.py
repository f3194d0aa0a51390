"""avian_amd/csrc/avn_spatial_triangle_pair.h -- the pair tests of the spatial queries against triangle colliders -- as a stand-alone host program under
AddressSanitizer and UBSan (tests/spatial_triangle_main.cpp): no GPU, no library, nothing loaded into Python.  The device header compiles as plain C++
(the HIP headers define __device__ away for a non-HIP compiler), with -ffp-contract=off so that every operation is rounded once as on the device.

Two inputs per scalar, each required to come out equal to tests/spatial_triangle_collider_reference.py bit for bit in every answer: the GPU test's rays and
query shapes paired with faces of its mesh (tests/spatial_triangle_set.py: gpu_case_rows), and 4 000 random rows (random_rows: rays, projections,
intersections, casts of the three query kinds and the segment - triangle distance, slivers and touching starts among them)."""
import os
import subprocess

import numpy as np
import pytest

import spatial_triangle_set as TS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spatial_triangle") / "spatial_triangle_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "avian_amd", "csrc"),
                        os.path.join(REPO, "tests", "spatial_triangle_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run(program, tmp_path, rows, bits):
    fin, fout = str(tmp_path / f"rows_{bits}.bin"), str(tmp_path / f"answers_{bits}.bin")
    TS.write_rows(fin, rows, bits)
    r = subprocess.run([program, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SPATIAL_TRIANGLE_OK" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr[-4000:]
    return TS.read_answers(fout, len(rows["op"]), bits)


def same(got, want, rows, what):
    (hit, res), (whit, wres, rounds) = got, want
    assert rounds.max() < 32, f"{what}: a cast reaches the Newton round cap"
    bad = np.nonzero((hit != whit) | (res.view(np.uint8).reshape(len(hit), -1) != wres.view(np.uint8).reshape(len(hit), -1)).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(hit)} rows differ; first row {bad[0]}: op {rows['op'][bad[0]]} kind {rows['kind'][bad[0]]} got {hit[bad[0]]} {res[bad[0]]} want {whit[bad[0]]} {wres[bad[0]]}"
    for name, op in TS.OPS.items():
        m = rows["op"] == op
        print(f"{what}: {name}: {m.sum()} rows, {hit[m].sum()} hits" + (f", most Newton rounds {rounds[m].max()}" if name == "cast" and m.any() else ""))


@pytest.mark.parametrize("bits", [32, 64])
def test_the_gpu_tests_case_set_equals_the_reference_bit_for_bit_under_sanitizers(program, tmp_path, bits):
    rows = TS.gpu_case_rows()
    got = run(program, tmp_path, rows, bits)
    same(got, TS.reference(rows, bits), rows, f"case set f{bits}")
    hit = got[0]
    for name, least in (("ray", 150), ("intersects", 100), ("cast", 300)):
        assert hit[rows["op"] == TS.OPS[name]].sum() >= least, name
    for kind in (TS.CUB, TS.BALL, TS.CAP):
        m = (rows["op"] == TS.OPS["cast"]) & (rows["kind"] == kind)
        assert (hit[m] == 1).sum() >= 60 and ((hit[m] == 1) & (got[1][m, 0] > 0)).sum() >= 30 and ((hit[m] == 1) & (got[1][m, 0] == 0)).sum() >= 5, kind


@pytest.mark.parametrize("bits", [32, 64])
def test_four_thousand_random_rows_equal_the_reference_bit_for_bit_under_sanitizers(program, tmp_path, bits):
    rows = TS.random_rows(np.random.default_rng(500 + bits), 4000)
    got = run(program, tmp_path, rows, bits)
    same(got, TS.reference(rows, bits), rows, f"random f{bits}")
    for name in TS.OPS:
        m = rows["op"] == TS.OPS[name]
        assert m.sum() >= 600 and got[0][m].sum() >= 100, name
    ray = rows["op"] == TS.OPS["ray"]
    assert (ray & (got[0] == 1) & (got[1][:, 0] == 0)).sum() >= 20, "rays that start on the triangle hit at t = 0"
