"""The staging arena's layout arithmetic (avian_amd/csrc/avn_stage.h) as a stand-alone host program under AddressSanitizer and UBSan: no GPU, no
library, nothing loaded into Python.  tests/stage_layout_main.cpp holds the checks."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stage_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "avian_amd", "csrc"), os.path.join(REPO, "tests", "stage_layout_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "STAGE_LAYOUT_OK" in r.stdout, r.stdout + r.stderr
