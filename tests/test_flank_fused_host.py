"""CPU: the flank sweeps' fused column pass as a host program.  tests/cpp/flank_fused_test.cpp runs the row step of
hipstr_amd/csrc/flank_sweep_step.h — the text band_sweep_coop compiles for the device — with the kernel's pass structure (column 0
initialised, one top-down pass per column over (M, I) per row, the last pass without its rows) on random blocks of 1-40 rows x 1-20
columns cut into bands of 1-15 rows, and compares every last-column M, every last-row M and every handed-over (M, D) pair with a plain
full-matrix evaluation of the recurrence in the reference's order: memcmp, 0 mismatches.  Built with -ffp-contract=off and the address
and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flank_fused") / "flank_fused_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-I", os.path.join(ROOT, "hipstr_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "flank_fused_test.cpp")], check=True)
    return exe


def test_fused_sweep_equals_the_full_matrix(program):
    r = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout
    assert " 0 mismatches" in r.stdout, r.stdout
