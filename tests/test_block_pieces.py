"""CPU: the piece arithmetic of the stage calls' cache blocks (hipstr_amd/csrc/block_pieces.h: 256-byte steps, zero takes a step, the mark
where the results end) through the stand-alone program tests/cpp/block_pieces_test.cpp built with -fsanitize=address,undefined (its own
process: nothing is preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sanitized_program(tmp_path):
    exe = str(tmp_path / "block_pieces_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "block_pieces_test.cpp")], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok "), r.stdout
