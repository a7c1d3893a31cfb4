"""The id space of a table (csrc/ids.h) without a GPU: local row <-> id and the block-cyclic placement arithmetic, against a
brute-force placement of every row, under the sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_ids_host.cpp: a stand-alone program over csrc/ids.h, built with the address and
    undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_ids_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_ids_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
