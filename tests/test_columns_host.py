"""The host copy of a per-row column (csrc/columns_host.h: the group id, the tags, the stamps) without a GPU: its rules under
the sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_rules_under_the_sanitizers(tmp_path):
    """tests/cpp/test_columns_host.cpp: a stand-alone program over csrc/columns_host.h — read with the default at and beyond
    the end, write that extends, truncation to 0 / the length / beyond it, and compact_column with 32- and 64-bit dead lists
    (none, first, last, every, alternating), against brute force for columns of 0, 1, 63, 64, 65 and 200 rows"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_columns_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_columns_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-4000:] + out.stderr[-4000:]
