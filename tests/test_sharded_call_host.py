"""What the sharded table's calls share on the host (csrc/sharded_call.h) without a GPU: the router of global ids against a
brute-force placement, the per-shard result lists and their merge against a plain sort, under the sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_sharded_call_host.cpp: a stand-alone program over the part of csrc/sharded_call.h without HIP in it,
    built with the address and undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_sharded_call_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_sharded_call_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
