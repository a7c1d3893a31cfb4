"""mi_knn_sharded_density, mi_knn_sharded_dbscan and mi_knn_sharded_dbscan_stats without a GPU: the bindings, the argument
checks that come in front of any device work, and the host-only rules (csrc/density_sharded_host.h) under the sanitizers.
The contract itself is the single table's (tests/test_density_host.py: expected_dbscan) over the pairs of the sharded join;
tests/test_density_sharded_gpu.py compares with it for equality."""
import ctypes
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import ShardedTable

NEW = ["mi_knn_sharded_density", "mi_knn_sharded_dbscan", "mi_knn_sharded_dbscan_stats"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID = -1


def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert mi.mi_abi_version() == 4
    assert len(_lib.SYMBOLS["mi_knn_sharded_density"][1]) == 3 and len(_lib.SYMBOLS["mi_knn_sharded_dbscan"][1]) == 8
    for name in ("neighbor_counts", "dbscan", "dbscan_stats"):
        assert callable(getattr(ShardedTable, name)), name
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in NEW:
        assert name + "(" in hpp, name
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"density_sharded.hip"' in build


def test_null_handles_and_bad_arguments_return_codes_without_a_device(mi):
    cluster, via = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64)
    via_dist, counts, summary = np.full(4, -7.0, np.float32), np.full(4, 7, np.uint32), np.full(4, 7, np.uint64)
    out = (cluster.ctypes.data, via.ctypes.data, via_dist.ctypes.data, counts.ctypes.data, summary.ctypes.data)
    fake = ctypes.c_void_p(16)          # a handle that is never followed: every case below is refused in front of it
    assert mi.mi_knn_sharded_density(None, 0.1, counts.ctypes.data) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert mi.mi_knn_sharded_density(fake, 0.1, None) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_density(fake, -0.5, counts.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_density(fake, float("nan"), counts.ctypes.data) == MI_ERR_INVALID
    assert b"max_dist" in mi.mi_last_error()
    assert mi.mi_knn_sharded_dbscan(None, 0.1, 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_dbscan(fake, 0.1, 0, *out) == MI_ERR_INVALID
    assert b"min_pts" in mi.mi_last_error()
    assert mi.mi_knn_sharded_dbscan(fake, -1.0, 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_dbscan(fake, float("nan"), 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_dbscan(fake, 0.1, 5, None, *out[1:]) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_dbscan(fake, 0.1, 5, *out[:4], None) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_dbscan_stats(None, (ctypes.c_uint64 * 8)()) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_dbscan_stats(fake, None) == MI_ERR_INVALID
    assert np.all(cluster == 7) and np.all(via == 7) and np.all(via_dist == -7.0) and np.all(counts == 7) and np.all(summary == 7)


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_density_sharded_host.cpp: a stand-alone program over csrc/density_sharded_host.h — the argument rules,
    the cross rectangle's tile counts against a brute-force walk, the local-to-global scatter and the forest merge against a
    flood fill — built with the address and undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_density_sharded_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_density_sharded_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
