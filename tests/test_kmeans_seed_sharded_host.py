"""mi_knn_sharded_kmeans_seed and mi_knn_sharded_kmeans_seed_stats without a GPU: the bindings, the argument checks that come
in front of any device work, the Python surface, and the host-only plan (csrc/kmeans_seed_sharded_host.h: candidates per
shard, chunks, global order, bytes exchanged) under the sanitizers.  The bits are compared on the GPU
(tests/test_kmeans_seed_sharded_gpu.py)."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ShardedTable

NEW = ["mi_knn_sharded_kmeans_seed", "mi_knn_sharded_kmeans_seed_stats"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5


def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
        assert name + "(" in hpp, name
    assert mi.mi_abi_version() == 4
    # the one-table call's argument list behind another handle type
    assert _lib.SYMBOLS["mi_knn_sharded_kmeans_seed"][1] == _lib.SYMBOLS["mi_knn_kmeans_seed"][1]
    assert len(_lib.SYMBOLS["mi_knn_sharded_kmeans_seed_stats"][1]) == 2
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"kmeans_seed_sharded.hip"' in build
    for f in ("kmeans_seed_sharded.hip", "kmeans_seed_sharded_kernels.h", "kmeans_seed_sharded_host.h"):
        assert os.path.exists(os.path.join(ROOT, "image_search_amd", "csrc", f)), f


def test_python_surface():
    p = inspect.signature(ShardedTable.kmeans_seed).parameters
    assert list(p) == ["self", "k", "seed", "among"] and p["seed"].default == 0 and p["among"].default is None
    assert list(p) == list(inspect.signature(EmbeddingTable.kmeans_seed).parameters)
    assert list(inspect.signature(ShardedTable.kmeans_seed_stats).parameters) == ["self"]
    p = inspect.signature(ShardedTable.kmeans_seeded).parameters
    assert list(p) == ["self", "k", "max_iters", "seed", "sample"]
    assert (p["max_iters"].default, p["seed"].default, p["sample"].default) == (20, 0, None)
    # init="kmeans++" inside kmeans still says why not; its docstring points to the call that does it
    assert "kmeans_seeded" in ShardedTable.kmeans.__doc__


def test_null_handles_and_bad_arguments_return_codes_without_a_device(mi):
    rows, cent = np.full(4, 7, np.uint64), np.full((4, 8), 3.0, np.float32)
    ids = np.arange(3, dtype=np.uint64)
    fake = ctypes.c_void_p(16)          # a handle that is never followed: every case below is refused in front of it
    seed = mi.mi_knn_sharded_kmeans_seed
    pot = ctypes.c_double(-7.0)
    assert seed(None, 4, 0, None, 0, rows.ctypes.data, cent.ctypes.data, ctypes.byref(pot)) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert pot.value == 0.0             # (as the one-table call: the potential is cleared first)
    assert seed(fake, 4, 0, None, 0, None, cent.ctypes.data, None) == MI_ERR_INVALID
    assert b"rows is null" in mi.mi_last_error()
    assert seed(fake, 0, 0, None, 0, rows.ctypes.data, cent.ctypes.data, None) == MI_ERR_INVALID
    assert b"C must be" in mi.mi_last_error()
    assert seed(fake, 4, 0, None, 3, rows.ctypes.data, cent.ctypes.data, None) == MI_ERR_INVALID
    assert b"among is null" in mi.mi_last_error()
    assert seed(fake, 65537, 0, ids.ctypes.data, 3, rows.ctypes.data, cent.ctypes.data, None) == MI_ERR_UNSUPPORTED
    assert b"65536" in mi.mi_last_error()
    out = (ctypes.c_uint64 * 4)()
    assert mi.mi_knn_sharded_kmeans_seed_stats(None, out) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_kmeans_seed_stats(fake, None) == MI_ERR_INVALID
    assert np.all(rows == 7) and np.all(cent == 3.0)


def test_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/test_kmeans_seed_sharded_host.cpp: a stand-alone program over csrc/kmeans_seed_sharded_host.h — the five
    layouts, all rows and subsets with gaps of whole blocks, chunks that concatenate to the sorted candidates in global order,
    none across a block or beyond 256 positions, empty shards, the exchange-byte formula — built with the address and
    undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_kmeans_seed_sharded_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_kmeans_seed_sharded_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
