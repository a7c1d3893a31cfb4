"""mi_knn_sharded_summarize and mi_knn_sharded_summarize_stats without a GPU: the bindings, the argument checks that come in
front of any device work, and the host-only rules (csrc/summary_sharded_host.h: the dealing of labels, the slots to global ids
and their merge, the exchanged bytes) under the sanitizers."""
import ctypes
import inspect
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ShardedTable

NEW = ["mi_knn_sharded_summarize", "mi_knn_sharded_summarize_stats"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5


def exchange_bytes(shards, C, dim):
    """what crosses between shards in one call (include/mi355clip.h): sums, sizes and slots inward, centroids outward"""
    return (shards - 1) * C * (8 * dim + 4 + 32) + (shards - 1) * 4 * C * dim


def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
        assert name + "(" in hpp, name
    assert mi.mi_abi_version() == 4
    assert len(_lib.SYMBOLS["mi_knn_sharded_summarize"][1]) == 13 == len(_lib.SYMBOLS["mi_knn_summarize"][1])
    assert len(_lib.SYMBOLS["mi_knn_sharded_summarize_stats"][1]) == 2
    for name in ("summarize", "summarize_stats"):
        assert callable(getattr(ShardedTable, name)), name
    assert inspect.signature(ShardedTable.summarize) == inspect.signature(EmbeddingTable.summarize)
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"summary_sharded.hip"' in build
    assert "k-means over a sharded table is not offered" not in header


def test_null_handles_and_bad_group_counts_return_codes_without_a_device(mi):
    C = 4
    cent = np.full((C, 8), -7.0, np.float32)
    u64 = [np.full(C, 7, np.uint64) for _ in range(5)]
    f32 = [np.full(C, -7.0, np.float32) for _ in range(2)]
    dist, totals = np.full(16, -7.0, np.float32), np.full(4, 7, np.uint64)
    labels = np.zeros(16, np.uint32)

    def call(h, c):
        return mi.mi_knn_sharded_summarize(h, labels.ctypes.data, c, cent.ctypes.data, u64[0].ctypes.data, u64[1].ctypes.data,
                                           f32[0].ctypes.data, u64[2].ctypes.data, f32[1].ctypes.data, u64[3].ctypes.data,
                                           u64[4].ctypes.data, dist.ctypes.data, totals.ctypes.data)

    fake = ctypes.c_void_p(16)          # a handle that is never followed: every case below is refused in front of it
    assert call(None, C) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert call(fake, 0) == MI_ERR_INVALID
    assert b"C must be" in mi.mi_last_error()
    assert call(fake, 65537) == MI_ERR_UNSUPPORTED
    assert b"65536" in mi.mi_last_error()
    assert call(fake, 0xFFFFFFFF) == MI_ERR_UNSUPPORTED
    out = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    assert mi.mi_knn_sharded_summarize_stats(None, out) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_summarize_stats(fake, None) == MI_ERR_INVALID
    assert list(out) == [7, 7, 7, 7]
    assert np.all(cent == -7.0) and all(np.all(a == 7) for a in u64) and all(np.all(a == -7.0) for a in f32)
    assert np.all(dist == -7.0) and np.all(totals == 7)


def test_host_rules_under_the_sanitizers(tmp_path):
    """tests/cpp/test_summary_sharded_host.cpp: a stand-alone program over csrc/summary_sharded_host.h — label dealing against
    cyclic_place, globalize then merge of per-shard slots in two shard orders against slots over the whole row set, the byte
    formula — built with the address and undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_summary_sharded_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_summary_sharded_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
