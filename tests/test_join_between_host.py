"""mi_knn_near_pairs_between, mi_knn_sharded_near_pairs and mi_index_matches without a GPU: the bindings, the argument rules
that are judged in front of a handle, and the host-only rules (csrc/join_between_host.h: the schedule of the shard pairs, the
rectangles of tiles, a shard's first_new, the column chunks) under the sanitizers.  What the calls compute:
tests/test_join_between_gpu.py."""
import ctypes
import inspect
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable

NEW = ["mi_knn_near_pairs_between", "mi_knn_near_pairs_between_stats", "mi_knn_sharded_near_pairs",
       "mi_knn_sharded_near_pairs_stats", "mi_index_matches"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID = -1


def test_symbols_are_declared_bound_and_named_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
        assert name + "(" in hpp, name
    assert mi.mi_abi_version() == 4
    assert len(_lib.SYMBOLS["mi_knn_near_pairs_between"][1]) == 8 and len(_lib.SYMBOLS["mi_knn_sharded_near_pairs"][1]) == 8
    assert len(_lib.SYMBOLS["mi_index_matches"][1]) == 8
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"join_between.hip"' in build


def defaults(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}


def params(fn):
    return list(inspect.signature(fn).parameters)


def test_python_signatures_and_defaults():
    assert params(EmbeddingTable.near_pairs_with) == ["self", "other", "max_dist", "cap"]
    assert defaults(EmbeddingTable.near_pairs_with) == {"cap": 1 << 20}
    assert params(EmbeddingTable.near_pairs_with_stats) == ["self"]
    assert params(ShardedTable.near_pairs) == ["self", "max_dist", "first_new", "cap"]
    assert defaults(ShardedTable.near_pairs) == {"first_new": 0, "cap": 1 << 20}
    assert params(ShardedTable.near_pairs_stats) == ["self"]
    assert params(ShardedTable.duplicates) == ["self", "max_dist", "first_new", "cap"]
    assert defaults(ShardedTable.duplicates) == {"first_new": 0, "cap": 1 << 20}
    assert params(ImageIndex.matches) == ["self", "other", "max_dist", "web", "max_pairs"]
    assert defaults(ImageIndex.matches) == {"web": False, "max_pairs": 1 << 20}
    # the single table's own join keeps its surface
    assert params(EmbeddingTable.near_pairs) == ["self", "max_dist", "first_new", "cap"]


def test_null_handles_and_bad_max_dist_return_codes_without_a_device(mi):
    a, b = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64)
    d = np.full(4, -7.0, np.float32)
    out = (a.ctypes.data, b.ctypes.data, d.ctypes.data, 4)
    fake, fake2 = ctypes.c_void_p(16), ctypes.c_void_p(32)   # handles that are never followed: every case is refused in front of them

    def refused(call):
        n = ctypes.c_uint64(7)
        assert call(ctypes.byref(n)) == MI_ERR_INVALID
        assert n.value == 0
        return mi.mi_last_error()

    for fn in (mi.mi_knn_near_pairs_between, mi.mi_index_matches):
        assert b"null" in refused(lambda n: fn(None, fake2, 0.1, *out, n))
        assert b"null" in refused(lambda n: fn(fake, None, 0.1, *out, n))
        assert b"same" in refused(lambda n: fn(fake, fake, 0.1, *out, n))
        for bad in (float("nan"), -0.5, float("-inf")):
            assert b"max_dist" in refused(lambda n: fn(fake, fake2, bad, *out, n))
        refused(lambda n: fn(fake, fake2, 0.1, None, b.ctypes.data, d.ctypes.data, 4, n))
        assert fn(fake, fake2, 0.1, *out, None) == MI_ERR_INVALID
    assert b"null" in refused(lambda n: mi.mi_knn_sharded_near_pairs(None, 0.1, 0, *out, n))
    for bad in (float("nan"), -0.5, float("-inf")):
        assert b"max_dist" in refused(lambda n: mi.mi_knn_sharded_near_pairs(fake, bad, 0, *out, n))
    refused(lambda n: mi.mi_knn_sharded_near_pairs(fake, 0.1, 0, a.ctypes.data, None, d.ctypes.data, 4, n))
    assert mi.mi_knn_sharded_near_pairs(fake, 0.1, 0, *out, None) == MI_ERR_INVALID
    stats = (ctypes.c_uint64 * 4)()
    assert mi.mi_knn_near_pairs_between_stats(None, stats) == MI_ERR_INVALID
    assert mi.mi_knn_near_pairs_between_stats(fake, None) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_near_pairs_stats(None, stats) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_near_pairs_stats(fake, None) == MI_ERR_INVALID
    assert np.all(a == 7) and np.all(b == 7) and np.all(d == -7.0)


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_join_between_host.cpp: a stand-alone program over csrc/join_between_host.h — the argument rules, the
    round-robin schedule (every shard pair once, no shard twice in a round, S = 1 .. 9), the rectangles of a (fn_a, fn_b) pair
    against a brute-force walk, the local first_new against an enumeration of the ids, the chunks that tile [0, n_b) — built
    with the address and undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_join_between_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_join_between_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
