"""mi_knn_compact without a GPU: the host rules (csrc/compact_host.h: the old-to-new map, the chunk plan with its straight /
staged decision, the host columns) under the sanitizers, the ABI surface, and the argument errors that need no device."""
import ctypes
import os
import shutil
import subprocess

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi_knn_compact", "mi_knn_compact_stats", "mi_index_compact", "mi_knn_sharded_compact_into"]
MI_ERR_INVALID = -1


def test_host_rules_under_the_sanitizers(tmp_path):
    """tests/cpp/test_compact_host.cpp: a stand-alone program over csrc/compact_host.h — map, plan and columns against brute
    force for every dead pattern and S in {1, 64, rows, > rows}, and every plan replayed with adversarial write orders"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_compact_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_compact_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-4000:] + out.stderr[-4000:]


def test_header_library_and_bindings_name_the_same_four_symbols(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert "int " + name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert mi.mi_abi_version() == 4
    assert len(_lib.SYMBOLS["mi_knn_compact"][1]) == 4 and len(_lib.SYMBOLS["mi_knn_compact_stats"][1]) == 2
    assert len(_lib.SYMBOLS["mi_index_compact"][1]) == 4 and len(_lib.SYMBOLS["mi_knn_sharded_compact_into"][1]) == 5
    for cls, names in ((EmbeddingTable, ("compact", "compact_stats")), (ImageIndex, ("compact",)), (ShardedTable, ("compact_into",))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"compact.hip"' in build
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    assert "mi_knn_compact(" in hpp and "mi_knn_compact_stats(" in hpp


def test_null_handles_are_refused_before_any_device_work(mi):
    removed = ctypes.c_uint64(7)
    out = (ctypes.c_uint64 * 4)()
    assert mi.mi_knn_compact(None, None, 0, ctypes.byref(removed)) == MI_ERR_INVALID
    assert removed.value == 7
    assert mi.mi_knn_compact_stats(None, out) == MI_ERR_INVALID
    assert mi.mi_index_compact(None, None, 0, None) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_compact_into(None, None, None, 0, None) == MI_ERR_INVALID
