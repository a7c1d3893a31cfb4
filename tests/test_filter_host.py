"""Filtered search without a GPU: the four entry points are declared in the header and bound in _lib, and the Python
methods take the new keyword arguments (None keeps today's call)."""
import inspect
import os
import re

from conftest import ROOT
from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable

NEW = ["mi_knn_search_filtered", "mi_knn_sharded_search_filtered", "mi_index_search_within"]


def test_filter_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert name in _lib.SYMBOLS, name
    # (the ids arrive as a pointer and a u64 count: a table's filter may hold more than 2^32 ids over all shards)
    assert _lib.SYMBOLS["mi_knn_search_filtered"][1][5] is _lib.ctypes.c_uint64
    assert _lib.SYMBOLS["mi_knn_sharded_search_filtered"][1][5] is _lib.ctypes.c_uint64


def test_python_methods_take_the_filter_keywords():
    for cls in (EmbeddingTable, ShardedTable):
        p = inspect.signature(cls.knn).parameters
        assert "within" in p and p["within"].default is None, cls
    p = inspect.signature(ImageIndex.web_search_text).parameters
    assert list(p)[:4] == ["self", "text_embedding", "referenced_images", "k"]
    assert "folders" in p and p["folders"].default is None

