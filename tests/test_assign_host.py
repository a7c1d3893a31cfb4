"""mi_knn_assign / mi_knn_kmeans / mi_knn_sharded_assign without a GPU: the bindings, the argument checks that need no
handle, and the pure parts of the Python helpers."""
import ctypes
import inspect

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import (NO_LABEL, EmbeddingTable, ImageIndex, ShardedTable, clusters_of,
                                     initial_centroid_rows)

NEW = ["mi_knn_assign", "mi_knn_assign_stats", "mi_knn_kmeans", "mi_knn_sharded_assign"]
MI_ERR_INVALID = -1


def test_new_symbols_are_bound_and_exported(mi):
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert _lib.SYMBOLS["mi_knn_kmeans"][1][-1] == ctypes.POINTER(ctypes.c_double)
    assert mi.mi_abi_version() == 4


def test_python_surface():
    for cls, names in ((EmbeddingTable, ("assign", "assign_stats", "kmeans")), (ShardedTable, ("assign",)),
                       (ImageIndex, ("label", "clusters"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    p = inspect.signature(EmbeddingTable.kmeans).parameters
    assert p["max_iters"].default == 20 and p["seed"].default == 0
    p = inspect.signature(ImageIndex.clusters).parameters
    assert p["max_iters"].default == 20 and p["seed"].default == 0 and p["web"].default is False
    assert int(NO_LABEL) == 0xFFFFFFFF


def test_null_handles_are_refused_without_a_device(mi):
    v = np.zeros((2, 768), np.float32)
    lab, d = np.zeros(4, np.uint32), np.zeros(4, np.float32)
    out = (ctypes.c_uint64 * 4)()
    assert mi.mi_knn_assign(None, v.ctypes.data, 2, lab.ctypes.data, d.ctypes.data) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert mi.mi_knn_assign_stats(None, out) == MI_ERR_INVALID
    it, ch, obj = ctypes.c_uint32(7), ctypes.c_uint64(7), ctypes.c_double(7.0)
    assert mi.mi_knn_kmeans(None, v.ctypes.data, 2, 3, lab.ctypes.data, d.ctypes.data, ctypes.byref(it), ctypes.byref(ch),
                            ctypes.byref(obj)) == MI_ERR_INVALID
    assert (it.value, ch.value, obj.value) == (0, 0, 0.0)
    assert mi.mi_knn_sharded_assign(None, v.ctypes.data, 2, lab.ctypes.data, d.ctypes.data) == MI_ERR_INVALID


def test_initial_centroids_are_seeded_distinct_live_rows():
    dead = [3, 4, 5, 99]
    a = initial_centroid_rows(100, dead, 40, seed=1)
    assert a.size == 40 and np.unique(a).size == 40 and not np.any(np.isin(a, dead))
    assert np.all(a[:-1] < a[1:]) and a.max() < 100
    assert np.array_equal(a, initial_centroid_rows(100, dead, 40, seed=1))
    assert not np.array_equal(a, initial_centroid_rows(100, dead, 40, seed=2))
    assert np.array_equal(initial_centroid_rows(100, dead, 96), np.setdiff1d(np.arange(100), dead))   # every live row
    for k in (0, 97):
        with pytest.raises(ValueError):
            initial_centroid_rows(100, dead, k)


def test_cluster_lists_largest_first():
    labels = np.array([2, 0, 2, NO_LABEL, 1, 2, 0, 1, 7], np.uint32)
    keys = list("abcdefghi")
    assert clusters_of(labels, keys) == [["a", "c", "f"], ["b", "g"], ["e", "h"], ["i"]]
    assert clusters_of(np.array([], np.uint32), []) == []
