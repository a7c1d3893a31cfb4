"""The threshold self-join without a GPU: the entry points are declared and bound, mi_pairs_to_groups (host-only) groups
pairs into connected components, and the argument checks that need no device answer MI_ERR_INVALID instead of aborting."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from image_search_amd import _lib
from image_search_amd import search
from image_search_amd.search import EmbeddingTable, ImageIndex, pairs_to_groups

NEW = ["mi_knn_near_pairs", "mi_knn_near_pairs_stats", "mi_pairs_to_groups", "mi_index_duplicates"]
MI_ERR_INVALID = -1


def test_join_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["mi_knn_near_pairs"][1][1] is ctypes.c_float
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in NEW:
        assert name in hpp, name


def test_python_mirrors_exist_with_the_documented_defaults():
    p = inspect.signature(EmbeddingTable.near_pairs).parameters
    assert list(p)[:4] == ["self", "max_dist", "first_new", "cap"]
    assert p["first_new"].default == 0 and p["cap"].default == 1 << 20
    assert hasattr(EmbeddingTable, "near_pairs_stats")
    p = inspect.signature(ImageIndex.duplicates).parameters
    assert list(p)[:4] == ["self", "max_dist", "first_new", "web"]
    assert p["first_new"].default == 0 and p["web"].default is False
    assert callable(search.pairs_to_groups)


def groups(a, b):
    return [[int(i) for i in g] for g in pairs_to_groups(a, b)]


def test_groups_chain_into_one_component(mi):
    assert groups([0, 1], [1, 2]) == [[0, 1, 2]]
    # a chain given back to front and out of order still is one group, ids ascending
    assert groups([7, 3, 5], [9, 5, 7]) == [[3, 5, 7, 9]]


def test_two_groups_are_ordered_by_their_smallest_id(mi):
    assert groups([10, 2, 11], [12, 40, 12]) == [[2, 40], [10, 11, 12]]


def test_duplicate_and_reversed_pairs_change_nothing(mi):
    assert groups([1, 2, 1, 2, 8], [2, 1, 2, 1, 6]) == [[1, 2], [6, 8]]


def test_no_pairs_no_groups(mi):
    assert groups([], []) == []
    n_ids, n_groups = ctypes.c_uint64(7), ctypes.c_uint64(7)
    start = np.full(1, 99, np.uint64)
    assert mi.mi_pairs_to_groups(None, None, 0, None, 0, start.ctypes.data, 1, ctypes.byref(n_ids), ctypes.byref(n_groups)) == 0
    assert (n_ids.value, n_groups.value) == (0, 0)
    assert start[0] == 0   # group_start holds n_groups + 1 entries: the single 0


def test_caps_smaller_than_the_result_keep_the_counts_and_the_bounds(mi):
    a = np.array([0, 1, 10, 20], np.uint64)
    b = np.array([1, 2, 11, 21], np.uint64)   # [0 1 2] [10 11] [20 21]: 7 ids, 3 groups, 4 start entries
    n_ids, n_groups = ctypes.c_uint64(), ctypes.c_uint64()
    ids = np.full(8, 777, np.uint64)
    start = np.full(8, 777, np.uint64)
    rc = mi.mi_pairs_to_groups(a.ctypes.data, b.ctypes.data, 4, ids.ctypes.data, 4, start.ctypes.data, 2, ctypes.byref(n_ids),
                               ctypes.byref(n_groups))
    assert rc == 0 and (n_ids.value, n_groups.value) == (7, 3)
    assert ids.tolist() == [0, 1, 2, 10, 777, 777, 777, 777]
    assert start.tolist() == [0, 3, 777, 777, 777, 777, 777, 777]
    # the first call of the two-call protocol: no arrays at all
    rc = mi.mi_pairs_to_groups(a.ctypes.data, b.ctypes.data, 4, None, 0, None, 0, ctypes.byref(n_ids), ctypes.byref(n_groups))
    assert rc == 0 and (n_ids.value, n_groups.value) == (7, 3)
    # ... and the second with exact caps
    rc = mi.mi_pairs_to_groups(a.ctypes.data, b.ctypes.data, 4, ids.ctypes.data, 7, start.ctypes.data, 4, ctypes.byref(n_ids),
                               ctypes.byref(n_groups))
    assert rc == 0 and ids[:7].tolist() == [0, 1, 2, 10, 11, 20, 21] and ids[7] == 777
    assert start[:4].tolist() == [0, 3, 5, 7] and start[4] == 777


def test_ids_near_two_to_the_63(mi):
    big = 1 << 63
    assert groups([big + 5, big - 1, 3], [big + 6, big + 5, big + 7]) == [[3, big + 7], [big - 1, big + 5, big + 6]]


def test_null_arguments_of_pairs_to_groups_are_invalid(mi):
    a = np.array([0], np.uint64)
    n = ctypes.c_uint64()
    assert mi.mi_pairs_to_groups(a.ctypes.data, a.ctypes.data, 1, None, 0, None, 0, None, ctypes.byref(n)) == MI_ERR_INVALID
    assert mi.mi_pairs_to_groups(None, a.ctypes.data, 1, None, 0, None, 0, ctypes.byref(n), ctypes.byref(n)) == MI_ERR_INVALID
    assert mi.mi_pairs_to_groups(a.ctypes.data, a.ctypes.data, 1, None, 4, None, 0, ctypes.byref(n), ctypes.byref(n)) == MI_ERR_INVALID


@pytest.mark.parametrize("max_dist", [float("nan"), -0.01, -float("inf")])
def test_join_argument_checks_need_no_device(mi, max_dist):
    n = ctypes.c_uint64(5)
    # no handle: invalid whatever else is passed, and nothing aborts
    assert mi.mi_knn_near_pairs(None, 0.1, 0, None, None, None, 0, ctypes.byref(n)) == MI_ERR_INVALID
    assert mi.mi_knn_near_pairs(None, max_dist, 0, None, None, None, 0, ctypes.byref(n)) == MI_ERR_INVALID
    assert n.value == 0
    assert b"max_dist" in mi.mi_last_error() or b"null" in mi.mi_last_error()
    out = (ctypes.c_uint64 * 4)()
    assert mi.mi_knn_near_pairs_stats(None, out) == MI_ERR_INVALID
    assert mi.mi_index_duplicates(None, max_dist, 0, 10, None, 0, None, 0, ctypes.byref(n), ctypes.byref(n)) == MI_ERR_INVALID
