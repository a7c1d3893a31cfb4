"""mi_knn_search_where and its kin without a GPU: the numpy restatement of the predicate (include/mi355clip.h) on hand-made
columns, the bindings, and the host-only rules (csrc/where_host.h) under the sanitizers.

The restatement works on the columns alone; the GPU tests (tests/test_where_gpu.py) compare the device's row lists with it for
equality."""
import ctypes
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable, make_where

NEW = ["mi_knn_set_attrs", "mi_knn_get_attrs", "mi_knn_count_where", "mi_knn_rows_where", "mi_knn_search_where",
       "mi_knn_sharded_set_attrs", "mi_knn_sharded_get_attrs", "mi_knn_sharded_count_where", "mi_knn_sharded_search_where",
       "mi_index_group_of", "mi_index_set_attrs", "mi_index_search_where"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID = -1
NO_GROUP = 0xFFFFFFFF
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BIT63 = 1 << 63


# ---- the restatement ------------------------------------------------------------------------------------------------

def where_rows(tags, stamps, groups, dead, where):
    """The rows a predicate keeps, ascending.  tags [n] uint64 / stamps [n] int64 (None: a table without attribute columns, every
    row 0 / 0); groups [n] uint32 or None (no group column); dead: the deleted rows; where: a dict with the fields of
    mi_knn_where that differ from "everything" (all_of, any_of, none_of, stamp_lo, stamp_hi, group)."""
    n = len(tags) if tags is not None else len(stamps) if stamps is not None else where["n"]
    tags = np.zeros(n, np.uint64) if tags is None else np.asarray(tags, np.uint64)
    stamps = np.zeros(n, np.int64) if stamps is None else np.asarray(stamps, np.int64)
    all_of, any_of, none_of = (np.uint64(where.get(f, 0)) for f in ("all_of", "any_of", "none_of"))
    ok = ((tags & all_of) == all_of) & ((tags & none_of) == 0)
    if any_of:
        ok &= (tags & any_of) != 0
    ok &= (stamps >= np.int64(where.get("stamp_lo", I64_MIN))) & (stamps <= np.int64(where.get("stamp_hi", I64_MAX)))
    if where.get("group") is not None:
        ok &= (np.asarray(groups, np.uint32) == np.uint32(where["group"])) if groups is not None else False
    ok[np.asarray(list(dead), np.int64)] = False
    return np.flatnonzero(ok).astype(np.uint64)


def as_kwargs(where):
    """the same dict as the keyword arguments of the Python surface (rows_where, knn_where, make_where)"""
    return dict(all_of=where.get("all_of", 0), any_of=where.get("any_of", 0), none_of=where.get("none_of", 0),
                stamp=(where.get("stamp_lo"), where.get("stamp_hi")), group=where.get("group"))


# ---- the restatement on hand-made columns -------------------------------------------------------------------------------

TAGS = np.array([0b000, 0b001, 0b010, 0b011, 0b100, 0b101, 0b110, 0b111], np.uint64)
STAMPS = np.array([-5, -1, 0, 1, 5, 10, 100, -100], np.int64)


def rows(where, tags=TAGS, stamps=STAMPS, groups=None, dead=()):
    return where_rows(tags, stamps, groups, dead, where).tolist()


def test_each_clause_alone():
    assert rows({}) == list(range(8))
    assert rows({"all_of": 0b011}) == [3, 7]
    assert rows({"any_of": 0b110}) == [2, 3, 4, 5, 6, 7]
    assert rows({"none_of": 0b101}) == [0, 2]
    assert rows({"stamp_lo": 0, "stamp_hi": 10}) == [2, 3, 4, 5]
    assert rows({"all_of": 0b001, "none_of": 0b100, "stamp_lo": 0}) == [3]
    assert rows({}, dead=(0, 7)) == list(range(1, 7))


def test_any_of_zero_is_no_clause_and_bit_63():
    assert rows({"any_of": 0}) == list(range(8))                 # not "no row has any of no bits"
    tags = np.array([0, BIT63, BIT63 | 1, 1, (1 << 64) - 1], np.uint64)
    z = np.zeros(5, np.int64)
    assert rows({"all_of": BIT63}, tags, z) == [1, 2, 4]
    assert rows({"any_of": BIT63}, tags, z) == [1, 2, 4]
    assert rows({"none_of": BIT63}, tags, z) == [0, 3]
    assert rows({"all_of": BIT63 | 1}, tags, z) == [2, 4]
    assert rows({"all_of": (1 << 64) - 1}, tags, z) == [4]


def test_negative_stamps_and_the_64_bit_extremes():
    stamps = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], np.int64)
    tags = np.zeros(7, np.uint64)
    assert rows({}, tags, stamps) == list(range(7))
    assert rows({"stamp_lo": I64_MIN, "stamp_hi": I64_MIN}, tags, stamps) == [0]
    assert rows({"stamp_lo": I64_MIN + 1}, tags, stamps) == [1, 2, 3, 4, 5, 6]
    assert rows({"stamp_hi": -1}, tags, stamps) == [0, 1, 2]                  # signed: the negatives are below, not above
    assert rows({"stamp_lo": 0}, tags, stamps) == [3, 4, 5, 6]
    assert rows({"stamp_lo": I64_MAX}, tags, stamps) == [6]
    assert rows({"stamp_hi": I64_MAX - 1}, tags, stamps) == [0, 1, 2, 3, 4, 5]
    assert rows({"stamp_lo": 1, "stamp_hi": 0}, tags, stamps) == []             # lo > hi
    assert rows({"stamp_lo": I64_MAX, "stamp_hi": I64_MIN}, tags, stamps) == []


def test_the_group_flag():
    groups = np.array([0, 1, NO_GROUP, 1, 2, NO_GROUP, 1, 0], np.uint32)
    assert rows({"group": 1}, groups=groups) == [1, 3, 6]
    assert rows({"group": 1, "all_of": 0b010}, groups=groups) == [3, 6]
    assert rows({"group": NO_GROUP}, groups=groups) == [2, 5]                   # NO_GROUP as the value: the rows without one
    assert rows({"group": 7}, groups=groups) == []
    assert rows({"group": 1}, groups=None) == []                                # no column: nothing, whatever the value
    assert rows({"group": NO_GROUP}, groups=None) == []
    assert rows({"group": 1}, groups=groups, dead=(3,)) == [1, 6]


def test_a_table_without_attribute_columns_holds_the_defaults():
    assert where_rows(None, None, None, (), {"n": 4}).tolist() == [0, 1, 2, 3]
    assert where_rows(None, None, None, (1,), {"n": 4, "stamp_lo": 0, "stamp_hi": 0, "none_of": 5}).tolist() == [0, 2, 3]
    assert where_rows(None, None, None, (), {"n": 4, "all_of": 1}).tolist() == []
    assert where_rows(None, None, None, (), {"n": 4, "stamp_lo": 1}).tolist() == []


def test_make_where_fills_the_structure():
    w = make_where()
    assert (w.all_of, w.any_of, w.none_of, w.stamp_lo, w.stamp_hi, w.flags) == (0, 0, 0, I64_MIN, I64_MAX, 0)
    w = make_where(all_of=BIT63 | 1, any_of=6, none_of=8, stamp=(-3, None), group=NO_GROUP)
    assert (w.all_of, w.any_of, w.none_of, w.stamp_lo, w.stamp_hi, w.group, w.flags) == (BIT63 | 1, 6, 8, -3, I64_MAX, NO_GROUP, 1)
    assert ctypes.sizeof(_lib.KnnWhere) == 48


# ---- the bindings -----------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert "#define MI_KNN_WHERE_GROUP 1u" in header and "typedef struct mi_knn_where {" in header
    assert mi.mi_abi_version() == 4
    args = _lib.SYMBOLS["mi_knn_search_where"][1]
    assert len(args) == 8 and args[4] == _lib.c_wherep and _lib.SYMBOLS["mi_knn_sharded_search_where"][1] == args
    for cls, names in ((EmbeddingTable, ("set_attrs", "get_attrs", "count_where", "rows_where", "knn_where")),
                       (ShardedTable, ("set_attrs", "get_attrs", "count_where", "rows_where", "knn_where")),
                       (ImageIndex, ("set_attrs", "web_search_where", "group_of"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in ("mi_knn_search_where(", "mi_knn_sharded_search_where(", "mi_index_search_where(", "mi_knn_set_attrs(", "mi_knn_rows_where("):
        assert name in hpp, name
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"where.hip"' in build


def test_null_handles_and_bad_arguments_return_codes_without_a_device(mi):
    v = np.zeros(768, np.float32)
    idx, dist = np.full(4, 7, np.uint64), np.full(4, -7.0, np.float32)
    ids, tags, stamps = np.zeros(3, np.uint64), np.full(3, 7, np.uint64), np.full(3, 7, np.int64)
    n, g, found = ctypes.c_uint64(7), ctypes.c_uint32(7), ctypes.c_uint32(7)
    w = make_where()
    for fn in (mi.mi_knn_set_attrs, mi.mi_knn_get_attrs, mi.mi_knn_sharded_set_attrs, mi.mi_knn_sharded_get_attrs):
        assert fn(None, ids.ctypes.data, 3, tags.ctypes.data, stamps.ctypes.data) == MI_ERR_INVALID
    for fn in (mi.mi_knn_count_where, mi.mi_knn_sharded_count_where):
        assert fn(None, ctypes.byref(w), ctypes.byref(n)) == MI_ERR_INVALID
    assert mi.mi_knn_rows_where(None, ctypes.byref(w), ids.ctypes.data, 3, ctypes.byref(n)) == MI_ERR_INVALID
    for fn in (mi.mi_knn_search_where, mi.mi_knn_sharded_search_where):
        assert fn(None, v.ctypes.data, 1, 4, ctypes.byref(w), idx.ctypes.data, dist.ctypes.data, ctypes.byref(n)) == MI_ERR_INVALID
    assert mi.mi_index_group_of(None, b"media/", ctypes.byref(g)) == MI_ERR_INVALID
    assert mi.mi_index_set_attrs(None, None, 0, None, None) == MI_ERR_INVALID
    assert mi.mi_index_search_where(None, v.ctypes.data, None, 0, 4, ctypes.byref(w), idx.ctypes.data, dist.ctypes.data,
                                    ctypes.byref(found), ctypes.byref(n)) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert np.all(idx == 7) and np.all(dist == -7.0) and np.all(tags == 7) and np.all(stamps == 7)
    assert n.value == 7 and g.value == 7 and found.value == 7


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_where_host.cpp: a stand-alone program over csrc/where_host.h — the argument checks (unknown flags, null
    pointers, the k limits), the predicate on one row against hand cases, the "where_chunk" rule — built with the address and
    undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_where_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_where_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
