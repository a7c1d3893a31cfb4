"""mi_knn_search_page without a GPU: the numpy restatement of the contract (include/mi355clip.h) on hand-made distance
arrays, the bindings, and the host-only rules (csrc/page_host.h) under the sanitizers.

The restatement works on one distance array alone; the GPU tests (tests/test_page_gpu.py) feed it the CPU oracle's
orc_cosine_dist(q, rows) and compare the device's ids, distance bits and counts with it for equality."""
import ctypes
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable

NEW = ["mi_knn_search_page", "mi_knn_sharded_search_page", "mi_index_search_page"]
NO_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID = -1
INF = np.float32(np.inf)


# ---- the restatement ------------------------------------------------------------------------------------------------

def dist_key(d):
    """dist_to_u32: numeric order, -0 before +0, every NaN last and equal"""
    d = np.asarray(d, np.float32)
    b = d.view(np.uint32)
    return np.where(np.isnan(d), np.uint32(0xFFFFFFFF), np.where(b >> 31 == 1, ~b, b | np.uint32(0x80000000))).astype(np.uint32)


def key_dist(key):
    """u32_to_dist"""
    key = np.asarray(key, np.uint32)
    return np.where(key >> 31 == 1, key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32).view(np.float32)


def expected_page(d, ids, k, after=None, max_dist=INF):
    """d [n]: every candidate's distance; ids [n]: its id (ids order as the local rows do).  after: None or (dist, id).
    -> idx [k], dist [k], counts {before, window, beyond, nan}"""
    d, ids = np.asarray(d, np.float32).reshape(-1), np.asarray(ids, np.uint64).reshape(-1)
    dk = dist_key(d)
    past = np.ones(ids.size, bool)
    if after is not None:                                    # key > cursor key, the id breaking ties
        ck = dist_key(np.float32(after[0]))
        past = (dk > ck) | ((dk == ck) & (ids > np.uint64(after[1])))
    within = dk <= dist_key(np.float32(max_dist))            # inclusive, on the key order; a NaN key is above every bound
    window = past & within
    nan = past & ~within & (dk == 0xFFFFFFFF)
    beyond = past & ~within & ~nan
    cand = np.flatnonzero(window)
    order = cand[np.lexsort((ids[cand], dk[cand]))][:k]
    idx, dist = np.full(k, NO_ID, np.uint64), np.full(k, np.inf, np.float32)
    idx[:order.size], dist[:order.size] = ids[order], key_dist(dk[order])
    return idx, dist, {"before": int((~past).sum()), "window": int(window.sum()), "beyond": int(beyond.sum()), "nan": int(nan.sum())}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def total(c):
    return c["before"] + c["window"] + c["beyond"] + c["nan"]


# ---- the restatement on hand-made arrays ------------------------------------------------------------------------------

def test_key_transform_orders_and_round_trips():
    d = np.array([-np.inf, -1.5, -0.0, 0.0, 1e-45, 0.25, 2.0, np.inf, np.nan], np.float32)
    k = dist_key(d)
    assert np.all(np.diff(k.astype(np.int64)) > 0)          # strictly ascending, -0 before +0, NaN last
    assert k[-1] == 0xFFFFFFFF and dist_key(np.float32(-np.nan)) == 0xFFFFFFFF
    assert np.array_equal(bits(key_dist(k[:-1])), bits(d[:-1]))


def test_minus_zero_against_plus_zero_at_the_cursor_and_at_the_bound():
    ids = np.arange(4, dtype=np.uint64)
    d = np.array([0.0, -0.0, 0.0, -0.0], np.float32)
    idx, dist, c = expected_page(d, ids, 4)
    assert idx.tolist() == [1, 3, 0, 2] and bits(dist).tolist() == [0x80000000, 0x80000000, 0, 0]
    # the cursor (-0, 3) leaves both +0 rows; the cursor (+0, 3) — the same id under the other zero — leaves none:
    # rows 0 and 2 sit at or below id 3 of that distance
    idx, dist, c = expected_page(d, ids, 4, after=(np.float32(-0.0), 3))
    assert idx.tolist() == [0, 2, int(NO_ID), int(NO_ID)] and c == {"before": 2, "window": 2, "beyond": 0, "nan": 0}
    idx, dist, c = expected_page(d, ids, 4, after=(np.float32(0.0), 3))
    assert np.all(idx == NO_ID) and c == {"before": 4, "window": 0, "beyond": 0, "nan": 0}
    idx, dist, c = expected_page(d, ids, 4, after=(np.float32(0.0), 1))
    assert idx.tolist() == [2, int(NO_ID), int(NO_ID), int(NO_ID)] and c["before"] == 3
    # the bound -0 takes the -0 rows alone, the bound +0 takes all four
    idx, dist, c = expected_page(d, ids, 4, max_dist=np.float32(-0.0))
    assert idx.tolist() == [1, 3, int(NO_ID), int(NO_ID)] and c == {"before": 0, "window": 2, "beyond": 2, "nan": 0}
    assert expected_page(d, ids, 4, max_dist=np.float32(0.0))[2]["window"] == 4


def test_a_tie_group_cut_by_the_cursor():
    ids = np.array([3, 5, 7, 9, 11, 13], np.uint64)
    d = np.array([0.5, 0.25, 0.5, 0.5, 0.75, 0.5], np.float32)
    full = expected_page(d, ids, 6)[0]
    assert full.tolist() == [5, 3, 7, 9, 13, 11]
    idx, dist, c = expected_page(d, ids, 2, after=(np.float32(0.5), 7))       # inside the group: the rest of it opens the page
    assert idx.tolist() == [9, 13] and np.array_equal(bits(dist), bits([0.5, 0.5])) and c == {"before": 3, "window": 3, "beyond": 0, "nan": 0}
    idx, dist, c = expected_page(d, ids, 2, after=(np.float32(0.5), 8))       # the cursor's row is gone: the same page
    assert idx.tolist() == [9, 13] and c["before"] == 3
    idx, dist, c = expected_page(d, ids, 2, after=(np.float32(0.5), 13))
    assert idx.tolist() == [11, int(NO_ID)] and np.isinf(dist[1]) and c["before"] == 5


def test_a_row_at_max_dist_and_one_below():
    ids = np.arange(4, dtype=np.uint64)
    at = np.float32(0.3)
    d = np.array([0.1, at, np.nextafter(at, np.float32(1)), 0.2], np.float32)
    idx, dist, c = expected_page(d, ids, 4, max_dist=at)                       # inclusive
    assert idx.tolist() == [0, 3, 1, int(NO_ID)] and c == {"before": 0, "window": 3, "beyond": 1, "nan": 0}
    idx, dist, c = expected_page(d, ids, 4, max_dist=np.nextafter(at, np.float32(0)))
    assert idx.tolist() == [0, 3, int(NO_ID), int(NO_ID)] and c == {"before": 0, "window": 2, "beyond": 2, "nan": 0}
    idx, dist, c = expected_page(d, ids, 4, max_dist=-np.inf)
    assert np.all(idx == NO_ID) and c["beyond"] == 4


def test_a_nan_distance_is_counted_and_never_returned():
    ids = np.arange(5, dtype=np.uint64)
    d = np.array([0.4, np.nan, 0.1, np.nan, np.inf], np.float32)
    idx, dist, c = expected_page(d, ids, 5)
    assert idx.tolist() == [2, 0, 4, int(NO_ID), int(NO_ID)] and c == {"before": 0, "window": 3, "beyond": 0, "nan": 2}
    assert np.isinf(dist[2]) and np.all(np.isinf(dist[3:]))
    idx, dist, c = expected_page(d, ids, 5, after=(np.float32(0.1), 2), max_dist=np.float32(1.0))
    assert idx.tolist() == [0] + [int(NO_ID)] * 4 and c == {"before": 1, "window": 1, "beyond": 1, "nan": 2}


def test_a_cursor_past_the_bound_k_beyond_the_hits_and_counts_that_add_up():
    rng = np.random.default_rng(7)
    ids = np.arange(200, dtype=np.uint64) * 3
    d = rng.random(200).astype(np.float32)
    d[[5, 77]] = np.nan
    d[100:110] = d[20]
    idx, dist, c = expected_page(d, ids, 10, after=(np.float32(0.9), 60), max_dist=np.float32(0.5))   # a cursor past the bound
    assert np.all(idx == NO_ID) and c["window"] == 0 and c["before"] == int((d < 0.9).sum() + ((d == np.float32(0.9)) & (ids <= 60)).sum())
    assert total(c) == 200
    idx, dist, c = expected_page(d, ids, 4096)                                                            # k beyond the hits
    assert int((idx != NO_ID).sum()) == 198 == c["window"] and np.all(np.isinf(dist[198:])) and total(c) == 200
    # pages of any size concatenate to the full list; before = what was delivered
    full = idx[:198]
    for size in (1, 7, 64, 198, 500):
        got, after = [], None
        while True:
            idx, dist, c = expected_page(d, ids, size, after=after, max_dist=np.float32(2.0))
            assert c["before"] == len(got) and total(c) == 200
            n = int((idx != NO_ID).sum())
            got += idx[:n].tolist()
            if n < size:
                break
            after = (dist[size - 1], idx[size - 1])
        assert got == full.tolist(), size


# ---- the bindings -----------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    args = _lib.SYMBOLS["mi_knn_search_page"][1]
    assert len(args) == 11 and args[2:6] == [ctypes.c_uint32, ctypes.c_float, ctypes.c_uint64, ctypes.c_float]
    assert _lib.SYMBOLS["mi_knn_sharded_search_page"][1] == args and len(_lib.SYMBOLS["mi_index_search_page"][1]) == 14
    assert mi.mi_abi_version() == 4
    for cls, names in ((EmbeddingTable, ("knn_page", "pages")), (ShardedTable, ("knn_page",)), (ImageIndex, ("web_search_page",))):
        for name in names:
            assert callable(getattr(cls, name)), name
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    assert "mi_knn_search_page(" in hpp and "mi_knn_sharded_search_page(" in hpp and "mi_index_search_page(" in hpp


def test_a_null_handle_is_invalid_without_a_device(mi):
    v = np.zeros(768, np.float32)
    idx, dist = np.full(4, 7, np.uint64), np.full(4, -7.0, np.float32)
    counts = np.full(4, 7, np.uint64)
    no = int(NO_ID)
    rc = mi.mi_knn_search_page(None, v.ctypes.data, 4, 0.0, no, np.inf, None, 0, idx.ctypes.data, dist.ctypes.data, counts.ctypes.data)
    assert rc == MI_ERR_INVALID and np.all(idx == 7) and np.all(dist == -7.0) and np.all(counts == 7)
    assert mi.mi_knn_sharded_search_page(None, v.ctypes.data, 4, 0.0, no, np.inf, None, 0, idx.ctypes.data, dist.ctypes.data, None) == MI_ERR_INVALID
    assert mi.mi_index_search_page(None, v.ctypes.data, None, 0, None, 0, 4, 0.0, no, np.inf, idx.ctypes.data, dist.ctypes.data, None,
                                   None) == MI_ERR_INVALID


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_page_host.cpp: a stand-alone program over csrc/page_host.h, built with the address and
    undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_page_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_page_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
