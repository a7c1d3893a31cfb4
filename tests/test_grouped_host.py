"""mi_knn_search_grouped without a GPU: the numpy restatement of the contract (include/mi355clip.h) on hand-made distance
arrays, the bindings, and the host-only rules (csrc/grouped_host.h) under the sanitizers.

The restatement works on one distance array and one group array alone; the GPU tests (tests/test_grouped_gpu.py) feed it the
CPU oracle's orc_cosine_dist(q, rows) and compare the device's ids, distance bits, groups, members, facets and totals with it
for equality."""
import ctypes
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable
from test_page_host import INF, NO_ID, bits, dist_key, expected_page, key_dist

NEW = ["mi_knn_set_groups", "mi_knn_get_groups", "mi_knn_groups_info", "mi_knn_search_grouped", "mi_knn_sharded_set_groups",
       "mi_knn_sharded_get_groups", "mi_knn_sharded_groups_info", "mi_knn_sharded_search_grouped", "mi_index_search_grouped",
       "mi_index_group_name", "mi_index_group_count"]
NO_GROUP = np.uint32(0xFFFFFFFF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID = -1
NG, NI = int(NO_GROUP), int(NO_ID)


# ---- the restatement ------------------------------------------------------------------------------------------------

def expected_grouped(d, ids, groups, k, max_dist=INF, n_groups=None):
    """d [n]: every candidate's distance; ids [n]: its id; groups [n]: its group or NO_GROUP.
    -> idx [k], dist [k], group [k], members [k], facets [n_groups], totals {groups, window, beyond, nan}"""
    d, ids = np.asarray(d, np.float32).reshape(-1), np.asarray(ids, np.uint64).reshape(-1)
    groups = np.asarray(groups, np.uint32).reshape(-1)
    if n_groups is None:
        n_groups = int(groups[groups != NO_GROUP].max()) + 1 if np.any(groups != NO_GROUP) else 0
    dk = dist_key(d)
    window = dk <= dist_key(np.float32(max_dist))             # inclusive, on the key order; a NaN key is above every bound
    nan = ~window & (dk == 0xFFFFFFFF)
    facets = np.bincount(groups[window & (groups != NO_GROUP)], minlength=n_groups).astype(np.uint64)
    cand = np.flatnonzero(window)
    order = cand[np.lexsort((ids[cand], dk[cand]))]           # the key order: distance word, then id
    first = np.ones(order.size, bool)                          # a group's first row in that order is its representative
    _, where = np.unique(groups[order], return_index=True)
    first[:] = groups[order] == NO_GROUP
    first[where] = True
    reps = order[first]
    top = reps[:k]
    idx, dist = np.full(k, NO_ID, np.uint64), np.full(k, np.inf, np.float32)
    group, members = np.full(k, NO_GROUP, np.uint32), np.zeros(k, np.uint64)
    idx[:top.size], dist[:top.size], group[:top.size] = ids[top], key_dist(dk[top]), groups[top]
    members[:top.size] = [1 if g == NO_GROUP else facets[g] for g in groups[top]]
    totals = {"groups": int(reps.size), "window": int(window.sum()), "beyond": int((~window & ~nan).sum()), "nan": int(nan.sum())}
    return idx, dist, group, members, facets, totals


def pad(values, k, fill):
    return list(values) + [fill] * (k - len(values))


# ---- the restatement on hand-made arrays ------------------------------------------------------------------------------

def test_ties_inside_a_group_and_between_groups_go_to_the_lower_id():
    ids = np.array([3, 5, 7, 9, 11, 13], np.uint64)
    d = np.array([0.5, 0.5, 0.5, 0.5, 0.25, 0.5], np.float32)
    groups = np.array([1, 0, 1, 0, 2, NG], np.uint32)
    idx, dist, group, members, facets, totals = expected_grouped(d, ids, groups, 4)
    # group 2 leads; groups 1 and 0 tie at 0.5: group 1 holds the lower id (3 before 5); inside each the lower id stands
    assert idx.tolist() == [11, 3, 5, 13] and group.tolist() == [2, 1, 0, NG] and members.tolist() == [1, 2, 2, 1]
    assert np.array_equal(bits(dist), bits([0.25, 0.5, 0.5, 0.5])) and facets.tolist() == [2, 2, 1]
    assert totals == {"groups": 4, "window": 6, "beyond": 0, "nan": 0}
    assert expected_grouped(d, ids, groups, 2)[0].tolist() == [11, 3]


def test_minus_zero_against_plus_zero():
    ids = np.arange(4, dtype=np.uint64)
    d = np.array([0.0, -0.0, 0.0, -0.0], np.float32)
    idx, dist, group, members, facets, totals = expected_grouped(d, ids, [0, 1, 1, 0], 3)
    # -0 sorts before +0: row 1 stands for group 1, row 3 for group 0, whatever their ids
    assert idx.tolist() == [1, 3, NI] and group.tolist() == [1, 0, NG] and bits(dist).tolist() == [0x80000000, 0x80000000, 0x7F800000]
    assert members.tolist() == [2, 2, 0]
    idx, dist, group, members, facets, totals = expected_grouped(d, ids, [0, 1, 1, 0], 3, max_dist=np.float32(-0.0))
    assert idx.tolist() == [1, 3, NI] and members.tolist() == [1, 1, 0] and totals == {"groups": 2, "window": 2, "beyond": 2, "nan": 0}
    assert expected_grouped(d, ids, [0, 0, 0, 0], 3, max_dist=np.float32(0.0))[3].tolist() == [4, 0, 0]


def test_a_row_at_max_dist_and_one_key_below():
    ids = np.arange(5, dtype=np.uint64)
    at = np.float32(0.3)
    d = np.array([0.1, at, np.nextafter(at, np.float32(1)), 0.2, at], np.float32)
    groups = np.array([0, 1, 1, 0, 2], np.uint32)
    idx, dist, group, members, facets, totals = expected_grouped(d, ids, groups, 4, max_dist=at)          # inclusive
    assert idx.tolist() == [0, 1, 4, NI] and members.tolist() == [2, 1, 1, 0] and facets.tolist() == [2, 1, 1]
    assert totals == {"groups": 3, "window": 4, "beyond": 1, "nan": 0}
    idx, dist, group, members, facets, totals = expected_grouped(d, ids, groups, 4, max_dist=np.nextafter(at, np.float32(0)))
    assert idx.tolist() == [0, NI, NI, NI] and facets.tolist() == [2, 0, 0] and totals == {"groups": 1, "window": 2, "beyond": 3, "nan": 0}
    idx, dist, group, members, facets, totals = expected_grouped(d, ids, groups, 2, max_dist=-np.inf)
    assert np.all(idx == NO_ID) and np.all(members == 0) and totals == {"groups": 0, "window": 0, "beyond": 5, "nan": 0}


def test_nan_rows_are_counted_and_never_stand_for_or_belong_to_a_group():
    ids = np.arange(6, dtype=np.uint64)
    d = np.array([np.nan, 0.4, np.nan, 0.1, np.nan, np.inf], np.float32)
    groups = np.array([0, 0, 1, NG, NG, 2], np.uint32)
    idx, dist, group, members, facets, totals = expected_grouped(d, ids, groups, 6)
    assert idx.tolist() == [3, 1, 5, NI, NI, NI] and group.tolist() == [NG, 0, 2, NG, NG, NG]
    assert members.tolist() == [1, 1, 1, 0, 0, 0] and facets.tolist() == [1, 0, 1]                       # group 1 holds a NaN row alone
    assert totals == {"groups": 3, "window": 3, "beyond": 0, "nan": 3} and np.isinf(dist[2])
    assert expected_grouped(d, ids, groups, 6, max_dist=np.float32(1.0))[5] == {"groups": 2, "window": 2, "beyond": 1, "nan": 3}


def test_singletons_among_grouped_rows_and_k_beyond_the_groups():
    ids = np.array([10, 11, 12, 13, 14, 15, 16], np.uint64)
    d = np.array([0.7, 0.2, 0.3, 0.2, 0.9, 0.6, 0.1], np.float32)
    groups = np.array([NG, 4, NG, 4, 4, NG, 1], np.uint32)
    idx, dist, group, members, facets, totals = expected_grouped(d, ids, groups, 8)
    assert idx.tolist() == pad([16, 11, 12, 15, 10], 8, NI) and group.tolist() == pad([1, 4, NG, NG, NG], 8, NG)
    assert members.tolist() == pad([1, 3, 1, 1, 1], 8, 0) and np.all(np.isinf(dist[5:]))
    assert facets.tolist() == [0, 1, 0, 0, 3] and totals == {"groups": 5, "window": 7, "beyond": 0, "nan": 0}
    assert expected_grouped(d, ids, groups, 8, n_groups=7)[4].tolist() == [0, 1, 0, 0, 3, 0, 0]


def test_the_four_identities():
    rng = np.random.default_rng(11)
    n = 300
    ids = np.arange(n, dtype=np.uint64) * 2 + 1
    d = rng.random(n).astype(np.float32)
    d[[5, 77]] = np.nan
    d[100:110] = d[20]
    bound = np.float32(0.6)
    # (a) every row NO_GROUP: the page call without a cursor, members = 1
    for k in (1, 10, 299, 400):
        idx, dist, group, members, facets, totals = expected_grouped(d, ids, np.full(n, NO_GROUP), k, bound)
        p_idx, p_dist, p_counts = expected_page(d, ids, k, None, bound)
        hit = p_idx != NO_ID
        assert np.array_equal(idx, p_idx) and np.array_equal(bits(dist), bits(p_dist)) and np.all(group == NO_GROUP)
        assert np.array_equal(members, hit.astype(np.uint64)) and facets.size == 0
        assert totals == {"groups": p_counts["window"], "window": p_counts["window"], "beyond": p_counts["beyond"], "nan": p_counts["nan"]}
    # (b) all rows in one group: one hit, the top-1, members = the window count
    idx, dist, group, members, facets, totals = expected_grouped(d, ids, np.zeros(n, np.uint32), 5, bound)
    p_idx, p_dist, p_counts = expected_page(d, ids, 1, None, bound)
    assert idx.tolist() == [int(p_idx[0])] + [NI] * 4 and bits(dist[0]) == bits(p_dist[0]) and members.tolist() == [p_counts["window"], 0, 0, 0, 0]
    assert totals["groups"] == 1 and facets.tolist() == [p_counts["window"]]
    # (c), (d) on a mixed layout
    groups = rng.integers(0, 12, n).astype(np.uint32)
    groups[rng.random(n) < 0.2] = NO_GROUP
    idx, dist, group, members, facets, totals = expected_grouped(d, ids, groups, 40, bound)
    in_window = dist_key(d) <= dist_key(bound)
    assert int(facets.sum()) + int((in_window & (groups == NO_GROUP)).sum()) == totals["window"]                  # (c)
    assert totals["groups"] == int((facets > 0).sum()) + int((in_window & (groups == NO_GROUP)).sum())
    for j in range(int((idx != NO_ID).sum())):                                                                     # (d)
        rows = np.flatnonzero(groups == group[j]) if group[j] != NO_GROUP else np.flatnonzero(ids == idx[j])
        f_idx, f_dist, _ = expected_page(d[rows], ids[rows], 1)
        assert f_idx[0] == idx[j] and bits(f_dist[0]) == bits(dist[j])
    assert np.all(np.diff(dist_key(dist[idx != NO_ID]).astype(np.int64)) >= 0)


# ---- the bindings -----------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert "#define MI_KNN_NO_GROUP 0xFFFFFFFFu" in header and "#define MI_KNN_GROUPS_MAX (1u << 24)" in header
    args = _lib.SYMBOLS["mi_knn_search_grouped"][1]
    assert len(args) == 13 and args[2:4] == [ctypes.c_uint32, ctypes.c_float] and args[11] == ctypes.c_uint64
    assert _lib.SYMBOLS["mi_knn_sharded_search_grouped"][1] == args and len(_lib.SYMBOLS["mi_index_search_grouped"][1]) == 16
    assert mi.mi_abi_version() == 4
    for cls, names in ((EmbeddingTable, ("set_groups", "groups", "knn_grouped")), (ShardedTable, ("set_groups", "groups", "knn_grouped")),
                       (ImageIndex, ("web_search_grouped", "group_name"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    assert "mi_knn_search_grouped(" in hpp and "mi_knn_sharded_search_grouped(" in hpp and "mi_index_search_grouped(" in hpp


def test_null_handles_and_bad_arguments_return_codes_without_a_device(mi):
    v = np.zeros(768, np.float32)
    idx, dist = np.full(4, 7, np.uint64), np.full(4, -7.0, np.float32)
    group, members, totals = np.full(4, 7, np.uint32), np.full(4, 7, np.uint64), np.full(4, 7, np.uint64)
    out = (idx.ctypes.data, dist.ctypes.data, group.ctypes.data, members.ctypes.data)
    rc = mi.mi_knn_search_grouped(None, v.ctypes.data, 4, np.inf, None, 0, *out, None, 0, totals.ctypes.data)
    assert rc == MI_ERR_INVALID
    assert mi.mi_knn_sharded_search_grouped(None, v.ctypes.data, 4, np.inf, None, 0, *out, None, 0, totals.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_index_search_grouped(None, v.ctypes.data, None, 0, None, 0, 4, np.inf, *out, None, None, 0, totals.ctypes.data) == MI_ERR_INVALID
    assert np.all(idx == 7) and np.all(dist == -7.0) and np.all(group == 7) and np.all(members == 7) and np.all(totals == 7)
    g = np.zeros(3, np.uint32)
    info = (ctypes.c_uint64 * 2)()
    n = ctypes.c_uint32()
    for fn in (mi.mi_knn_set_groups, mi.mi_knn_get_groups, mi.mi_knn_sharded_set_groups, mi.mi_knn_sharded_get_groups):
        assert fn(None, None, 3, g.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_knn_groups_info(None, info) == MI_ERR_INVALID and mi.mi_knn_sharded_groups_info(None, info) == MI_ERR_INVALID
    assert mi.mi_index_group_name(None, 0, 1, None, 0, None) == MI_ERR_INVALID
    assert mi.mi_index_group_count(None, ctypes.byref(n)) == MI_ERR_INVALID


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_grouped_host.cpp: a stand-alone program over csrc/grouped_host.h — the argument checks, the record layout,
    the sharded merge by group, the directory -> group rule of the index ("a/b/c.jpg" and "a/b/d.jpg" share a group, "a/bb/c.jpg"
    does not, files directly in the media directory form one) — built with the address and undefined-behaviour sanitizers; it
    needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_grouped_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_grouped_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
