"""mi_knn_density, mi_knn_dbscan and mi_index_themes without a GPU: the numpy restatement of the contract
(include/mi355clip.h) on hand-written pair lists, the bindings, and the host-only rules (csrc/density_host.h) under the
sanitizers.

The restatement works on a pair list alone — the pairs (a < b, d) mi_knn_near_pairs reports; the GPU tests
(tests/test_density_gpu.py) feed it the CPU oracle's pairs and the device's own and compare ids, distance bits, counts and
summary with it for equality."""
import ctypes
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, dense_labels
from test_page_host import INF, NO_ID, bits, dist_key

NEW = ["mi_knn_density", "mi_knn_dbscan", "mi_knn_dbscan_stats", "mi_index_themes"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID = -1


# ---- the restatement ------------------------------------------------------------------------------------------------

def expected_dbscan(n, a, b, d, min_pts, live=None, ids=None):
    """n rows; the pairs (a[i] < b[i], d[i]) over local rows, live rows only; live [n] bool (None: all); ids [n] (None: the
    rows).  -> cluster [n] u64, via [n] u64, via_dist [n] f32, counts [n] u32, summary [clusters, core, border, noise]"""
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    d = np.asarray(d, np.float32).reshape(-1)
    live = np.ones(n, bool) if live is None else np.asarray(live, bool)
    ids = np.arange(n, dtype=np.uint64) if ids is None else np.asarray(ids, np.uint64)
    deg = (np.bincount(a, minlength=n) + np.bincount(b, minlength=n)).astype(np.uint32)
    core = live & (deg.astype(np.int64) + 1 >= min_pts)
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in zip(a, b):
        if core[x] and core[y]:
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)   # the smallest row is the root
    key = dist_key(d).astype(np.uint64) << np.uint64(32)
    best = np.full(n, NO_ID, np.uint64)              # min over the core neighbours of (dist key, core row)
    for x, y, k in zip(a, b, key):
        for border, c in ((x, y), (y, x)):
            if core[c] and not core[border]:
                best[border] = min(best[border], k | np.uint64(c))
    cluster, via = np.full(n, NO_ID, np.uint64), np.full(n, NO_ID, np.uint64)
    via_dist = np.full(n, np.inf, np.float32)
    summary = [0, 0, 0, 0]
    dist_of = {}
    for x, y, k, dd in zip(a, b, key, d):
        dist_of[(int(x), int(y))] = dd
    for r in range(n):
        if not live[r]:
            continue
        if core[r]:
            root = find(r)
            cluster[r], via[r], via_dist[r] = ids[root], ids[r], np.float32(0.0)
            summary[1] += 1
            summary[0] += int(root == r)
        elif best[r] != NO_ID:
            c = int(best[r] & np.uint64(0xFFFFFFFF))
            cluster[r], via[r] = ids[find(c)], ids[c]
            via_dist[r] = dist_of[(min(r, c), max(r, c))]
            summary[2] += 1
        else:
            summary[3] += 1
    return cluster, via, via_dist, deg, summary


def check_same(got, want, what=""):
    """got: EmbeddingTable.dbscan's dict; want: expected_dbscan's tuple — equality, distances by their bits"""
    cluster, via, via_dist, deg, summary = want
    assert np.array_equal(got["counts"], deg), what
    assert np.array_equal(got["cluster"], cluster), what
    assert np.array_equal(got["via"], via), what
    assert np.array_equal(bits(got["via_dist"]), bits(via_dist)), what
    assert [got["summary"][k] for k in ("clusters", "core", "border", "noise")] == summary, what
    assert np.array_equal(got["labels"], dense_labels(cluster)), what


# ---- the restatement on hand-written pair lists -------------------------------------------------------------------------

def clique(rows, d=0.05):
    return [(x, y, d) for i, x in enumerate(rows) for y in rows[i + 1:]]


def run(n, pairs, min_pts, **kw):
    pairs = sorted((min(x, y), max(x, y), d) for x, y, d in pairs)
    a, b, d = (np.array([p[j] for p in pairs]) for j in range(3)) if pairs else (np.zeros(0), np.zeros(0), np.zeros(0))
    return expected_dbscan(n, a, b, d, min_pts, **kw)


def test_a_bridge_of_non_core_rows_keeps_two_blobs_apart_until_min_pts_lets_it_through():
    # blobs 0..4 and 10..14 (cliques: 4 neighbours each), a bridge 4 - 5 - 6 - 7 - 10 of rows with 2 neighbours; 8, 9 alone
    pairs = clique([0, 1, 2, 3, 4]) + clique([10, 11, 12, 13, 14]) + [(4, 5, 0.1), (5, 6, 0.1), (6, 7, 0.1), (7, 10, 0.1)]
    cluster, via, via_dist, deg, summary = run(15, pairs, 4)
    assert deg.tolist() == [4, 4, 4, 4, 5, 2, 2, 2, 0, 0, 5, 4, 4, 4, 4]
    assert cluster.tolist() == [0] * 5 + [0, int(NO_ID), 10, int(NO_ID), int(NO_ID)] + [10] * 5
    assert via[5] == 4 and via[7] == 10 and via[6] == NO_ID and via[3] == 3
    assert summary == [2, 10, 2, 3]                         # 6 is noise: its neighbours are no cores
    assert dense_labels(cluster).tolist() == [0] * 6 + [-1, 1, -1, -1] + [1] * 5
    cluster, via, via_dist, deg, summary = run(15, pairs, 2)
    assert cluster.tolist() == [0] * 8 + [int(NO_ID)] * 2 + [0] * 5 and summary == [1, 13, 0, 2]
    assert via_dist[8] == INF and bits(via_dist[:8]).tolist() == [0] * 8


def test_a_border_row_between_two_cores_at_equal_distance_bits_takes_the_smaller_row():
    # cores 0 (with 1, 2, 3) and 6 (with 7, 8, 9); 4 is a border of both at the same bits, 5 nearer to 6; 10 alone
    pairs = clique([0, 1, 2, 3]) + clique([6, 7, 8, 9]) + [(0, 4, 0.125), (4, 6, 0.125), (0, 5, 0.125), (5, 6, 0.1)]
    cluster, via, via_dist, deg, summary = run(11, pairs, 4)
    assert deg.tolist() == [5, 3, 3, 3, 2, 2, 5, 3, 3, 3, 0]
    assert via[4] == 0 and cluster[4] == 0 and via_dist[4] == np.float32(0.125)
    assert via[5] == 6 and cluster[5] == 6 and via_dist[5] == np.float32(0.1)
    assert summary == [2, 8, 2, 1] and cluster[10] == NO_ID
    # ids that are not the rows
    ids = np.arange(11, dtype=np.uint64) + np.uint64(1 << 40)
    c2 = run(11, pairs, 4, ids=ids)[0]
    assert c2[4] == (1 << 40) and c2[7] == (1 << 40) + 6
    # a cluster is named by its smallest CORE row: a border row below it does not rename it
    pairs2 = clique([1, 2, 3]) + [(0, 2, 0.1)]
    cluster, via, _, deg, summary = run(4, pairs2, 3)
    assert deg.tolist() == [1, 2, 3, 2] and cluster.tolist() == [1, 1, 1, 1] and via[0] == 2 and summary == [1, 3, 1, 0]


def test_minus_zero_beats_plus_zero():
    pairs = clique([0, 1, 2, 3]) + clique([6, 7, 8, 9]) + [(0, 4, 0.0), (4, 6, -0.0)]
    cluster, via, via_dist, _, _ = run(10, pairs, 4)
    assert via[4] == 6 and cluster[4] == 6 and bits(via_dist[4]) == 0x80000000
    pairs = clique([0, 1, 2, 3]) + clique([6, 7, 8, 9]) + [(0, 4, -0.0), (4, 6, 0.0)]
    cluster, via, via_dist, _, _ = run(10, pairs, 4)
    assert via[4] == 0 and bits(via_dist[4]) == 0x80000000


def test_min_pts_one_makes_every_live_row_a_core_singletons_included():
    live = np.array([True, True, False, True, True])
    cluster, via, via_dist, deg, summary = run(5, [(0, 3, 0.1)], 1, live=live)
    assert cluster.tolist() == [0, 1, int(NO_ID), 0, 4] and via.tolist() == [0, 1, int(NO_ID), 3, 4]
    assert summary == [3, 4, 0, 0] and via_dist[2] == INF and deg.tolist() == [1, 0, 0, 1, 0]
    assert run(1, [], 1)[4] == [1, 1, 0, 0] and run(1, [], 2)[4] == [0, 0, 0, 1] and run(0, [], 1)[4] == [0, 0, 0, 0]


# ---- the bindings -----------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert mi.mi_abi_version() == 4
    assert len(_lib.SYMBOLS["mi_knn_dbscan"][1]) == 8 and len(_lib.SYMBOLS["mi_index_themes"][1]) == 10
    for cls, names in ((EmbeddingTable, ("neighbor_counts", "dbscan", "dbscan_stats")), (ImageIndex, ("themes",))):
        for name in names:
            assert callable(getattr(cls, name)), name
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in ("mi_knn_density(", "mi_knn_dbscan(", "mi_knn_dbscan_stats(", "mi_index_themes("):
        assert name in hpp, name
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"density.hip"' in build


def test_null_handles_and_bad_arguments_return_codes_without_a_device(mi):
    cluster, via = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64)
    via_dist, counts, summary = np.full(4, -7.0, np.float32), np.full(4, 7, np.uint32), np.full(4, 7, np.uint64)
    n = [ctypes.c_uint64(7) for _ in range(3)]
    refs = [ctypes.byref(v) for v in n]
    out = (cluster.ctypes.data, via.ctypes.data, via_dist.ctypes.data, counts.ctypes.data, summary.ctypes.data)
    fake = ctypes.c_void_p(16)          # a handle that is never followed: every case below is refused in front of it
    assert mi.mi_knn_density(None, 0.1, counts.ctypes.data) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert mi.mi_knn_density(fake, 0.1, None) == MI_ERR_INVALID
    assert mi.mi_knn_density(fake, -0.5, counts.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_knn_density(fake, float("nan"), counts.ctypes.data) == MI_ERR_INVALID
    assert b"max_dist" in mi.mi_last_error()
    assert mi.mi_knn_dbscan(None, 0.1, 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan(fake, 0.1, 0, *out) == MI_ERR_INVALID
    assert b"min_pts" in mi.mi_last_error()
    assert mi.mi_knn_dbscan(fake, -1.0, 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan(fake, float("nan"), 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan(fake, 0.1, 5, None, *out[1:]) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan(fake, 0.1, 5, *out[:4], None) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan_stats(None, (ctypes.c_uint64 * 8)()) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan_stats(fake, None) == MI_ERR_INVALID
    assert mi.mi_index_themes(None, 0.1, 5, cluster.ctypes.data, 4, via.ctypes.data, 4, *refs) == MI_ERR_INVALID
    assert mi.mi_index_themes(fake, 0.1, 0, cluster.ctypes.data, 4, via.ctypes.data, 4, *refs) == MI_ERR_INVALID
    assert mi.mi_index_themes(fake, float("nan"), 5, cluster.ctypes.data, 4, via.ctypes.data, 4, *refs) == MI_ERR_INVALID
    assert mi.mi_index_themes(fake, -0.1, 5, cluster.ctypes.data, 4, via.ctypes.data, 4, *refs) == MI_ERR_INVALID
    assert mi.mi_index_themes(fake, 0.1, 5, None, 4, via.ctypes.data, 4, *refs) == MI_ERR_INVALID
    assert mi.mi_index_themes(fake, 0.1, 5, cluster.ctypes.data, 4, via.ctypes.data, 4, refs[0], refs[1], None) == MI_ERR_INVALID
    assert np.all(cluster == 7) and np.all(via == 7) and np.all(via_dist == -7.0) and np.all(counts == 7) and np.all(summary == 7)
    assert [v.value for v in n] == [7, 7, 7]


def test_dense_labels_follow_the_cluster_ids():
    c = np.array([9, NO_ID, 3, 9, 1 << 40, 3, NO_ID], np.uint64)
    assert dense_labels(c).tolist() == [1, -1, 0, 1, 2, 0, -1]
    assert dense_labels(np.zeros(0, np.uint64)).size == 0
    assert dense_labels(c).astype(np.uint32)[1] == 0xFFFFFFFF      # NO_GROUP: what set_groups takes for "a row of its own"


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_density_host.cpp: a stand-alone program over csrc/density_host.h — the argument rules, the tile counts
    against a brute-force walk, the dense renumbering and the cluster lists — built with the address and undefined-behaviour
    sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_density_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_density_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
