"""mi_knn_density_levels, mi_knn_dbscan_levels and mi_dbscan_levels_tree without a GPU: the restatement of the contract
(include/mi355clip.h) — L calls of tests/test_density_host.py's expected_dbscan on the pair list thresholded per level, plus the
tree between the levels — on hand-written pair lists, the bindings, and the host-only rules (csrc/density_levels_host.h)
under the sanitizers.  The GPU tests (tests/test_density_levels_gpu.py) compare the device's result with it for equality."""
import ctypes
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, dbscan_levels_tree
from test_density_host import clique, expected_dbscan
from test_page_host import NO_ID

NEW = ["mi_knn_density_levels", "mi_knn_dbscan_levels", "mi_dbscan_levels_tree"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID = -1


# ---- the restatement ------------------------------------------------------------------------------------------------

def expected_tree(clusters, degs, min_pts):
    """clusters, degs: per level [n] -> [(level, child cluster id, parent cluster id)] ascending by (level, child): the parent of
    a level-l cluster is the level-(l + 1) cluster of its core rows, which must all agree"""
    edges = []
    for l in range(len(clusters) - 1):
        core = (clusters[l] != NO_ID) & (degs[l].astype(np.int64) + 1 >= min_pts)
        for c in np.unique(clusters[l][core]):
            parents = np.unique(clusters[l + 1][core & (clusters[l] == c)])
            assert parents.size == 1 and parents[0] != NO_ID, (l, c, parents)
            edges.append((l, int(c), int(parents[0])))
    return edges


def expected_dbscan_levels(n, a, b, d, max_dists, min_pts, live=None, ids=None):
    """the pairs (a[i] < b[i], d[i]) within the LARGEST distance -> (per level expected_dbscan's tuple on the pairs with
    d <= float32(max_dists[l]), the tree's edges)"""
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    d = np.asarray(d, np.float32).reshape(-1)
    levels = []
    for eps in max_dists:
        keep = d <= np.float32(eps)
        levels.append(expected_dbscan(n, a[keep], b[keep], d[keep], min_pts, live=live, ids=ids))
    return levels, expected_tree([lv[0] for lv in levels], [lv[3] for lv in levels], min_pts)


def run_levels(n, pairs, max_dists, min_pts, **kw):
    pairs = sorted((min(x, y), max(x, y), d) for x, y, d in pairs)
    a, b, d = (np.array([p[j] for p in pairs]) for j in range(3))
    return expected_dbscan_levels(n, a, b, d, max_dists, min_pts, **kw)


# ---- the restatement on hand-written pair lists -------------------------------------------------------------------------

def test_every_clusters_cores_lie_in_one_cluster_of_the_next_level():
    # bursts {0, 1, 2} and {3, 4, 5} at 0.01 inside a theme that closes at 0.1; a second theme {8, 9, 10} at 0.1; {12, 13, 14}
    # only at 0.2, where 6 also joins the first theme and 10 - 12 ties the second and the third together; 15 alone
    pairs = (clique([0, 1, 2], 0.01) + clique([3, 4, 5], 0.01) + [(2, 3, 0.09), (1, 4, 0.09)] + clique([8, 9, 10], 0.08)
             + clique([12, 13, 14], 0.18) + [(5, 6, 0.15), (4, 6, 0.16), (10, 12, 0.19)])
    levels, tree = run_levels(16, pairs, (0.02, 0.1, 0.2), 3)
    c0, c1, c2 = (lv[0] for lv in levels)
    assert c0.tolist() == [0, 0, 0, 3, 3, 3] + [int(NO_ID)] * 10
    assert c1.tolist() == [0] * 6 + [int(NO_ID)] * 2 + [8, 8, 8] + [int(NO_ID)] * 5
    assert c2.tolist() == [0] * 7 + [int(NO_ID)] + [8, 8, 8, int(NO_ID), 8, 8, 8, int(NO_ID)]
    assert [lv[4] for lv in levels] == [[2, 6, 0, 10], [2, 9, 0, 7], [2, 13, 0, 3]]
    assert tree == [(0, 0, 0), (0, 3, 0), (1, 0, 0), (1, 8, 8)]
    # nesting, spelt out: the core rows of every level-l cluster share one level-(l + 1) cluster
    for l in range(2):
        cl, deg = levels[l][0], levels[l][3]
        for c in np.unique(cl[cl != NO_ID]):
            cores = (cl == c) & (deg + 1 >= 3)
            assert cores.any() and np.unique(levels[l + 1][0][cores]).size == 1
    # the degrees are cumulative and every level is the single call on its own pairs
    assert np.all(levels[0][3] <= levels[1][3]) and np.all(levels[1][3] <= levels[2][3])
    one, _ = run_levels(16, [p for p in pairs if p[2] <= 0.1], (0.1,), 3)
    assert all(np.array_equal(x, y) for x, y in zip(one[0][:4], levels[1][:4])) and one[0][4] == levels[1][4]


def test_a_bridge_fuses_two_blobs_only_at_the_upper_level():
    # test_density_host's bridge: blobs 0..4 and 10..14 at 0.05, the bridge 4 - 5 - 6 - 7 - 10 at 0.15.  min_pts 3: the bridge's
    # rows have 2 neighbours and are cores once the upper level lets their pairs in
    pairs = clique([0, 1, 2, 3, 4]) + clique([10, 11, 12, 13, 14]) + [(4, 5, 0.15), (5, 6, 0.15), (6, 7, 0.15), (7, 10, 0.15)]
    levels, tree = run_levels(15, pairs, (0.1, 0.2), 3)
    lower, upper = levels
    assert lower[0].tolist() == [0] * 5 + [int(NO_ID)] * 5 + [10] * 5 and lower[4] == [2, 10, 0, 5]
    assert upper[0].tolist() == [0] * 8 + [int(NO_ID)] * 2 + [0] * 5 and upper[4] == [1, 13, 0, 2]
    assert tree == [(0, 0, 0), (0, 10, 0)]
    # with min_pts 4 the bridge's rows never are cores: two clusters at both levels, 5 and 7 border rows above
    levels, tree = run_levels(15, pairs, (0.1, 0.2), 4)
    assert levels[1][0].tolist() == [0] * 6 + [int(NO_ID), 10] + [int(NO_ID)] * 2 + [10] * 5
    assert tree == [(0, 0, 0), (0, 10, 10)]


def test_a_border_row_may_sit_in_a_cluster_that_is_not_its_lower_clusters_parent():
    # Lower level (0.1), min_pts 4: cluster 0 = the clique {0, 1, 2, 3}; row 4 is a border row of it through 3 at 0.09.
    # Row 5 has one neighbour at the lower level (4, at 0.05) and three more at the upper one (6, 7, 8 at 0.15), so it is a core
    # only at the upper level (0.2) — and nearer to 4 than 4's lower-level core 3.  At the upper level 4 is still no core
    # (2 neighbours), and its nearest core is now 5: it sits in cluster 5, while its lower-level cluster 0 has parent 0.
    pairs = clique([0, 1, 2, 3], 0.05) + [(3, 4, 0.09), (4, 5, 0.05), (5, 6, 0.15), (5, 7, 0.15), (5, 8, 0.15)]
    levels, tree = run_levels(9, pairs, (0.1, 0.2), 4)
    lower, upper = levels
    assert lower[3].tolist() == [3, 3, 3, 4, 2, 1, 0, 0, 0] and upper[3].tolist() == [3, 3, 3, 4, 2, 4, 1, 1, 1]
    assert lower[0].tolist() == [0, 0, 0, 0, 0] + [int(NO_ID)] * 4 and lower[1][4] == 3
    assert upper[0].tolist() == [0, 0, 0, 0, 5, 5, 5, 5, 5] and upper[1][4] == 5 and upper[2][4] == np.float32(0.05)
    assert lower[4] == [1, 4, 1, 4] and upper[4] == [2, 5, 4, 0]
    # the tree is still well defined: it goes through the core rows, which all stay in cluster 0
    assert tree == [(0, 0, 0)]
    assert lower[0][4] == 0 and upper[0][4] != dict((c, p) for _, c, p in tree)[int(lower[0][4])]


def test_deleted_rows_and_ids_go_through_every_level():
    live = np.ones(6, bool)
    live[2] = False
    ids = np.arange(6, dtype=np.uint64) + np.uint64(1 << 40)
    pairs = [(0, 1, 0.01), (3, 4, 0.01), (1, 3, 0.1), (4, 5, 0.15)]
    levels, tree = run_levels(6, pairs, (0.02, 0.12, 0.2), 2, live=live, ids=ids)
    base = 1 << 40
    assert levels[0][0].tolist() == [base, base, int(NO_ID), base + 3, base + 3, int(NO_ID)]
    assert levels[1][0].tolist() == [base, base, int(NO_ID), base, base, int(NO_ID)]
    assert levels[2][0].tolist() == [base, base, int(NO_ID), base, base, base]
    assert tree == [(0, base, base), (0, base + 3, base), (1, base, base)]


# ---- the bindings -----------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert "#define MI_KNN_LEVELS_MAX 8" in header
    assert mi.mi_abi_version() == 4
    assert len(_lib.SYMBOLS["mi_knn_density_levels"][1]) == 4 and len(_lib.SYMBOLS["mi_knn_dbscan_levels"][1]) == 9
    assert len(_lib.SYMBOLS["mi_dbscan_levels_tree"][1]) == 10
    for cls, names in ((EmbeddingTable, ("neighbor_counts_levels", "dbscan_levels")), (ImageIndex, ("theme_tree",))):
        for name in names:
            assert callable(getattr(cls, name)), name
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in ("mi_knn_density_levels(", "mi_knn_dbscan_levels(", "mi_dbscan_levels_tree("):
        assert name in hpp, name
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"density_levels.hip"' in build


def test_null_handles_and_bad_arguments_return_codes_without_a_device(mi):
    cluster, via = np.full(12, 7, np.uint64), np.full(12, 7, np.uint64)
    via_dist, counts, summary = np.full(12, -7.0, np.float32), np.full(12, 7, np.uint32), np.full(12, 7, np.uint64)
    out = (cluster.ctypes.data, via.ctypes.data, via_dist.ctypes.data, counts.ctypes.data, summary.ctypes.data)
    fake = ctypes.c_void_p(16)          # a handle that is never followed: every case below is refused in front of it

    def f32(*v):
        return np.array(v, np.float32)

    good = f32(0.02, 0.1, 0.2)
    bad = [f32(0.02, np.nan, 0.2), f32(-0.1, 0.1, 0.2), f32(0.02, 0.1, 0.1), f32(0.02, 0.2, 0.1), f32(np.nan, 0.1, 0.2)]
    nine = np.arange(9, dtype=np.float32) * np.float32(0.01)
    assert mi.mi_knn_density_levels(None, good.ctypes.data, 3, counts.ctypes.data) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert mi.mi_knn_density_levels(fake, None, 3, counts.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_knn_density_levels(fake, good.ctypes.data, 3, None) == MI_ERR_INVALID
    assert mi.mi_knn_density_levels(fake, good.ctypes.data, 0, counts.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_knn_density_levels(fake, nine.ctypes.data, 9, counts.ctypes.data) == MI_ERR_INVALID
    assert b"n_levels" in mi.mi_last_error()
    for d in bad:
        assert mi.mi_knn_density_levels(fake, d.ctypes.data, 3, counts.ctypes.data) == MI_ERR_INVALID, d
        assert mi.mi_knn_dbscan_levels(fake, d.ctypes.data, 3, 5, *out) == MI_ERR_INVALID, d
    assert b"max_dists" in mi.mi_last_error()
    assert mi.mi_knn_dbscan_levels(None, good.ctypes.data, 3, 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan_levels(fake, None, 3, 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan_levels(fake, good.ctypes.data, 0, 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan_levels(fake, nine.ctypes.data, 9, 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan_levels(fake, good.ctypes.data, 3, 0, *out) == MI_ERR_INVALID
    assert b"min_pts" in mi.mi_last_error()
    assert mi.mi_knn_dbscan_levels(fake, good.ctypes.data, 3, 5, None, *out[1:]) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan_levels(fake, good.ctypes.data, 3, 5, *out[:4], None) == MI_ERR_INVALID
    assert np.all(cluster == 7) and np.all(via == 7) and np.all(via_dist == -7.0) and np.all(counts == 7) and np.all(summary == 7)


def test_the_tree_call_needs_no_device(mi):
    no = int(NO_ID)
    cluster = np.array([[0, 0, 2, 2, 4, no], [0, 0, 0, 0, 4, 4]], np.uint64)
    counts = np.array([[1, 1, 1, 1, 0, 0], [3, 3, 3, 3, 1, 1]], np.uint32)
    level, child, parent = dbscan_levels_tree(cluster, counts, 1)
    assert level.tolist() == [0, 0, 0] and child.tolist() == [0, 2, 4] and parent.tolist() == [0, 0, 4]
    assert list(zip(level.tolist(), child.tolist(), parent.tolist())) == expected_tree(list(cluster), list(counts), 1)
    level, child, parent = dbscan_levels_tree(cluster, counts, 2)                 # row 4 is no core any more: cluster 4 has no edge
    assert child.tolist() == [0, 2] and parent.tolist() == [0, 0]
    # the cap convention: the full count, the first cap edges, the rest of the arrays untouched
    lv, ch, pa = np.full(3, 9, np.uint32), np.full(3, 9, np.uint64), np.full(3, 9, np.uint64)
    n = ctypes.c_uint64(77)
    args = (cluster.ctypes.data, counts.ctypes.data, 6, 2, 1)
    assert mi.mi_dbscan_levels_tree(*args, lv.ctypes.data, ch.ctypes.data, pa.ctypes.data, 2, ctypes.byref(n)) == 0
    assert n.value == 3 and lv.tolist() == [0, 0, 9] and ch.tolist() == [0, 2, 9] and pa.tolist() == [0, 0, 9]
    assert mi.mi_dbscan_levels_tree(*args, None, None, None, 0, ctypes.byref(n)) == 0 and n.value == 3
    # the cores of cluster 0 disagree: not a result of mi_knn_dbscan_levels; an error writes nothing
    split = cluster.copy()
    split[1, 1] = 4
    n = ctypes.c_uint64(77)
    lv[:] = 9
    assert mi.mi_dbscan_levels_tree(split.ctypes.data, counts.ctypes.data, 6, 2, 1, lv.ctypes.data, ch.ctypes.data, pa.ctypes.data, 3,
                                    ctypes.byref(n)) == MI_ERR_INVALID
    assert b"two clusters" in mi.mi_last_error() and n.value == 77 and lv.tolist() == [9, 9, 9]
    for bad in ((None, counts.ctypes.data, 6, 2, 1), (cluster.ctypes.data, None, 6, 2, 1), (cluster.ctypes.data, counts.ctypes.data, 6, 0, 1),
                (cluster.ctypes.data, counts.ctypes.data, 6, 9, 1), (cluster.ctypes.data, counts.ctypes.data, 6, 2, 0)):
        assert mi.mi_dbscan_levels_tree(*bad, lv.ctypes.data, ch.ctypes.data, pa.ctypes.data, 3, ctypes.byref(n)) == MI_ERR_INVALID, bad
    assert mi.mi_dbscan_levels_tree(*args, None, ch.ctypes.data, pa.ctypes.data, 3, ctypes.byref(n)) == MI_ERR_INVALID
    assert mi.mi_dbscan_levels_tree(*args, lv.ctypes.data, ch.ctypes.data, pa.ctypes.data, 3, None) == MI_ERR_INVALID
    assert n.value == 77
    # no rows, and one level: no edges
    level, child, parent = dbscan_levels_tree(np.zeros((3, 0), np.uint64), np.zeros((3, 0), np.uint32), 5)
    assert level.size == 0 and child.size == 0 and parent.size == 0
    assert dbscan_levels_tree(cluster[:1], counts[:1], 1)[0].size == 0


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_density_levels_host.cpp: a stand-alone program over csrc/density_levels_host.h — the argument rules, the
    level a distance falls into, the tree builder against a brute-force restatement, a disagreeing input and the cap — built
    with the address and undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_density_levels_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_density_levels_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
