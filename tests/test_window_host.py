"""The windowed pair calls without a GPU (mi_knn_near_pairs_window, mi_knn_density_window, mi_knn_dbscan_window,
mi_knn_window_stats, mi_index_bursts, mi_index_events): the bindings, a Python-int restatement of the stamp test on the
edge values, the windowed DBSCAN as expected_dbscan over a filtered pair list on two hand-made cases, and the host-only
rules (csrc/window_host.h) under the sanitizers.

W_win is the pairs of mi_knn_near_pairs whose two stamps pass the stamp test; the GPU tests (tests/test_window_gpu.py) feed
the same restatement with the CPU oracle's pairs."""
import ctypes
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable
from test_density_host import clique, expected_dbscan
from test_page_host import NO_ID

NEW = ["mi_knn_near_pairs_window", "mi_knn_density_window", "mi_knn_dbscan_window", "mi_knn_window_stats", "mi_index_bursts",
       "mi_index_events"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID = -1
I64_MIN, I64_MAX, U64_MAX = -2 ** 63, 2 ** 63 - 1, 2 ** 64 - 1


# ---- the restatement ------------------------------------------------------------------------------------------------

def stamp_within(sa, sb, window):
    """the stamp test on Python integers: exact whatever the values"""
    return abs(int(sa) - int(sb)) <= int(window)


def stamp_within_u64(sa, sb, window):
    """... and as the header words it: hi = max, lo = min (signed compare), (uint64)hi - (uint64)lo in wrapping arithmetic"""
    hi, lo = max(int(sa), int(sb)), min(int(sa), int(sb))
    return ((hi % 2 ** 64) - (lo % 2 ** 64)) % 2 ** 64 <= int(window)


def window_pairs(a, b, d, stamps, window):
    """W -> W_win: the pairs whose two rows pass the stamp test; ids, order and distance bits stay.  stamps None: all 0"""
    a, b, d = np.asarray(a), np.asarray(b), np.asarray(d)
    if stamps is None:
        return a, b, d
    keep = np.array([stamp_within(stamps[x], stamps[y], window) for x, y in zip(a, b)], bool).reshape(-1)
    return a[keep], b[keep], d[keep]


def expected_dbscan_window(n, a, b, d, stamps, window, min_pts, **kw):
    return expected_dbscan(n, *window_pairs(a, b, d, stamps, window), min_pts, **kw)


def run(n, pairs, stamps, window, min_pts, **kw):
    pairs = sorted((min(x, y), max(x, y), d) for x, y, d in pairs)
    a, b, d = (np.array([p[j] for p in pairs]) for j in range(3))
    return expected_dbscan_window(n, a, b, d, stamps, window, min_pts, **kw)


# ---- the stamp test on its edge values -----------------------------------------------------------------------------------

def test_the_stamp_test_on_the_edge_values():
    cases = [(7, 7, 0, True), (7, 8, 0, False),                                  # window 0: equal stamps only
             (1000, 1060, 60, True), (1000, 1061, 60, False), (1061, 1000, 60, False),   # exactly window, and window + 1
             (I64_MIN, I64_MAX, U64_MAX - 1, False), (I64_MIN, I64_MAX, U64_MAX, True), (I64_MAX, I64_MIN, U64_MAX, True),
             (I64_MIN, 0, 2 ** 63 - 1, False), (I64_MIN, 0, 2 ** 63, True), (0, I64_MIN, 2 ** 63, True),
             (-1, 1, 1, False), (-1, 1, 2, True), (1, -1, 2, True),
             (I64_MAX, 0, 2 ** 63 - 1, True), (I64_MAX, 0, 2 ** 63 - 2, False)]
    for sa, sb, window, want in cases:
        assert stamp_within(sa, sb, window) == want, (sa, sb, window)
        assert stamp_within_u64(sa, sb, window) == want, (sa, sb, window)
    # what a signed 64-bit subtraction would make of the extremes: INT64_MIN - INT64_MAX wraps to 1
    wrapped = ((I64_MIN - I64_MAX) + 2 ** 63) % 2 ** 64 - 2 ** 63
    assert wrapped == 1 and not stamp_within(I64_MIN, I64_MAX, 1)
    rng = np.random.default_rng(5)
    for sa, sb in rng.integers(I64_MIN, I64_MAX, (200, 2), dtype=np.int64, endpoint=True):
        for window in (0, int(rng.integers(0, U64_MAX, dtype=np.uint64, endpoint=True)), U64_MAX):
            assert stamp_within_u64(sa, sb, window) == stamp_within(sa, sb, window)


# ---- the windowed DBSCAN on hand-written pair lists --------------------------------------------------------------------------

def test_one_visual_clique_is_split_into_two_clusters_by_time():
    # ten look-alikes: rows 0..4 taken in 2019, rows 5..9 in 2023
    pairs = clique(list(range(10)))
    stamps = np.array([1_560_000_000 + i for i in range(5)] + [1_690_000_000 + i for i in range(5)], np.int64)
    cluster, via, via_dist, deg, summary = run(10, pairs, None, 0, 4)
    assert cluster.tolist() == [0] * 10 and deg.tolist() == [9] * 10 and summary == [1, 10, 0, 0]
    cluster, via, via_dist, deg, summary = run(10, pairs, stamps, 86_400, 4)
    assert cluster.tolist() == [0] * 5 + [5] * 5 and deg.tolist() == [4] * 10 and summary == [2, 10, 0, 0]
    assert run(10, pairs, stamps, U64_MAX, 4)[0].tolist() == [0] * 10
    # at window 0 nobody has a neighbour: noise at min_pts 2, ten clusters of one at min_pts 1
    assert run(10, pairs, stamps, 0, 2)[4] == [0, 0, 0, 10] and run(10, pairs, stamps, 0, 1)[4] == [10, 10, 0, 0]


def test_a_border_row_whose_nearest_core_is_outside_the_window_joins_through_a_farther_one():
    # cores 0 (with 1, 2, 3) and 6 (with 7, 8, 9); 4 is nearer to 0 (0.05) than to 6 (0.1), but 0 was taken long before
    pairs = clique([0, 1, 2, 3]) + clique([6, 7, 8, 9]) + [(0, 4, 0.05), (4, 6, 0.1)]
    stamps = np.array([100, 101, 102, 103, 5000, 0, 5001, 5002, 5003, 5004], np.int64)
    cluster, via, via_dist, deg, summary = run(10, pairs, None, 0, 4)
    assert via[4] == 0 and cluster[4] == 0 and via_dist[4] == np.float32(0.05) and deg[4] == 2
    cluster, via, via_dist, deg, summary = run(10, pairs, stamps, 10, 4)
    assert via[4] == 6 and cluster[4] == 6 and via_dist[4] == np.float32(0.1) and deg[4] == 1
    assert deg[0] == 3 and summary == [2, 8, 1, 1] and cluster[5] == NO_ID


# ---- the bindings -----------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
        assert name + "(" in hpp, name
    assert mi.mi_abi_version() == 4
    # the siblings' argument lists with `window` behind max_dist
    for new, old in (("mi_knn_near_pairs_window", "mi_knn_near_pairs"), ("mi_knn_density_window", "mi_knn_density"),
                     ("mi_knn_dbscan_window", "mi_knn_dbscan"), ("mi_index_bursts", "mi_index_duplicates"),
                     ("mi_index_events", "mi_index_themes")):
        args, sibling = _lib.SYMBOLS[new][1], _lib.SYMBOLS[old][1]
        assert args == sibling[:2] + [ctypes.c_uint64] + sibling[2:], new
    for cls, names in ((EmbeddingTable, ("near_pairs_window", "neighbor_counts_window", "dbscan_window", "window_stats")),
                       (ImageIndex, ("bursts", "events"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    assert not any(hasattr(ShardedTable, name) for name in ("near_pairs_window", "dbscan_window", "neighbor_counts_window"))
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"window.hip"' in build


def test_null_handles_and_bad_arguments_return_codes_without_a_device(mi):
    cluster, via = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64)
    via_dist, counts, summary = np.full(4, -7.0, np.float32), np.full(4, 7, np.uint32), np.full(4, 7, np.uint64)
    n = [ctypes.c_uint64(7) for _ in range(3)]
    refs = [ctypes.byref(v) for v in n]
    out = (cluster.ctypes.data, via.ctypes.data, via_dist.ctypes.data, counts.ctypes.data, summary.ctypes.data)
    fake = ctypes.c_void_p(16)          # a handle that is never followed: every case below is refused in front of it
    assert mi.mi_knn_density_window(None, 0.1, 5, counts.ctypes.data) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert mi.mi_knn_density_window(fake, 0.1, 5, None) == MI_ERR_INVALID
    assert mi.mi_knn_density_window(fake, -0.5, 5, counts.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_knn_density_window(fake, float("nan"), 5, counts.ctypes.data) == MI_ERR_INVALID
    assert b"max_dist" in mi.mi_last_error()
    assert mi.mi_knn_dbscan_window(None, 0.1, 5, 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan_window(fake, 0.1, 5, 0, *out) == MI_ERR_INVALID
    assert b"min_pts" in mi.mi_last_error()
    assert mi.mi_knn_dbscan_window(fake, -1.0, 5, 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan_window(fake, float("nan"), 5, 5, *out) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan_window(fake, 0.1, 5, 5, None, *out[1:]) == MI_ERR_INVALID
    assert mi.mi_knn_dbscan_window(fake, 0.1, 5, 5, *out[:4], None) == MI_ERR_INVALID
    a, b, d = cluster.ctypes.data, via.ctypes.data, via_dist.ctypes.data
    assert mi.mi_knn_near_pairs_window(None, 0.1, 5, 0, a, b, d, 4, refs[0]) == MI_ERR_INVALID
    assert mi.mi_knn_near_pairs_window(fake, float("nan"), 5, 0, a, b, d, 4, refs[1]) == MI_ERR_INVALID
    assert mi.mi_knn_near_pairs_window(fake, -0.1, 5, 0, a, b, d, 4, refs[1]) == MI_ERR_INVALID
    assert [v.value for v in n] == [0, 0, 7]                                   # the cap protocol's count, as mi_knn_near_pairs
    assert mi.mi_knn_near_pairs_window(fake, 0.1, 5, 0, a, b, d, 4, None) == MI_ERR_INVALID
    assert mi.mi_knn_window_stats(None, (ctypes.c_uint64 * 8)()) == MI_ERR_INVALID
    assert mi.mi_knn_window_stats(fake, None) == MI_ERR_INVALID
    n = [ctypes.c_uint64(7) for _ in range(3)]
    refs = [ctypes.byref(v) for v in n]
    assert mi.mi_index_events(None, 0.1, 5, 5, cluster.ctypes.data, 4, via.ctypes.data, 4, *refs) == MI_ERR_INVALID
    assert mi.mi_index_events(fake, 0.1, 5, 0, cluster.ctypes.data, 4, via.ctypes.data, 4, *refs) == MI_ERR_INVALID
    assert mi.mi_index_events(fake, float("nan"), 5, 5, cluster.ctypes.data, 4, via.ctypes.data, 4, *refs) == MI_ERR_INVALID
    assert mi.mi_index_events(fake, 0.1, 5, 5, None, 4, via.ctypes.data, 4, *refs) == MI_ERR_INVALID
    assert mi.mi_index_events(fake, 0.1, 5, 5, cluster.ctypes.data, 4, via.ctypes.data, 4, refs[0], refs[1], None) == MI_ERR_INVALID
    assert [v.value for v in n] == [7, 7, 7]
    assert mi.mi_index_bursts(None, 0.1, 5, 0, 100, cluster.ctypes.data, 4, via.ctypes.data, 4, refs[0], refs[1]) == MI_ERR_INVALID
    assert np.all(cluster == 7) and np.all(via == 7) and np.all(via_dist == -7.0) and np.all(counts == 7) and np.all(summary == 7)


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_window_host.cpp: a stand-alone program over csrc/window_host.h — the exact stamp difference and the gap
    on the extremes of int64, empty ranges, the columns a banded, a full and an all-skipped strip launch, and computed +
    skipped = the triangle against a brute-force walk in 128-bit arithmetic — built with the address and
    undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_window_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_window_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
