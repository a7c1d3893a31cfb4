"""mi_knn_summarize and mi_index_folder_overview without a GPU: the numpy restatement of the contract
(include/mi355clip.h) on hand-written arrays, the bindings and error codes, and the host-only rules
(csrc/summary_host.h) under the sanitizers.

The restatement covers everything but the centroid and `dist`: the GPU tests (tests/test_summary_gpu.py) feed it the
device's own distances and compare counts, ids, distance bits, sums and totals with it for equality."""
import ctypes
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, dist_keys, typical_order
from test_page_host import INF, NO_ID, bits, dist_key

NEW = ["mi_knn_summarize", "mi_knn_summarize_stats", "mi_index_folder_overview"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
NO_LABEL = 0xFFFFFFFF
NAN = np.float32(np.nan)


# ---- the restatement ------------------------------------------------------------------------------------------------

def weight(d):
    """w(d) = floor(min(max(d, 0), 2) * 2^30): a power-of-two scaling of an fp32 value is exact, so float64 restates it"""
    return np.floor(np.clip(np.asarray(d, np.float32).astype(np.float64), 0.0, 2.0) * 2.0 ** 30).astype(np.uint64)


def expected_summary(labels, live, usable, dist, ids, C):
    """labels [n] (>= C: belongs to nothing), live [n] bool, usable [n] bool, dist [n] f32 (read for the members only),
    ids [n] u64 ascending with the row -> dict(count, cover, cover_dist, odd, odd_dist, measured, spread [C], totals [4])"""
    labels = np.asarray(labels).astype(np.uint32).reshape(-1)
    live, usable = np.asarray(live, bool), np.asarray(usable, bool)
    dist, ids = np.asarray(dist, np.float32), np.asarray(ids, np.uint64)
    inside = live & (labels < C)
    member = inside & usable
    out = {"count": np.zeros(C, np.uint64), "cover": np.full(C, NO_ID, np.uint64), "cover_dist": np.full(C, np.inf, np.float32),
           "odd": np.full(C, NO_ID, np.uint64), "odd_dist": np.full(C, np.inf, np.float32), "measured": np.zeros(C, np.uint64),
           "spread": np.zeros(C, np.uint64)}
    key = dist_key(dist).astype(np.uint64)
    rows_all = np.flatnonzero(member)
    rows_all = rows_all[np.argsort(labels[rows_all], kind="stable")]          # by group, ascending by row inside
    cuts = np.searchsorted(labels[rows_all], np.arange(C + 1))
    for c in np.flatnonzero(np.diff(cuts)):
        rows = rows_all[cuts[c]:cuts[c + 1]]
        out["count"][c] = rows.size
        best = min(rows, key=lambda r: (int(key[r]), int(ids[r])))
        out["cover"][c], out["cover_dist"][c] = ids[best], dist[best]
        num = rows[~np.isnan(dist[rows])]
        out["measured"][c] = num.size
        if num.size:
            worst = min(num, key=lambda r: (-int(key[r]), int(ids[r])))
            out["odd"][c], out["odd_dist"][c] = ids[worst], dist[worst]
            out["spread"][c] = int(weight(dist[num]).sum())
    out["totals"] = [int(member.sum()), int((live & (labels >= C)).sum()), int((inside & ~usable).sum()), int((out["count"] > 0).sum())]
    return out


def check_same(got, want, what=""):
    """got: EmbeddingTable.summarize's dict; want: expected_summary's — equality, distances by their bits"""
    for k in ("count", "cover", "odd", "measured", "spread"):
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8])
    for k in ("cover_dist", "odd_dist"):
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)
    assert [got["totals"][k] for k in ("members", "outside", "unusable", "groups")] == want["totals"], (what, got["totals"], want["totals"])


# ---- the restatement on hand-written arrays ---------------------------------------------------------------------------

def test_empty_group_group_of_one_and_labels_beyond_c():
    #            group 0 (one member)  group 1 empty   group 2            beyond C        deleted
    labels = np.array([0,               2, 2, 2,        5, NO_LABEL, 3,    2], np.uint32)
    dist = np.array([0.25,              0.5, 0.125, 0.75, 9, 9, 9,         0.01], np.float32)
    live = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    e = expected_summary(labels, live, np.ones(8, bool), dist, np.arange(8) + 100, 3)
    assert e["count"].tolist() == [1, 0, 3] and e["measured"].tolist() == [1, 0, 3]
    assert e["cover"].tolist() == [100, int(NO_ID), 102] and e["odd"].tolist() == [100, int(NO_ID), 103]
    assert e["cover_dist"].tolist() == [0.25, INF, 0.125] and e["odd_dist"].tolist() == [0.25, INF, 0.75]
    assert e["spread"].tolist() == [1 << 28, 0, (1 << 29) + (1 << 27) + (3 << 28)]
    assert e["totals"] == [4, 3, 0, 2]


def test_equal_distance_bits_the_lowest_id_is_cover_and_odd_one_out():
    dist = np.full(5, 0.375, np.float32)
    e = expected_summary(np.zeros(5, np.uint32), np.ones(5, bool), np.ones(5, bool), dist, np.array([7, 8, 9, 10, 11]), 1)
    assert e["cover"][0] == 7 and e["odd"][0] == 7 and e["count"][0] == 5 and e["spread"][0] == 5 * (3 << 27)
    # one member nearer, one farther, copies in between: the lowest id among the equal keys wins on both ends
    dist = np.array([0.5, 0.25, 0.25, 0.75, 0.75], np.float32)
    e = expected_summary(np.zeros(5, np.uint32), np.ones(5, bool), np.ones(5, bool), dist, np.arange(5), 1)
    assert e["cover"][0] == 1 and e["odd"][0] == 3


def test_minus_zero_comes_before_plus_zero():
    dist = np.array([0.0, -0.0, 0.0], np.float32)
    e = expected_summary(np.zeros(3, np.uint32), np.ones(3, bool), np.ones(3, bool), dist, np.arange(3), 1)
    assert e["cover"][0] == 1 and bits(e["cover_dist"])[0] == 0x80000000
    assert e["odd"][0] == 0 and bits(e["odd_dist"])[0] == 0 and e["spread"][0] == 0


def test_a_group_whose_distances_are_all_nan_has_a_cover_and_no_odd_one_out():
    dist = np.array([NAN, NAN, 0.5, NAN], np.float32)
    labels = np.array([0, 0, 1, 1], np.uint32)
    e = expected_summary(labels, np.ones(4, bool), np.ones(4, bool), dist, np.arange(4) + 10, 2)
    assert e["count"].tolist() == [2, 2] and e["measured"].tolist() == [0, 1]
    assert e["cover"][0] == 10 and np.isnan(e["cover_dist"][0]) and e["odd"][0] == NO_ID and e["odd_dist"][0] == INF
    assert e["cover"][1] == 12 and e["odd"][1] == 12 and e["spread"].tolist() == [0, 1 << 29]
    # an unusable row is no member: it counts in totals[2] alone
    e = expected_summary(labels, np.ones(4, bool), np.array([1, 0, 1, 1], bool), dist, np.arange(4) + 10, 2)
    assert e["count"].tolist() == [1, 2] and e["totals"] == [3, 0, 1, 2]


def test_the_weight_is_clamped_below_zero_and_above_two():
    dist = np.array([-1e-7, 2.0000002, 2.0, 1.0, np.float32(1.0) + np.float32(2.0 ** -23)], np.float32)
    assert weight(dist).tolist() == [0, 1 << 31, 1 << 31, 1 << 30, (1 << 30) + (1 << 7)]
    e = expected_summary(np.zeros(5, np.uint32), np.ones(5, bool), np.ones(5, bool), dist, np.arange(5), 1)
    assert e["spread"][0] == (1 << 32) + (1 << 31) + (1 << 7) and e["cover"][0] == 0 and e["odd"][0] == 1
    assert weight(np.float32(np.inf)) == 1 << 31 and weight(np.float32(-np.inf)) == 0


def test_typical_order_lists_each_group_by_key_then_row():
    labels = np.array([1, 0, 1, NO_LABEL, 1, 0, 1, 1], np.uint32)
    dist = np.array([0.5, 0.25, NAN, np.inf, 0.0, 0.25, -0.0, np.inf], np.float32)
    got = typical_order(labels, dist)
    assert [g.tolist() for g in got] == [[1, 5], [6, 4, 0, 2]]      # -0 first, the NaN last, the +inf rows are no members
    assert [g.tolist() for g in typical_order(labels, dist, 3)] == [[1, 5], [6, 4, 0, 2], []]
    assert np.array_equal(dist_keys(dist), dist_key(dist))
    assert typical_order(np.zeros(0, np.uint32), np.zeros(0, np.float32)) == []


# ---- the bindings -----------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert mi.mi_abi_version() == 4
    assert len(_lib.SYMBOLS["mi_knn_summarize"][1]) == 13 and len(_lib.SYMBOLS["mi_index_folder_overview"][1]) == 10
    for cls, names in ((EmbeddingTable, ("summarize", "summarize_stats")),
                       (ImageIndex, ("folder_overview", "cluster_overview", "theme_overview"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in ("mi_knn_summarize(", "mi_knn_summarize_stats(", "mi_index_folder_overview("):
        assert name in hpp, name
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"summary.hip"' in build


def test_null_handles_and_bad_group_counts_return_codes_without_a_device(mi):
    C = 4
    cent = np.full((C, 8), -7.0, np.float32)
    u64 = [np.full(C, 7, np.uint64) for _ in range(5)]
    f32 = [np.full(C, -7.0, np.float32) for _ in range(2)]
    dist, totals = np.full(16, -7.0, np.float32), np.full(4, 7, np.uint64)
    labels = np.zeros(16, np.uint32)

    def call(h, c):
        return mi.mi_knn_summarize(h, labels.ctypes.data, c, cent.ctypes.data, u64[0].ctypes.data, u64[1].ctypes.data, f32[0].ctypes.data,
                                   u64[2].ctypes.data, f32[1].ctypes.data, u64[3].ctypes.data, u64[4].ctypes.data, dist.ctypes.data,
                                   totals.ctypes.data)

    fake = ctypes.c_void_p(16)          # a handle that is never followed: every case below is refused in front of it
    assert call(None, C) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert call(fake, 0) == MI_ERR_INVALID
    assert b"C must be" in mi.mi_last_error()
    assert call(fake, 65537) == MI_ERR_UNSUPPORTED
    assert b"65536" in mi.mi_last_error()
    assert call(fake, 0xFFFFFFFF) == MI_ERR_UNSUPPORTED
    assert mi.mi_knn_summarize_stats(None, (ctypes.c_uint64 * 4)()) == MI_ERR_INVALID
    assert mi.mi_knn_summarize_stats(fake, None) == MI_ERR_INVALID
    n = ctypes.c_uint32(7)
    assert mi.mi_index_folder_overview(None, C, *(a.ctypes.data for a in (u64[0], u64[1], f32[0], u64[2], f32[1], u64[3], u64[4])),
                                       ctypes.byref(n)) == MI_ERR_INVALID
    assert mi.mi_index_folder_overview(fake, C, *(a.ctypes.data for a in (u64[0], u64[1], f32[0], u64[2], f32[1], u64[3], u64[4])),
                                       None) == MI_ERR_INVALID
    assert np.all(cent == -7.0) and all(np.all(a == 7) for a in u64) and all(np.all(a == -7.0) for a in f32)
    assert np.all(dist == -7.0) and np.all(totals == 7) and n.value == 7


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_summary_host.cpp: a stand-alone program over csrc/summary_host.h — the argument rules, the weight, the
    keys and the decoding of the per-group slots — built with the address and undefined-behaviour sanitizers; it needs
    neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_summary_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_summary_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
