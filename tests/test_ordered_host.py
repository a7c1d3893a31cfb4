"""mi_knn_search_ordered and mi_knn_stamp_histogram without a GPU: the numpy restatement of the contract
(include/mi355clip.h) on hand-made columns, the bindings, and the host-only rules (csrc/ordered_host.h) under the sanitizers.

The restatement works on the columns alone; the GPU tests (tests/test_ordered_gpu.py) feed it the CPU oracle's distances and
the predicate's restatement (tests/test_where_host.py: where_rows) and compare the device's ids, distance bits, stamps and
counts with it for equality."""
import ctypes
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import MI_KNN_ORDER_AFTER, MI_KNN_ORDER_DESC, EmbeddingTable, ImageIndex, ShardedTable, make_where
from test_page_host import INF, NO_ID, bits, dist_key, key_dist

NEW = ["mi_knn_search_ordered", "mi_knn_stamp_histogram", "mi_knn_sharded_search_ordered", "mi_knn_sharded_stamp_histogram",
       "mi_index_search_ordered", "mi_index_stamp_histogram"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ---- the restatement ------------------------------------------------------------------------------------------------

def okey(stamps, descending):
    """(uint64) s ^ 2^63, complemented when descending: the unsigned order is the result order"""
    k = np.asarray(stamps, np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    return ~k if descending else k


def expected_ordered(dist_bits, ids, stamps, keep, max_dist, descending, after, k):
    """dist_bits [n] uint32: every row's distance as bits; ids [n]; stamps [n] int64; keep: the candidates (indices into the
    columns: the live rows the predicate keeps).  after: None or (stamp, id).
    -> idx [k], dist [k] float32, stamps [k], counts {within, before, beyond, nan}"""
    keep = np.asarray(keep, np.int64).reshape(-1)
    ids, stamps = np.asarray(ids, np.uint64).reshape(-1)[keep], np.asarray(stamps, np.int64).reshape(-1)[keep]
    dk = dist_key(np.asarray(dist_bits, np.uint32).reshape(-1)[keep].view(np.float32))
    nan = dk == 0xFFFFFFFF
    within = (dk <= dist_key(np.float32(max_dist))) & ~nan        # inclusive, on the key order
    ok = okey(stamps, descending)
    past = np.ones(ids.size, bool)
    if after is not None:
        ck = okey(np.array([after[0]], np.int64), descending)[0]
        past = (ok > ck) | ((ok == ck) & (ids > np.uint64(after[1])))
    cand = np.flatnonzero(within)
    order = cand[np.lexsort((ids[cand], ok[cand]))]
    order = order[past[order]][:k]                                # cut at the cursor
    idx, dist, st = np.full(k, NO_ID, np.uint64), np.full(k, np.inf, np.float32), np.zeros(k, np.int64)
    idx[:order.size], dist[:order.size], st[:order.size] = ids[order], key_dist(dk[order]), stamps[order]
    counts = {"within": int(within.sum()), "before": int((within & ~past).sum()), "beyond": int((~within & ~nan).sum()),
              "nan": int(nan.sum())}
    return idx, dist, st, counts


def expected_hist(dist_bits, stamps, keep, max_dist, edges):
    """hist [len(edges) + 1]: the rows within the bound by the number of edges <= their stamp"""
    keep = np.asarray(keep, np.int64).reshape(-1)
    dk = dist_key(np.asarray(dist_bits, np.uint32).reshape(-1)[keep].view(np.float32))
    within = (dk <= dist_key(np.float32(max_dist))) & (dk != 0xFFFFFFFF)
    b = np.searchsorted(np.asarray(edges, np.int64), np.asarray(stamps, np.int64).reshape(-1)[keep][within], "right")
    return np.bincount(b, minlength=len(edges) + 1).astype(np.uint64)


# ---- the restatement on hand-made columns -------------------------------------------------------------------------------

EXT = np.array([0, I64_MAX, -1, I64_MIN, 1], np.int64)


def run(d, stamps, k, max_dist=INF, descending=False, after=None, keep=None, ids=None):
    d = np.asarray(d, np.float32)
    ids = np.arange(d.size) if ids is None else ids
    keep = np.arange(d.size) if keep is None else keep
    return expected_ordered(bits(d), ids, stamps, keep, max_dist, descending, after, k)


def test_the_extremes_in_both_directions():
    d = np.full(5, 0.5, np.float32)
    idx, dist, st, c = run(d, EXT, 5)
    assert idx.tolist() == [3, 2, 0, 4, 1] and st.tolist() == [I64_MIN, -1, 0, 1, I64_MAX]      # signed, not unsigned
    assert c == {"within": 5, "before": 0, "beyond": 0, "nan": 0}
    idx, dist, st, c = run(d, EXT, 5, descending=True)
    assert idx.tolist() == [1, 4, 0, 2, 3] and st.tolist() == [I64_MAX, 1, 0, -1, I64_MIN]
    idx, dist, st, c = run(d, EXT, 7, descending=True, after=(0, 0))
    assert idx.tolist() == [2, 3] + [int(NO_ID)] * 5 and st.tolist() == [-1, I64_MIN, 0, 0, 0, 0, 0] and np.all(np.isinf(dist[2:]))
    assert c["before"] == 3 and c["within"] == 5
    assert run(d, EXT, 5, after=(I64_MAX, 1))[0].tolist() == [int(NO_ID)] * 5                   # behind the last key: nothing
    assert run(d, EXT, 5, descending=True, after=(I64_MIN, 3))[0].tolist() == [int(NO_ID)] * 5


def test_ties_break_by_id_in_both_directions_and_are_cut_at_the_cursor_id():
    d = np.full(6, 0.25, np.float32)
    stamps = np.array([7, 3, 7, 7, 3, 7], np.int64)
    assert run(d, stamps, 6)[0].tolist() == [1, 4, 0, 2, 3, 5]
    assert run(d, stamps, 6, descending=True)[0].tolist() == [0, 2, 3, 5, 1, 4]                 # ids ascend inside a tie here too
    idx, _, _, c = run(d, stamps, 6, after=(7, 2))
    assert idx.tolist() == [3, 5] + [int(NO_ID)] * 4 and c["before"] == 4
    idx, _, _, c = run(d, stamps, 2, descending=True, after=(7, 2))
    assert idx.tolist() == [3, 5] and c["before"] == 2
    # the cursor's row need not be a candidate (deleted since, or outside the predicate): the cut is the same
    idx, _, _, c = run(d, stamps, 6, after=(7, 2), keep=[0, 1, 3, 4, 5])
    assert idx.tolist() == [3, 5] + [int(NO_ID)] * 4 and c == {"within": 5, "before": 3, "beyond": 0, "nan": 0}
    # a stamp no row holds: everything of larger stamps follows
    assert run(d, stamps, 6, after=(5, 0))[0].tolist() == [0, 2, 3, 5] + [int(NO_ID)] * 2
    # ids that are not the positions
    ids = np.array([1 << 40, 5, (1 << 40) + 1, 9, 6, 7], np.uint64)
    assert run(d, stamps, 6, ids=ids)[0].tolist() == [5, 6, 7, 9, 1 << 40, (1 << 40) + 1]


def test_the_bound_is_inclusive_on_the_key_order_and_nan_counts_apart():
    d = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.25, np.nan, -0.0, 0.0, np.inf], np.float32)
    stamps = np.arange(7, dtype=np.int64)[::-1].copy()
    idx, dist, st, c = run(d, stamps, 7, max_dist=0.5)
    assert idx.tolist() == [5, 4, 2, 0] + [int(NO_ID)] * 3 and c == {"within": 4, "before": 0, "beyond": 2, "nan": 1}
    assert bits(dist[:4]).tolist() == [0, 0x80000000, bits(np.float32(0.25)).item(), bits(np.float32(0.5)).item()]
    idx, _, _, c = run(d, stamps, 7, max_dist=-0.0)
    assert idx.tolist() == [4] + [int(NO_ID)] * 6 and c == {"within": 1, "before": 0, "beyond": 5, "nan": 1}   # -0 before +0
    idx, _, _, c = run(d, stamps, 7)
    assert idx.tolist() == [6, 5, 4, 2, 1, 0, int(NO_ID)] and c == {"within": 6, "before": 0, "beyond": 0, "nan": 1}
    assert run(d, stamps, 7, max_dist=-1.0)[3] == {"within": 0, "before": 0, "beyond": 6, "nan": 1}


def test_the_histogram_counts_an_edge_equal_to_a_stamp_to_the_right():
    d = np.array([0.1, 0.2, 0.3, 0.9, np.nan, 0.1], np.float32)
    stamps = np.array([-5, 0, 0, 0, 0, 7], np.int64)
    keep = np.arange(6)
    assert expected_hist(bits(d), stamps, keep, INF, [0]).tolist() == [1, 4]
    assert expected_hist(bits(d), stamps, keep, 0.5, [-5, 0, 7]).tolist() == [0, 1, 2, 1]
    assert expected_hist(bits(d), stamps, keep, 0.5, [-100]).tolist() == [0, 4]
    assert expected_hist(bits(d), stamps, keep, 0.5, [100, 200]).tolist() == [4, 0, 0]
    assert expected_hist(bits(d), stamps, [0, 5], 0.5, [1]).tolist() == [1, 1]
    assert expected_hist(bits(d), EXT.repeat(2)[:6], keep, INF, [I64_MIN, I64_MAX]).sum() == 5
    for e in ([0], [-5, 0, 7]):
        assert expected_hist(bits(d), stamps, keep, 0.5, e).sum() == run(d, stamps, 1, max_dist=0.5)[3]["within"]


# ---- the bindings -----------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert "#define MI_KNN_ORDER_DESC  1u" in header and "#define MI_KNN_ORDER_AFTER 2u" in header
    assert (MI_KNN_ORDER_DESC, MI_KNN_ORDER_AFTER) == (1, 2) and mi.mi_abi_version() == 4
    args = _lib.SYMBOLS["mi_knn_search_ordered"][1]
    assert len(args) == 12 and args[4] == _lib.c_wherep and _lib.SYMBOLS["mi_knn_sharded_search_ordered"][1] == args
    assert _lib.SYMBOLS["mi_knn_stamp_histogram"][1] == _lib.SYMBOLS["mi_knn_sharded_stamp_histogram"][1]
    for cls, names in ((EmbeddingTable, ("knn_ordered", "timeline", "stamp_histogram")),
                       (ShardedTable, ("knn_ordered", "timeline", "stamp_histogram")),
                       (ImageIndex, ("web_search_ordered", "web_timeline_histogram"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in ("mi_knn_search_ordered(", "mi_knn_sharded_search_ordered(", "mi_index_search_ordered(", "mi_knn_stamp_histogram(",
                 "mi_knn_sharded_stamp_histogram(", "mi_index_stamp_histogram("):
        assert name in hpp, name
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"ordered.hip"' in build


def test_null_handles_and_bad_arguments_return_codes_without_a_device(mi):
    v = np.zeros(768, np.float32)
    idx, dist, stamps = np.full(4, 7, np.uint64), np.full(4, -7.0, np.float32), np.full(4, 7, np.int64)
    counts, hist, found = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64), ctypes.c_uint32(7)
    edges = np.array([1, 2, 3], np.int64)
    w = make_where()
    out = (idx.ctypes.data, dist.ctypes.data, stamps.ctypes.data)
    fake = ctypes.c_void_p(16)          # a handle that is never followed: every case below is refused in front of it
    for fn in (mi.mi_knn_search_ordered, mi.mi_knn_sharded_search_ordered):
        assert fn(None, v.ctypes.data, 4, 1.0, ctypes.byref(w), 0, 0, 0, *out, counts.ctypes.data) == MI_ERR_INVALID
        assert b"null" in mi.mi_last_error()
        assert fn(fake, None, 4, 1.0, None, 0, 0, 0, *out, counts.ctypes.data) == MI_ERR_INVALID
        assert fn(fake, v.ctypes.data, 4, float("nan"), None, 0, 0, 0, *out, counts.ctypes.data) == MI_ERR_INVALID
        assert fn(fake, v.ctypes.data, 4, 1.0, None, 4, 0, 0, *out, counts.ctypes.data) == MI_ERR_INVALID
        assert b"flags" in mi.mi_last_error()
        bad = make_where()
        bad.flags = 2
        assert fn(fake, v.ctypes.data, 4, 1.0, ctypes.byref(bad), 0, 0, 0, *out, counts.ctypes.data) == MI_ERR_INVALID
        assert fn(fake, v.ctypes.data, 0, 1.0, None, 0, 0, 0, *out, counts.ctypes.data) == MI_ERR_INVALID
        assert fn(fake, v.ctypes.data, 4097, 1.0, None, 0, 0, 0, *out, counts.ctypes.data) == MI_ERR_UNSUPPORTED
    for fn in (mi.mi_knn_stamp_histogram, mi.mi_knn_sharded_stamp_histogram):
        assert fn(None, v.ctypes.data, 1.0, None, edges.ctypes.data, 3, hist.ctypes.data) == MI_ERR_INVALID
        assert fn(fake, v.ctypes.data, 1.0, None, edges.ctypes.data, 0, hist.ctypes.data) == MI_ERR_INVALID
        assert fn(fake, v.ctypes.data, 1.0, None, None, 3, hist.ctypes.data) == MI_ERR_INVALID
        assert fn(fake, v.ctypes.data, float("nan"), None, edges.ctypes.data, 3, hist.ctypes.data) == MI_ERR_INVALID
        assert fn(fake, v.ctypes.data, 1.0, None, edges[::-1].copy().ctypes.data, 3, hist.ctypes.data) == MI_ERR_INVALID
        assert b"ascending" in mi.mi_last_error()
    assert mi.mi_index_search_ordered(None, v.ctypes.data, None, 0, 4, 1.0, None, 0, 0, 0, *out, ctypes.byref(found),
                                      counts.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_index_search_ordered(fake, v.ctypes.data, None, 0, 4, 1.0, None, 8, 0, 0, *out, ctypes.byref(found),
                                      counts.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_index_stamp_histogram(None, v.ctypes.data, None, 0, 1.0, None, edges.ctypes.data, 3, hist.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_index_stamp_histogram(fake, v.ctypes.data, None, 0, 1.0, None, edges.ctypes.data, 0, hist.ctypes.data) == MI_ERR_INVALID
    assert np.all(idx == 7) and np.all(dist == -7.0) and np.all(stamps == 7) and np.all(counts == 7) and np.all(hist == 7)
    assert found.value == 7


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_ordered_host.cpp: a stand-alone program over csrc/ordered_host.h — the argument rules, the order key, the
    cursor comparison, the cursor of a shard against a brute-force count, the edge rule, the record and the merge — built with the
    address and undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_ordered_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_ordered_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
