"""mi_knn_search_compound without a GPU: the numpy restatement of the contract (include/mi355clip.h) on hand-made distance
arrays, and the bindings.

The restatement works on per-term distance arrays alone; the GPU tests (tests/test_compound_gpu.py) feed it the CPU oracle's
orc_cosine_dist(term, rows) per term and compare the device's ids and distance bits with it for equality."""
import ctypes
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable

NEW = ["mi_knn_search_compound", "mi_knn_search_compound_stats", "mi_knn_sharded_search_compound", "mi_index_search_compound"]
NO_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID = -1


# ---- the restatement ------------------------------------------------------------------------------------------------

def dist_key(d):
    """dist_to_u32: numeric order, -0 before +0, every NaN last and equal"""
    d = np.asarray(d, np.float32)
    b = d.view(np.uint32)
    return np.where(np.isnan(d), np.uint32(0xFFFFFFFF), np.where(b >> 31 == 1, ~b, b | np.uint32(0x80000000))).astype(np.uint32)


def key_dist(key):
    """u32_to_dist: a NaN comes back as 0x7FC00000"""
    key = np.asarray(key, np.uint32)
    b = np.where(key == 0xFFFFFFFF, np.uint32(0x7FC00000), np.where(key >> 31 == 1, key & np.uint32(0x7FFFFFFF), ~key))
    return b.astype(np.uint32).view(np.float32)


def _terms_by_rows(D, n):
    D = np.asarray(D, np.float32)
    return D if D.ndim == 2 else D.reshape(0 if D.size == 0 else -1, n)


def expected(D_pos, D_neg, neg_within, mode, k, ids):
    """D_pos [n_pos, n] / D_neg [n_neg, n]: every candidate's distance to every term; ids [n].
    -> idx [k], dist [k], the hits' coordinates in rank order, candidates excluded, candidates (not excluded) with a NaN score"""
    ids = np.asarray(ids, np.uint64)
    D_pos, D_neg = _terms_by_rows(D_pos, len(ids)), _terms_by_rows(D_neg, len(ids))
    keys = dist_key(D_pos)
    score = keys.max(axis=0) if mode == "all" else keys.min(axis=0)
    excluded = np.zeros(len(ids), bool)
    with np.errstate(invalid="ignore"):
        for d, w in zip(D_neg, np.asarray(neg_within, np.float32).reshape(-1)):
            excluded |= d <= w          # an ordinary float comparison: a NaN never excludes
    nan = ~excluded & (score == 0xFFFFFFFF)
    cand = np.flatnonzero(~excluded & ~nan)
    order = cand[np.lexsort((ids[cand], score[cand]))][:k]
    idx, dist = np.full(k, NO_ID, np.uint64), np.full(k, np.inf, np.float32)
    idx[:order.size], dist[:order.size] = ids[order], key_dist(score[order])
    return idx, dist, order, int(excluded.sum()), int(nan.sum())


def expected_term_dist(D_pos, D_neg, order, k):
    """term_dist [k, n_pos + n_neg]: the hits' distances, positives first; +inf in the padding"""
    D_pos = np.asarray(D_pos, np.float32).reshape(len(D_pos), -1)
    D = np.concatenate([D_pos, _terms_by_rows(D_neg, D_pos.shape[1])])
    out = np.full((k, D.shape[0]), np.inf, np.float32)
    out[:order.size] = D[:, order].T
    return out


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- the restatement on hand-made arrays ------------------------------------------------------------------------------

def test_key_transform_orders_and_round_trips():
    d = np.array([-np.inf, -1.5, -0.0, 0.0, 1e-45, 0.25, 2.0, np.inf, np.nan], np.float32)
    k = dist_key(d)
    assert np.all(np.diff(k.astype(np.int64)) > 0)          # strictly ascending, -0 before +0, NaN last
    assert k[-1] == 0xFFFFFFFF and dist_key(np.float32(-np.nan)) == 0xFFFFFFFF
    assert np.array_equal(bits(key_dist(k))[:-1], bits(d)[:-1]) and bits(key_dist(k))[-1] == 0x7FC00000


def test_minus_zero_before_plus_zero():
    ids = np.arange(4, dtype=np.uint64)
    D = np.array([[0.0, -0.0, 0.0, -0.0]], np.float32)
    idx, dist, order, ex, nan = expected(D, [], [], "all", 4, ids)
    assert idx.tolist() == [1, 3, 0, 2] and bits(dist).tolist() == [0x80000000, 0x80000000, 0, 0]
    # ALL takes the LARGER key: (+0, -0) scores +0; ANY the smaller: -0 — and the score carries that term's bits
    D2 = np.array([[0.0, 0.5], [-0.0, 0.5]], np.float32)
    assert bits(expected(D2, [], [], "all", 1, ids[:2])[1])[0] == 0
    assert bits(expected(D2, [], [], "any", 1, ids[:2])[1])[0] == 0x80000000


def test_nan_in_one_term():
    ids = np.array([10, 11, 12], np.uint64)
    D = np.array([[0.1, np.nan, np.nan], [0.3, 0.2, np.nan]], np.float32)
    idx, dist, order, ex, nan = expected(D, [], [], "all", 3, ids)      # one NaN term makes the score NaN: left out
    assert idx.tolist() == [10, int(NO_ID), int(NO_ID)] and bits(dist)[0] == bits(np.float32(0.3)) and nan == 2
    idx, dist, order, ex, nan = expected(D, [], [], "any", 3, ids)      # ignored unless every term is NaN
    assert idx.tolist() == [10, 11, int(NO_ID)] and np.array_equal(bits(dist[:2]), bits([0.1, 0.2])) and nan == 1
    assert np.isinf(dist[2])


def test_negative_threshold_exact_and_one_below():
    ids = np.arange(3, dtype=np.uint64)
    D = np.array([[0.1, 0.2, 0.3]], np.float32)
    Dn = np.array([[0.5, 0.25, np.nan]], np.float32)
    at = np.float32(0.25)
    idx, dist, order, ex, nan = expected(D, Dn, [at], "all", 3, ids)                      # exactly at the threshold: excluded
    assert idx.tolist() == [0, 2, int(NO_ID)] and ex == 1 and nan == 0
    idx, dist, order, ex, nan = expected(D, Dn, [np.nextafter(at, np.float32(0))], "all", 3, ids)   # one ulp below: returned
    assert idx.tolist() == [0, 1, 2] and ex == 0
    idx, dist, order, ex, nan = expected(D, Dn, [np.inf], "all", 3, ids)                  # +inf: all but the NaN distance
    assert idx.tolist() == [2, int(NO_ID), int(NO_ID)] and ex == 2
    td = expected_term_dist(D, Dn, order, 3)
    assert bits(td[0]).tolist() == [bits(np.float32(0.3)), bits(np.float32(np.nan))] and np.all(np.isinf(td[1:]))


def test_ties_go_to_the_lower_id_and_k_beyond_the_hits():
    ids = np.array([7, 3, 9, 5], np.uint64)
    D = np.array([[0.5, 0.5, 0.5, 0.25], [0.5, 0.1, 0.5, 0.25]], np.float32)
    idx, dist, order, ex, nan = expected(D, [], [], "all", 6, ids)
    assert idx.tolist() == [5, 3, 7, 9, int(NO_ID), int(NO_ID)] and order.tolist() == [3, 1, 0, 2]
    assert np.all(np.isinf(dist[4:])) and np.array_equal(bits(dist[:4]), bits([0.25, 0.5, 0.5, 0.5]))
    idx, dist, order, ex, nan = expected(D, [], [], "any", 2, ids)
    assert idx.tolist() == [3, 5] and np.array_equal(bits(dist), bits([0.1, 0.25]))
    # a repeated positive term changes nothing
    again = expected(np.concatenate([D, D[:1]]), [], [], "all", 6, ids)
    assert np.array_equal(again[0], expected(D, [], [], "all", 6, ids)[0])


# ---- the bindings -----------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert "#define MI_COMPOUND_ALL 0" in header and "#define MI_COMPOUND_ANY 1" in header
    args = _lib.SYMBOLS["mi_knn_search_compound"][1]
    assert len(args) == 13 and args[2:4] == [ctypes.c_uint32, ctypes.c_int] and args[6:8] == [ctypes.c_uint32, ctypes.c_uint32]
    assert len(_lib.SYMBOLS["mi_knn_sharded_search_compound"][1]) == 12 and len(_lib.SYMBOLS["mi_index_search_compound"][1]) == 14
    assert mi.mi_abi_version() == 4
    for cls, names in ((EmbeddingTable, ("knn_compound", "knn_compound_stats")), (ShardedTable, ("knn_compound",)),
                       (ImageIndex, ("web_search_compound",))):
        for name in names:
            assert callable(getattr(cls, name)), name
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    assert "mi_knn_search_compound(" in hpp and "mi_index_search_compound(" in hpp


def test_a_null_handle_is_invalid_without_a_device(mi):
    v = np.zeros(768, np.float32)
    idx, dist = np.full(4, 7, np.uint64), np.full(4, -7.0, np.float32)
    rc = mi.mi_knn_search_compound(None, v.ctypes.data, 1, 0, None, None, 0, 4, None, 0, idx.ctypes.data, dist.ctypes.data, None)
    assert rc == MI_ERR_INVALID and np.all(idx == 7) and np.all(dist == -7.0)
    assert mi.mi_knn_sharded_search_compound(None, v.ctypes.data, 1, 0, None, None, 0, 4, None, 0, idx.ctypes.data, dist.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_index_search_compound(None, v.ctypes.data, 1, 0, None, None, 0, None, 0, 4, idx.ctypes.data, dist.ctypes.data, None, None) == MI_ERR_INVALID
    assert mi.mi_knn_search_compound_stats(None, None) == MI_ERR_INVALID


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_compound_host.cpp: a stand-alone program over csrc/compound_host.h, built with the address and
    undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_compound_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_compound_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
