"""mi_knn_sharded_kmeans, mi_knn_sharded_kmeans_stats and the option "kmeans_fixed_sum" without a GPU: the bindings, the
argument checks that come in front of any device work, the host-only rules (csrc/kmeans_fixed_host.h) under the sanitizers,
and the numpy restatement of the fixed-point update (expected_fixed_update) that tests/test_kmeans_sharded_gpu.py compares
the device with to the bit."""
import ctypes
import os

import numpy as np

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ShardedTable

NEW = ["mi_knn_sharded_kmeans", "mi_knn_sharded_kmeans_stats"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
DIM = 768


def expected_fixed_update(rows, inv, labels, dist, C, previous):
    """One update of k-means on the exact integer sums (include/mi355clip.h, at mi_knn_kmeans): the centroids [C, dim] float32
    from the rows, their 1 / |x| as the device holds it, and an assign's labels / dist; an empty cluster keeps `previous`."""
    v = np.asarray(rows, np.float32) * np.asarray(inv, np.float32)[:, None]            # the fp32 product of the float path
    with np.errstate(invalid="ignore"):
        q = np.where(np.abs(v) < 2.0, np.rint(v.astype(np.float64) * 2.0 ** 30), 0.0).astype(np.int64)   # exact scaling, ties to even
    out = np.array(previous, dtype=np.float32).reshape(C, -1).copy()
    member = (np.asarray(labels) < C) & ~np.isnan(dist)
    for c in range(C):
        m = member & (np.asarray(labels) == c)
        if m.any():
            out[c] = (q[m].sum(axis=0).astype(np.float64) * 2.0 ** -30 / np.float64(m.sum())).astype(np.float32)
    return out


def fixed_bound(unit_members, want):
    """per component: 12 roundings of a member's fp32 x / |x| (the sum of squares carries at most 18 at dim 768, the root halves
    them, root, reciprocal and product add 1.5), half a unit of 2^-30 from the quantisation, one rounding of the stored
    centroid.  No term grows with the cluster's size."""
    return 12.0 * 2.0 ** -24 * np.abs(unit_members).mean(axis=0) + 2.0 ** -31 + 2.0 ** -24 * np.abs(want)


def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
        assert name + "(" in hpp, name
    assert '"kmeans_fixed_sum"' in header
    assert mi.mi_abi_version() == 4
    assert len(_lib.SYMBOLS["mi_knn_sharded_kmeans"][1]) == 9 and len(_lib.SYMBOLS["mi_knn_sharded_kmeans_stats"][1]) == 2
    for name in ("kmeans", "kmeans_stats"):
        assert callable(getattr(ShardedTable, name)), name
    import inspect
    assert inspect.signature(EmbeddingTable.kmeans).parameters["fixed_sum"].default is None
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"kmeans_sharded.hip"' in build


def test_null_handles_and_bad_arguments_return_codes_without_a_device(mi):
    cent = np.full((2, DIM), 3.0, np.float32)
    labels, dist = np.full(4, 7, np.uint32), np.full(4, -7.0, np.float32)
    iters, changed, obj = ctypes.c_uint32(7), ctypes.c_uint64(7), ctypes.c_double(-7.0)
    tail = (labels.ctypes.data, dist.ctypes.data, ctypes.byref(iters), ctypes.byref(changed), ctypes.byref(obj))
    fake = ctypes.c_void_p(16)          # a handle that is never followed: every case below is refused in front of it
    assert mi.mi_knn_sharded_kmeans(None, cent.ctypes.data, 2, 3, *tail) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert mi.mi_knn_sharded_kmeans(fake, None, 2, 3, *tail) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_kmeans(fake, cent.ctypes.data, 0, 3, *tail) == MI_ERR_INVALID
    assert b"C must be" in mi.mi_last_error()
    assert mi.mi_knn_sharded_kmeans(fake, cent.ctypes.data, 65537, 3, *tail) == MI_ERR_UNSUPPORTED
    assert b"65536" in mi.mi_last_error()
    assert mi.mi_knn_sharded_kmeans_stats(None, (ctypes.c_uint64 * 4)()) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_kmeans_stats(fake, None) == MI_ERR_INVALID
    assert np.all(cent == 3.0) and np.all(labels == 7) and np.all(dist == -7.0)
    assert (iters.value, changed.value, obj.value) == (7, 7, -7.0)


def test_kmeans_plus_plus_on_a_sharded_table_says_why():
    import pytest
    with pytest.raises(ValueError, match="across shards"):
        ShardedTable.kmeans(object(), 4, init="kmeans++")   # (refused before the handle is looked at)


def test_host_rules_under_the_sanitizers(tmp_path):
    """tests/cpp/test_kmeans_fixed_host.cpp: a stand-alone program over csrc/kmeans_fixed_host.h — the quantisation on its edge
    values, the conversion, the merge against a sum in another order — built with the address and undefined-behaviour
    sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_kmeans_fixed_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_kmeans_fixed_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def _gaussian(n=1500, C=6):
    rng = np.random.default_rng(31)
    rows = rng.standard_normal((n, DIM)).astype(np.float32) * rng.uniform(0.1, 10.0, (n, 1)).astype(np.float32)
    inv = (np.float32(1.0) / np.sqrt(np.sum(rows * rows, axis=1, dtype=np.float32))).astype(np.float32)
    labels = rng.integers(0, C + 1, n).astype(np.uint32)      # C: belongs to nothing
    labels[labels == C] = 0xFFFFFFFF
    labels[labels == C - 1] = 0                               # the last cluster is empty
    dist = rng.uniform(0.0, 1.0, n).astype(np.float32)
    dist[::97] = np.nan                                       # no member either
    return rows, inv, labels, dist, C


def test_restatement_against_fp64_means():
    rows, inv, labels, dist, C = _gaussian()
    previous = np.full((C, DIM), 5.0, np.float32)
    got = expected_fixed_update(rows, inv, labels, dist, C, previous)
    unit = rows.astype(np.float64) / np.linalg.norm(rows.astype(np.float64), axis=1, keepdims=True)
    worst = 0.0
    for c in range(C):
        m = (labels == c) & ~np.isnan(dist)
        if c == C - 1:
            assert not m.any() and np.array_equal(got[c], previous[c])
            continue
        assert m.sum() > 100
        want = unit[m].mean(axis=0)
        err, bound = np.abs(got[c].astype(np.float64) - want), fixed_bound(unit[m], want)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (c, float(np.max(err / bound)))
    print(f"largest error / bound: {worst:.3f}")


def test_restatement_ignores_the_order_of_the_rows_and_the_rows_that_must_not_count():
    rows, inv, labels, dist, C = _gaussian()
    previous = np.zeros((C, DIM), np.float32)
    want = expected_fixed_update(rows, inv, labels, dist, C, previous)
    p = np.random.default_rng(32).permutation(rows.shape[0])
    got = expected_fixed_update(rows[p], inv[p], labels[p], dist[p], C, previous)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a row outside every cluster may hold anything, an inf or NaN product included
    out = np.flatnonzero(labels == 0xFFFFFFFF)[:3]
    rows2, inv2 = rows.copy(), inv.copy()
    rows2[out[0], 5], inv2[out[1]], rows2[out[2]] = np.inf, np.nan, 1e30
    got = expected_fixed_update(rows2, inv2, labels, dist, C, previous)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # ... and a member's inf or NaN component adds 0 (the guard of the rule)
    member = np.flatnonzero((labels == 1) & ~np.isnan(dist))[0]
    rows3 = rows.copy()
    rows3[member, 7] = np.inf
    got = expected_fixed_update(rows3, inv, labels, dist, C, previous)
    assert np.all(np.isfinite(got))
