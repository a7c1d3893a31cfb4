"""mi_knn_kmeans_seed without a GPU: the numpy restatement of the contract (include/mi355clip.h), the pick rule on hand-made
weights, the quality of the seeds on a planted corpus of very unequal clusters, and the bindings.

The restatement takes the distances from a callback, dist_from(c) -> float32[S] = what mi_knn_search(q = candidate c)
reports for every candidate (the CPU oracle's kNN with k = rows gives those bits), and does all sums in integers; the GPU
tests (tests/test_kmeans_seed_gpu.py) compare the device's picks, rows, potential and fallback count with it for equality."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, initial_centroid_rows
from oracle.binding import orc_cosine_dist, orc_knn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi_knn_kmeans_seed", "mi_knn_kmeans_seed_stats"]
MI_ERR_INVALID = -1
MASK64 = (1 << 64) - 1


# ---- the restatement ------------------------------------------------------------------------------------------------

def splitmix64(seed, n):
    """z_0 .. z_{n-1}"""
    out, state = [], int(seed) & MASK64
    for _ in range(n):
        state = (state + 0x9E3779B97F4A7C15) & MASK64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        out.append(z ^ (z >> 31))
    return out


def pick_position(w, z, picked):
    """one pick over the weights w (uint32) -> (position, was it a fallback pick)"""
    prefix = np.cumsum(np.asarray(w, np.uint64), dtype=np.uint64)   # (exact: S x 2^31 < 2^64)
    total = int(prefix[-1])
    if total == 0:
        return int(np.flatnonzero(~np.asarray(picked, bool))[0]), True
    T = (int(z) * total) >> 64
    return int(np.searchsorted(prefix, np.uint64(T), side="right")), False   # the smallest p with prefix[p] > T


def weights_of(D, usable, picked):
    w = np.zeros(D.shape[0], np.uint32)
    ok = usable & ~picked & ~np.isnan(D)
    scaled = np.minimum(np.maximum(D[ok], np.float32(0.0)), np.float32(2.0)) * np.float32(2.0 ** 30)   # exact in fp32
    w[ok] = np.floor(scaled).astype(np.int64).astype(np.uint32)
    return w


def restate_seed(S, C, seed, dist_from, usable=None):
    """-> (positions in pick order, potential, fallback picks).  usable: bool [S], or None = from dist_from(p)[p]"""
    if usable is None:
        usable = np.array([not np.isnan(dist_from(p)[p]) for p in range(S)])
    usable = np.asarray(usable, bool)
    z = splitmix64(seed, C + 1)
    D = np.full(S, np.nan, np.float32)
    picked = np.zeros(S, bool)
    w = usable.astype(np.uint32)
    picks, fallbacks = [], 0
    for j in range(C):
        p, fell_back = pick_position(w, z[j], picked)
        assert not picked[p]
        fallbacks += int(fell_back)
        picks.append(p)
        picked[p] = True
        d = np.asarray(dist_from(p), np.float32)
        with np.errstate(invalid="ignore"):
            lower = ~np.isnan(d) & (np.isnan(D) | (d < D))
        D[lower] = d[lower]
        w = weights_of(D, usable, picked)
    return picks, float(int(np.sum(w.astype(np.uint64)))) / 2.0 ** 30, fallbacks


def oracle_dist_from(orc, rows):
    """dist_from for the candidates `rows` [S, dim] (cached per centre), and their usable flags"""
    rows = np.ascontiguousarray(rows, np.float32)
    S = rows.shape[0]
    cache = {}

    def dist_from(c):
        if c not in cache:
            idx, dist = orc_knn(orc, rows[c], rows, S)   # k = rows: every row's distance, the search's bits
            d = np.empty(S, np.float32)
            d[idx.astype(np.int64)] = dist
            cache[c] = d
        return cache[c]

    usable = np.array([not np.isnan(orc_cosine_dist(orc, rows[p], rows[p:p + 1])[0]) for p in range(S)])
    return dist_from, usable


# ---- 1: the random stream and the pick rule ----------------------------------------------------------------------------

def test_splitmix64_stream():
    # the published test vector of splitmix64 (seed 1234567)
    assert splitmix64(1234567, 3) == [6457827717110365317, 3203168211198807973, 9817491932198370423]
    assert splitmix64(0, 1) == [0xE220A8397B1DCDAF]
    assert splitmix64(MASK64 + 1 + 5, 2) == splitmix64(5, 2)


def test_pick_rule_on_hand_made_weights():
    none = np.zeros(6, bool)
    # total 0: the lowest position not picked before
    assert pick_position([0] * 6, 123, none) == (0, True)
    assert pick_position([0] * 6, MASK64, np.array([1, 1, 0, 1, 0, 0], bool)) == (2, True)
    # a single non-zero weight takes every z
    for z in (0, 1, 1 << 63, MASK64):
        assert pick_position([0, 0, 7, 0], z, none[:4]) == (2, False)
    # T on a boundary: w = [2, 2], total 4, T = floor(z / 2^62); T = 1 is the last of position 0, T = 2 the first of 1
    assert pick_position([2, 2], (1 << 63) - 1, none[:2]) == (0, False)       # T = 1
    assert pick_position([2, 2], 1 << 63, none[:2]) == (1, False)             # T = 2
    assert pick_position([2, 0, 0, 2], 1 << 63, none[:4]) == (3, False)       # zero weights are stepped over
    assert pick_position([0, 2, 2], 0, none[:3]) == (1, False)                # T = 0 is the first position WITH weight
    # weights summing past 2^32: total = 3 * 2^31, T = floor(z * 3 / 2^33)
    big = [1 << 31] * 3
    assert pick_position(big, 0, none[:3]) == (0, False)
    assert pick_position(big, ((1 << 64) // 3), none[:3]) == (0, False)       # T = 2^31 - 1
    assert pick_position(big, ((1 << 64) // 3) + 1, none[:3]) == (1, False)   # T = 2^31
    assert pick_position(big, MASK64, none[:3]) == (2, False)
    assert weights_of(np.array([-1e-7, 0.5, 2.5, np.nan, 1.0, 1.0], np.float32), np.array([1, 1, 1, 1, 0, 1], bool),
                      np.array([0, 0, 0, 0, 0, 1], bool)).tolist() == [0, 1 << 29, 1 << 31, 0, 0, 0]


def test_restatement_falls_back_when_nothing_has_weight():
    """three distinct directions, four copies each: after three picks every D is 0 -> fallbacks at the lowest positions"""
    own = np.array([0, 1, 2] * 4)
    dmat = np.where(own[:, None] == own[None, :], np.float32(0.0), np.float32(1.0)).astype(np.float32)
    picks, potential, fallbacks = restate_seed(12, 6, 3, lambda c: dmat[c])
    assert sorted(own[picks[:3]]) == [0, 1, 2] and fallbacks == 3 and potential == 0.0
    rest = [p for p in range(12) if p not in picks[:3]]
    assert picks[3:] == rest[:3]


# ---- 2: quality on the planted unequal corpus --------------------------------------------------------------------------

def planted_unequal(noise=0.08):
    """16 clusters in dim 256, one holding 82 % of the 1 960 rows; rows scaled by 0.1 .. 10 -> (rows, own)"""
    r = np.random.default_rng(5)
    centres = r.standard_normal((16, 256))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    own = np.concatenate([np.zeros(1600, np.int64), np.repeat(np.arange(1, 16), 24)])
    own = own[r.permutation(own.size)]
    x = centres[own] + noise * r.standard_normal((own.size, 256)) / np.sqrt(256)
    x *= r.uniform(0.1, 10.0, (own.size, 1))
    return x.astype(np.float32), own


@pytest.fixture(scope="module")
def planted(orc):
    rows, own = planted_unequal()
    dist_from, usable = oracle_dist_from(orc, rows)
    return rows, own, dist_from, usable


@pytest.mark.parametrize("seed", range(8))
def test_seeds_cover_the_small_clusters(planted, seed):
    """Observed on the oracle's bits, seeds 0 .. 7: planted clusters covered by the 16 k-means++ seeds
    14, 13, 16, 14, 14, 15, 15, 15; by the uniform choice 6, 2, 6, 4, 2, 3, 3, 3."""
    rows, own, dist_from, usable = planted
    assert usable.all()
    picks, potential, fallbacks = restate_seed(rows.shape[0], 16, seed, dist_from, usable)
    covered = len(set(own[picks].tolist()))
    uniform = len(set(own[initial_centroid_rows(rows.shape[0], [], 16, seed).astype(np.int64)].tolist()))
    print(f"seed {seed}: k-means++ covers {covered} planted clusters, the uniform choice {uniform}; potential {potential:.3f}")
    assert fallbacks == 0 and len(set(picks)) == 16
    assert covered >= 12
    assert covered > uniform


# ---- 3: the surface -----------------------------------------------------------------------------------------------------

def test_header_bindings_and_library_carry_the_new_symbols(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert _lib.SYMBOLS["mi_knn_kmeans_seed"][1][1:3] == [ctypes.c_uint32, ctypes.c_uint64]
    assert _lib.SYMBOLS["mi_knn_kmeans_seed"][1][-1] == ctypes.POINTER(ctypes.c_double)
    assert mi.mi_abi_version() == 4
    hpp = open(os.path.join(ROOT, "image_search_amd", "host", "image_search.hpp")).read()
    assert "mi_knn_kmeans_seed(" in hpp and "mi_knn_kmeans_seed_stats(" in hpp


def test_python_surface():
    for name in ("kmeans_seed", "kmeans_seed_stats"):
        assert callable(getattr(EmbeddingTable, name)), name
    p = inspect.signature(EmbeddingTable.kmeans_seed).parameters
    assert list(p)[1:] == ["k", "seed", "among"] and p["seed"].default == 0 and p["among"].default is None
    for fn in (EmbeddingTable.kmeans, ImageIndex.clusters):
        p = inspect.signature(fn).parameters
        assert p["init"].default == "uniform" and p["sample"].default is None
    t = EmbeddingTable.__new__(EmbeddingTable)   # no handle: the argument is refused before anything is called
    with pytest.raises(ValueError, match="init"):
        t.kmeans(4, init="nonsense")
    t._h = None


def test_null_arguments_are_refused_without_a_device(mi):
    rows = np.zeros(4, np.uint64)
    out = (ctypes.c_uint64 * 4)()
    assert mi.mi_knn_kmeans_seed(None, 4, 0, None, 0, rows.ctypes.data, None, None) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert mi.mi_knn_kmeans_seed_stats(None, out) == MI_ERR_INVALID
