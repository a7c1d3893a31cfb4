"""mi_knn_search_diverse without a GPU: the numpy restatement of the contract (include/mi355clip.h), what it does on a
planted corpus of bursts, and the bindings.

The restatement takes everything from the CPU oracle: the pool is orc_knn's list, G[a, b] = what the single pass with q = row a
reports for row b (orc_cosine_dist), read at (min, max).  The GPU tests (tests/test_diverse_gpu.py) compare the device's ids,
distance bits, hidden counts, rep and n_kept with it for equality."""
import ctypes
import os

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex
from oracle.binding import orc_cosine_dist, orc_knn

NEW = ["mi_knn_search_diverse", "mi_knn_search_diverse_stats", "mi_index_search_diverse"]
NO_ID, NO_LABEL = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint32(0xFFFFFFFF)
DIM = 768
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------

def greedy_diverse(order, dists, G, k, min_gap):
    """order: the pool in rank order as coordinates of G (ascending in id), padding and NaN entries already removed; dists:
    their distances.  -> (kept coordinates, kept distances, hidden [n_kept], rep [P] with -1 = left over)"""
    kept, hidden, rep = [], [], np.full(len(order), -1, np.int64)
    gap = np.float32(min_gap)
    for r, x in enumerate(order):
        ks = np.asarray(kept, np.int64)
        g = G[np.minimum(ks, x), np.maximum(ks, x)] if ks.size else np.zeros(0, np.float32)
        first = np.flatnonzero(g <= gap)      # (a NaN compares false: never a conflict); kept is in rank = slot order
        if first.size:
            hidden[first[0]] += 1
            rep[r] = first[0]
        elif len(kept) < k:
            rep[r] = len(kept)
            kept.append(int(x))
            hidden.append(0)
    at = [int(np.flatnonzero(rep == s)[0]) for s in range(len(kept))]
    return np.asarray(kept, np.int64), np.asarray(dists, np.float32)[at], np.asarray(hidden, np.uint32), rep


def expected(ids, dists, G, coord_of, k, pool, min_gap):
    """The call's outputs from a search's list (ids / dists [pool], padding and NaN entries still in it): idx [k], dist [k],
    hidden [k], rep [pool], n_kept, entries hidden.  coord_of(id) -> coordinate of G."""
    ok = (ids != NO_ID) & ~np.isnan(dists)
    ids, dists = ids[ok], dists[ok]
    order = np.array([coord_of(int(i)) for i in ids], np.int64)
    kept, kd, hid, rep = greedy_diverse(order, dists, G, k, min_gap)
    idx, dist = np.full(k, NO_ID, np.uint64), np.full(k, np.inf, np.float32)
    hidden, rep_out = np.zeros(k, np.uint32), np.full(pool, NO_LABEL, np.uint32)
    n = kept.size
    idx[:n] = ids[[int(np.flatnonzero(rep == s)[0]) for s in range(n)]]
    dist[:n], hidden[:n] = kd, hid
    rep_out[:rep.size] = np.where(rep < 0, int(NO_LABEL), rep).astype(np.uint32)
    return idx, dist, hidden, rep_out, n, int(hid.sum())


def distance_matrix(orc, rows):
    """G[a, b] = what the single pass with q = row a reports for row b"""
    return np.stack([orc_cosine_dist(orc, rows[a], rows) for a in range(rows.shape[0])])


def planted_bursts():
    """2000 random rows and 38 bursts of 8 noisy, rescaled copies of one of them"""
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((2304, 768)).astype(np.float32)
    at = 2000
    for burst in range(38):
        base = rows[rng.integers(0, 2000)]
        for member in range(8):
            s = rng.uniform(0.05, 0.35)
            rows[at] = ((base + s * rng.standard_normal(768)) * rng.uniform(0.1, 10)).astype(np.float32)
            at += 1
    return rows


def planted_queries(rows):
    """three burst members, two random rows with noise added"""
    rng = np.random.default_rng(12)
    qs = [rows[2003], rows[2100], rows[2301]]
    qs += [(rows[r] + 0.3 * rng.standard_normal(768)).astype(np.float32) for r in (17, 1234)]
    return np.stack(qs).astype(np.float32)


def chains(order, rep, kept, G, min_gap):
    """kept entries that conflict with an EARLIER entry hidden behind something else: connected components would have merged them"""
    gap, n, slot_rank = np.float32(min_gap), 0, {}
    for r in range(len(order)):
        if rep[r] >= 0 and rep[r] not in slot_rank:
            slot_rank[int(rep[r])] = r
    kept_ranks = set(slot_rank.values())
    hidden_ranks = np.array([r for r in range(len(order)) if rep[r] >= 0 and r not in kept_ranks], np.int64)
    for r in sorted(kept_ranks):
        h = hidden_ranks[hidden_ranks < r]
        if h.size == 0:
            continue
        x, ys = order[r], order[h]
        n += bool(np.any(G[np.minimum(ys, x), np.maximum(ys, x)] <= gap))
    return n


@pytest.fixture(scope="module")
def corpus(orc):
    rows = planted_bursts()
    return rows, distance_matrix(orc, rows)


# ---- the contract on the planted corpus -------------------------------------------------------------------------------

def test_bursts_are_hidden_and_chains_are_cut(orc, corpus):
    rows, G = corpus
    for q in planted_queries(rows)[:3]:
        ids, dists = orc_knn(orc, q, rows, 2304)
        idx, dist, hidden, rep, n_kept, n_hidden = expected(ids, dists, G, int, 2304, 2304, 0.05)
        order = ids.astype(np.int64)
        rep_i = np.where(rep == NO_LABEL, -1, rep.astype(np.int64))
        n_chains = chains(order, rep_i, idx[:n_kept], G, 0.05)
        print(f"kept {n_kept}, hidden {n_hidden}, chains {n_chains}")
        assert n_kept + n_hidden == 2304 and hidden.sum() == n_hidden
        assert n_hidden >= 100
        assert n_chains >= 20
        # greedy, not components: a kept entry never conflicts with an earlier KEPT one, though it may with a hidden one
        kept = idx[:n_kept].astype(np.int64)
        for j in range(1, n_kept, 97):
            g = G[np.minimum(kept[:j], kept[j]), np.maximum(kept[:j], kept[j])]
            assert not np.any(g <= np.float32(0.05))


def test_infinite_gap_keeps_exactly_one(orc, corpus):
    rows, G = corpus
    ids, dists = orc_knn(orc, planted_queries(rows)[0], rows, 300)
    idx, dist, hidden, rep, n_kept, n_hidden = expected(ids, dists, G, int, 50, 300, np.inf)
    assert n_kept == 1 and idx[0] == ids[0] and hidden[0] == 299 and n_hidden == 299
    assert np.all(rep == 0) and np.all(idx[1:] == NO_ID) and np.all(np.isinf(dist[1:]))


def test_zero_gap_without_copies_is_the_plain_top_k(orc, corpus):
    rows, G = corpus
    plain = rows[:2000]
    ids, dists = orc_knn(orc, planted_queries(rows)[3], plain, 200)
    idx, dist, hidden, rep, n_kept, n_hidden = expected(ids, dists, G, int, 50, 200, 0.0)
    assert n_kept == 50 and n_hidden == 0 and not hidden.any()
    assert np.array_equal(idx, ids[:50]) and np.array_equal(dist.view(np.uint32), dists[:50].view(np.uint32))
    assert np.array_equal(rep[:50], np.arange(50, dtype=np.uint32)) and np.all(rep[50:] == NO_LABEL)


def test_a_chain_of_three_by_hand():
    # A ~ B, B ~ C, A !~ C in rank order: A kept, B behind A, C kept
    G = np.full((3, 3), 1.0, np.float32)
    G[0, 1] = G[1, 2] = 0.01
    kept, kd, hidden, rep = greedy_diverse(np.array([0, 1, 2]), np.array([0.1, 0.2, 0.3], np.float32), G, 3, 0.05)
    assert kept.tolist() == [0, 2] and hidden.tolist() == [1, 0] and rep.tolist() == [0, 0, 1]
    # with k = 1 the third is left over; a NaN never conflicts
    kept, kd, hidden, rep = greedy_diverse(np.array([0, 1, 2]), np.array([0.1, 0.2, 0.3], np.float32), G, 1, 0.05)
    assert kept.tolist() == [0] and hidden.tolist() == [1] and rep.tolist() == [0, 0, -1]
    G[0, 1] = np.nan
    kept, kd, hidden, rep = greedy_diverse(np.array([0, 1, 2]), np.array([0.1, 0.2, 0.3], np.float32), G, 3, np.inf)
    assert kept.tolist() == [0, 1] and hidden.tolist() == [1, 0] and rep.tolist() == [0, 1, 0]


# ---- the bindings -----------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_the_abi_version_stays(mi):
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert _lib.SYMBOLS["mi_knn_search_diverse"][1][2:5] == [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float]
    assert _lib.SYMBOLS["mi_knn_search_diverse"][1][-1] == ctypes.POINTER(ctypes.c_uint32)
    assert mi.mi_abi_version() == 4
    for cls, names in ((EmbeddingTable, ("knn_diverse", "knn_diverse_stats")), (ImageIndex, ("web_search_diverse",))):
        for name in names:
            assert callable(getattr(cls, name)), name


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_diverse_host.cpp: a stand-alone program over csrc/diverse_host.h, built with the address and
    undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_diverse_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_diverse_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
