"""mi_knn_search_many_where / mi_knn_neighbors_where / mi_knn_sharded_search_many_where / mi_knn_propose_groups without a
GPU: the bindings, the numpy restatement of the vote (`propose`, what tests/test_search_many_where_gpu.py holds the device
against) on hand-written distance rows, and tests/test_search_many_host.py's emulation of stage 1 with a column mask: a
masked column never enters a residue slot and is never emitted, and the exact top m OF THE UNMASKED columns is always inside
the emitted set — also under the mask that leaves one residue only (c % 16 == 0 at m = 16), where no threshold forms and
every unmasked column is emitted."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import NO_GROUP, EmbeddingTable, ImageIndex, ShardedTable
from test_join_bound import EPS2
from test_search_many_host import cosines, hard_corpus, thresholds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi_knn_search_many_where", "mi_knn_neighbors_where", "mi_knn_sharded_search_many_where", "mi_knn_propose_groups",
       "mi_knn_propose_groups_stats"]
MI_ERR_INVALID = -1
INF = np.float32(np.inf)
NAN = np.float32(np.nan)


def test_header_bindings_and_library_carry_the_new_symbols(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert _lib.SYMBOLS["mi_knn_search_many_where"][1] == _lib.SYMBOLS["mi_knn_sharded_search_many_where"][1]
    assert _lib.SYMBOLS["mi_knn_search_many_where"][1][4] == _lib.c_wherep and len(_lib.SYMBOLS["mi_knn_search_many_where"][1]) == 8
    assert _lib.SYMBOLS["mi_knn_neighbors_where"][1][1:5] == [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, _lib.c_wherep]
    args = _lib.SYMBOLS["mi_knn_propose_groups"][1]
    assert len(args) == 10 and args[1:5] == [ctypes.c_uint32, ctypes.c_float, ctypes.c_uint32, _lib.c_wherep]
    assert mi.mi_abi_version() == 4


def test_python_surface():
    for cls, names in ((EmbeddingTable, ("knn_many_where", "neighbors_where", "propose_groups", "propose_groups_stats")),
                       (ShardedTable, ("knn_many_where",)), (ImageIndex, ("best_per_label_where", "related_where", "suggest_folders"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    p = inspect.signature(EmbeddingTable.neighbors_where).parameters
    assert list(p)[1:4] == ["k", "first", "n"] and p["first"].default == 0 and p["n"].default is None
    p = inspect.signature(EmbeddingTable.propose_groups).parameters
    assert p["k"].default == 10 and p["max_dist"].default == float("inf") and p["ask_group"].default is None
    p = inspect.signature(ImageIndex.suggest_folders).parameters
    assert list(p)[1] == "inbox" and p["k"].default == 10 and p["max_dist"].default == float("inf") and p["min_votes"].default == 1
    assert p["web"].default is False
    p = inspect.signature(ImageIndex.best_per_label_where).parameters
    assert p["names"].default is None and p["k"].default == 10 and p["web"].default is False
    p = inspect.signature(ImageIndex.related_where).parameters
    assert p["k"].default == 10 and p["web"].default is False


def test_null_handles_and_bad_flags_are_refused_without_a_device(mi):
    q = np.zeros((2, 768), np.float32)
    idx, d = np.full(8, 7, np.uint64), np.full(8, 7.0, np.float32)
    g = np.full(8, 7, np.uint32)
    matched = ctypes.c_uint64(7)
    out = (ctypes.c_uint64 * 4)()
    ok = _lib.KnnWhere(0, 0, 0, -(1 << 63), (1 << 63) - 1, 0, 0)
    bad = _lib.KnnWhere(0, 0, 0, -(1 << 63), (1 << 63) - 1, 0, 2)   # an unknown flag bit
    for w in (None, ctypes.byref(ok)):
        assert mi.mi_knn_search_many_where(None, q.ctypes.data, 2, 4, w, idx.ctypes.data, d.ctypes.data, ctypes.byref(matched)) == MI_ERR_INVALID
        assert b"null" in mi.mi_last_error()
        assert mi.mi_knn_neighbors_where(None, 0, 2, 4, w, idx.ctypes.data, d.ctypes.data) == MI_ERR_INVALID
        assert mi.mi_knn_sharded_search_many_where(None, q.ctypes.data, 2, 4, w, idx.ctypes.data, d.ctypes.data, None) == MI_ERR_INVALID
        assert mi.mi_knn_propose_groups(None, 4, np.inf, 0, w, g.ctypes.data, None, None, None, None) == MI_ERR_INVALID
    assert mi.mi_knn_propose_groups_stats(None, out) == MI_ERR_INVALID
    assert mi.mi_knn_search_many_where(None, q.ctypes.data, 2, 4, ctypes.byref(bad), idx.ctypes.data, d.ctypes.data, None) == MI_ERR_INVALID
    assert b"flags" in mi.mi_last_error()
    assert np.all(idx == 7) and np.all(d == 7.0) and np.all(g == 7) and matched.value == 7


# ---- the vote, restated -------------------------------------------------------------------------------------------------------
def dist_keys(d):
    """the search's 32-bit distance key (knn_shared.h dist_to_u32): numeric order, -0 before +0, every NaN last"""
    d = np.ascontiguousarray(d, np.float32)
    b = d.view(np.uint32)
    k = np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))
    return np.where(np.isnan(d), np.uint32(0xFFFFFFFF), k)


def propose(D, groups, live, ask_group, voters, k, max_dist):
    """mi_knn_propose_groups in numpy.  D [rows, rows] float32: D[r, c] = the distance the search reports for row c when the
    query is row r; groups [rows] uint32; live [rows] bool; voters: None or [rows] bool, the rows the voters' predicate keeps.
    -> (group, votes, heard, dist, totals)"""
    D = np.asarray(D, np.float32)
    groups = np.asarray(groups, np.uint32)
    n = groups.size
    ask = live & (groups == np.uint32(ask_group))
    vote = live & (groups != NO_GROUP) & (groups != np.uint32(ask_group))
    if voters is not None:
        vote = vote & voters
    hi = int(dist_keys(np.float32([max_dist]))[0])
    group, votes, heard = np.full(n, NO_GROUP, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    dist = np.full(n, INF, np.float32)
    cols = np.nonzero(vote)[0]
    for r in np.nonzero(ask)[0]:
        key = dist_keys(D[r, cols]).astype(np.int64)
        keep = ~np.isnan(D[r, cols]) & (key <= hi)
        c, key = cols[keep], key[keep]
        L = c[np.lexsort((c, key))][:k]   # by (key, id)
        heard[r] = L.size
        if L.size == 0:
            continue
        count, first = {}, {}
        for pos, col in enumerate(L):
            g = int(groups[col])
            count[g] = count.get(g, 0) + 1
            first.setdefault(g, pos)
        win = min(count, key=lambda g: (-count[g], first[g]))
        group[r], votes[r], dist[r] = win, count[win], D[r, L[first[win]]]
    totals = {"askers": int(ask.sum()), "proposed": int((group != NO_GROUP).sum()), "voters": int(vote.sum()),
              "unanimous": int(((votes == heard) & (heard > 0)).sum())}
    return group, votes, heard, dist, totals


def one_asker(d, groups, k, max_dist=np.inf, live=None, voters=None, ask_group=NO_GROUP):
    """row 0 asks with the distances d to rows 0 .. n - 1 -> its (group, votes, heard, dist bits)"""
    n = len(groups)
    D = np.full((n, n), NAN, np.float32)
    D[0] = np.asarray(d, np.float32)
    live = np.ones(n, bool) if live is None else np.asarray(live, bool)
    g, v, h, dd, tot = propose(D, np.asarray(groups, np.uint32), live, ask_group, voters, k, max_dist)
    return int(g[0]), int(v[0]), int(h[0]), dd[:1].view(np.uint32)[0], tot


def bits(x):
    return np.float32([x]).view(np.uint32)[0]


N = int(NO_GROUP)


def test_restatement_on_hand_written_cases():
    # a count tie: groups 2 and 1 hold two of the four nearest each; 2 holds the nearest entry
    assert one_asker([0, 0.1, 0.2, 0.3, 0.4, 0.9], [N, 2, 1, 1, 2, 1], 4)[:4] == (2, 2, 4, bits(0.1))
    # ... and with k = 5 group 1 has three
    assert one_asker([0, 0.1, 0.2, 0.3, 0.4, 0.9], [N, 2, 1, 1, 2, 1], 5)[:4] == (1, 3, 5, bits(0.2))
    # equal distances: the lower id stands first, so its group is "the nearest" of a tie
    assert one_asker([0, 0.5, 0.5], [N, 4, 3], 2)[:4] == (4, 1, 2, bits(0.5))
    # a NaN row (a zero-norm asker): every entry is removed, no proposal
    assert one_asker([NAN] * 4, [N, 1, 1, 2], 3)[:4] == (N, 0, 0, bits(np.inf))
    # single NaN entries (zero-norm voters) are removed, the rest stays
    assert one_asker([0, NAN, 0.3, NAN], [N, 1, 2, 1], 3)[:4] == (2, 1, 1, bits(0.3))
    # max_dist exactly on an entry's key: inclusive; one key below it: that entry is out
    d = np.float32([0, 0.1, 0.2, 0.3])
    assert one_asker(d, [N, 1, 2, 2], 3, max_dist=d[2])[:4] == (1, 1, 2, bits(0.1))
    assert one_asker(d, [N, 1, 2, 2], 3, max_dist=np.nextafter(d[2], np.float32(0)))[:4] == (1, 1, 1, bits(0.1))
    assert one_asker(d, [N, 1, 2, 2], 3, max_dist=np.inf)[:4] == (2, 2, 3, bits(0.2))
    # -0 stands before +0 whatever the ids, and a window of -0 ends between them
    assert one_asker([0, 0.0, -0.0], [N, 1, 2], 1)[:4] == (2, 1, 1, bits(-0.0))
    assert one_asker([0, 0.0, -0.0], [N, 1, 2], 2, max_dist=np.float32(-0.0))[:4] == (2, 1, 1, bits(-0.0))
    assert one_asker([0, 0.0, -0.0], [N, 1, 2], 2, max_dist=np.float32(0.0))[:4] == (2, 1, 2, bits(-0.0))
    # no voters: nobody holds a group / the only grouped row is deleted / the predicate keeps none
    assert one_asker([0, 0.1, 0.2], [N, N, N], 2) == (N, 0, 0, bits(np.inf), {"askers": 3, "proposed": 0, "voters": 0, "unanimous": 0})
    assert one_asker([0, 0.1, 0.2], [N, 1, N], 2, live=[1, 0, 1])[4]["voters"] == 0
    assert one_asker([0, 0.1, 0.2], [N, 1, 1], 2, voters=np.zeros(3, bool))[:3] == (N, 0, 0)
    # an asker without a voter in reach
    g, v, h, db, tot = one_asker([0, 0.6, 0.7], [N, 1, 2], 2, max_dist=0.5)
    assert (g, v, h, db) == (N, 0, 0, bits(np.inf)) and tot == {"askers": 1, "proposed": 0, "voters": 2, "unanimous": 0}
    # asking for a group: its rows ask, the rows without a group neither ask nor vote, the others vote
    g, v, h, db, tot = one_asker([0, 0.1, 0.2, 0.3], [5, N, 5, 6], 3, ask_group=5)
    assert (g, v, h, db) == (6, 1, 1, bits(0.3)) and tot["askers"] == 2 and tot["voters"] == 1
    # a deleted row never asks
    assert one_asker([0, 0.1], [N, 1], 1, live=[0, 1])[4]["askers"] == 0


# ---- stage 1 under a column mask ---------------------------------------------------------------------------------------------
def emitted_masked(coarse, keep, m, segments, stride):
    """search_many_tiles_kernel with the mask in place of the deletion bitmap: a masked column has weight 0 — it stays out of
    the slots (its coarse value is never offered) and is never emitted"""
    offered = np.where(keep[None, :], coarse, -np.inf)
    t = thresholds(offered, m, segments, stride)
    return (coarse >= (t - 2.0 * EPS2)[:, None]) & keep[None, :], t


@pytest.fixture(scope="module")
def hard():
    rows, vec = hard_corpus(17)
    return cosines(rows, vec)


@pytest.mark.parametrize("m", [1, 3, 16])
def test_masked_two_pass_rule_keeps_the_exact_masked_top_m(hard, m):
    coarse, exact = hard
    C = coarse.shape[1]
    rng = np.random.default_rng(5)
    masks = {"a third": rng.random(C) < 0.33, "all": np.ones(C, bool), "c % 16 == 0": np.arange(C) % 16 == 0,
             "fewer than m": np.isin(np.arange(C), rng.permutation(C)[:max(m - 1, 1)]), "none": np.zeros(C, bool)}
    for name, keep in masks.items():
        n_keep = int(keep.sum())
        masked = np.where(keep[None, :], exact, -np.inf)
        top = keep[None, :] & (masked >= np.sort(masked, axis=1)[:, -min(m, n_keep)][:, None]) if n_keep else np.zeros_like(masked, bool)
        for segments in (1, 2, 5):
            for stride in (1, 2, 8):
                got, t = emitted_masked(coarse, keep, m, segments, stride)
                assert np.all(got[top]), (name, m, segments, stride)
                assert not np.any(got[:, ~keep]), name
        got, t = emitted_masked(coarse, keep, m, 1, 1)
        print(f"m {m}, mask '{name}' ({n_keep} columns): emitted {got[:, keep].mean() if n_keep else 0.0:.3f} of the unmasked pairs")
        if name == "c % 16 == 0" and m == 16:
            # the known cost: the unmasked columns fill ONE residue slot, the other 15 stay empty, no threshold forms
            assert np.all(np.isneginf(t)) and np.all(got[:, keep])
        if name == "c % 16 == 0" and m == 1:
            assert got[32:, keep].mean() < 0.9   # one slot: the rule does filter
        if name == "a third" and m < 16:
            assert got[32:, keep].mean() < 0.9
