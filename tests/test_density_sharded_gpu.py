"""Density and DBSCAN over a sharded table on the GPU (mi_knn_sharded_density, mi_knn_sharded_dbscan): ids, distance bits,
counts and summary equal (i) the restatement of tests/test_density_host.py (expected_dbscan) over the CPU oracle's pairs with
global rows and (ii) what one EmbeddingTable holding the same rows returns — for every shard count, block size and staging.
Every shard lives on device 0: a staged column side ("join_stage") takes there the path a shard on another device takes."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd._lib import MiError
from image_search_amd.search import EmbeddingTable, ShardedTable
from oracle.binding import orc_cosine_dist
from test_density_gpu import (A0, B0, BRIDGE0, COPY_A, COPY_B, DIM, MAX_DISTS, MIN_PTS, N, N_BRIDGE, RIM, distance_matrix, oracle_pairs,
                              planted_corpus)
from test_density_host import check_same, expected_dbscan
from test_join_between_gpu import planted_corpus as join_corpus
from test_join_between_gpu import sharded_of
from test_page_host import NO_ID, bits

pytestmark = pytest.mark.gpu

LAYOUTS = ((3, 64), (2, 128), (4, 64), (2, 960))          # (shards, block rows)
STAGINGS = ({"join_stage": 1}, {"join_stage": 1, "join_stage_rows": 256}, {"join_stage_rows": 256})


def shard_of(rows, shards, block):
    return (np.asarray(rows) // block) % shards


def crossings(want, pairs, shards, block, min_pts):
    """from the oracle's pairs and the layout alone: (core-core pairs that cross shards, border rows whose via lies in another
    shard, clusters with cores on more than one shard)"""
    cluster, via, _, deg, _ = want
    a, b, _ = pairs
    core = deg.astype(np.int64) + 1 >= min_pts
    n_cc = int((core[a] & core[b] & (shard_of(a, shards, block) != shard_of(b, shards, block))).sum())
    rows = np.arange(N, dtype=np.uint64)
    border = np.flatnonzero((via != NO_ID) & (via != rows))
    n_via = int((shard_of(border, shards, block) != shard_of(via[border].astype(np.int64), shards, block)).sum())
    spread = 0
    for c in np.unique(cluster[core]):
        spread += int(np.unique(shard_of(np.flatnonzero(core & (cluster == c)), shards, block)).size > 1)
    return n_cc, n_via, spread


@pytest.fixture(scope="module")
def corpus(built, orc):
    rows = planted_corpus()
    D = distance_matrix(orc, rows)
    pairs = {md: oracle_pairs(D, md) for md in MAX_DISTS}
    want = {(md, mp): expected_dbscan(N, *pairs[md], mp) for md in MAX_DISTS for mp in MIN_PTS}
    # before anything runs on the device: the layouts put the hard cases across shards.  3 x 64, from the corpus constants:
    # blob A lies on shards 1 and 2, COPY_A on shard 1, COPY_B and RIM on shard 2 — the equal-bits tie of RIM's via is between a
    # core in its own shard and one in another, and the other shard's smaller row wins
    assert shard_of([A0, A0 + 27, A0 + 28, A0 + 39], 3, 64).tolist() == [1, 1, 2, 2]
    assert shard_of([COPY_A, COPY_B, RIM], 3, 64).tolist() == [1, 2, 2]
    assert want[(0.1, 5)][1][RIM] == COPY_A and bits(D[COPY_A, RIM]) == bits(D[COPY_B, RIM])
    assert shard_of([A0 + 27, A0 + 28], 2, 128).tolist() == [0, 1] and shard_of([A0 + 27, A0 + 28], 4, 64).tolist() == [1, 2]
    assert shard_of([COPY_A, COPY_B, RIM], 4, 64).tolist() == [2, 3, 3]
    for shards, block in ((3, 64), (4, 64)):
        n_cc, n_via, spread = crossings(want[(0.1, 5)], pairs[0.1], shards, block, 5)
        assert n_cc >= 1 and n_via >= 1 and spread >= 1, (shards, block, n_cc, n_via, spread)
    n_cc, _, spread = crossings(want[(0.1, 5)], pairs[0.1], 2, 128, 5)
    assert n_cc >= 1 and spread >= 1
    for key in ((0.1, 5), (0.2, 5)):
        s = want[key][4]
        assert s[0] >= 2 and s[2] >= 1 and s[3] >= 1, (key, s)
    return rows, D, pairs, want


@pytest.fixture(scope="module")
def single(corpus):
    """one table with every row: what a sharded table must equal"""
    t = EmbeddingTable(DIM, 0)
    t.insert(corpus[0])
    res = {(md, mp): t.dbscan(md, mp) for md in MAX_DISTS for mp in MIN_PTS}
    counts = {md: t.neighbor_counts(md) for md in MAX_DISTS}
    t.close()
    return res, counts


def same_result(x, y, what=""):
    for k in ("labels", "cluster", "via", "counts"):
        assert np.array_equal(x[k], y[k]), (what, k)
    assert np.array_equal(bits(x["via_dist"]), bits(y["via_dist"])), what
    assert x["summary"] == y["summary"], what


def check_everything(t, corpus, single, what):
    rows, D, pairs, want = corpus
    res, counts = single
    for max_dist in MAX_DISTS:
        got = t.neighbor_counts(max_dist)
        assert np.array_equal(got, want[(max_dist, 1)][3]) and np.array_equal(got, counts[max_dist]), (what, max_dist)
        assert t.dbscan_stats()["pairs"] == pairs[max_dist][0].size
        for min_pts in MIN_PTS:
            got = t.dbscan(max_dist, min_pts)
            st = t.dbscan_stats()
            print(what, max_dist, min_pts, got["summary"], st)
            check_same(got, want[(max_dist, min_pts)], f"{what}: oracle {max_dist} {min_pts}")
            same_result(got, res[(max_dist, min_pts)], f"{what}: one table {max_dist} {min_pts}")
            assert st["pairs"] == pairs[max_dist][0].size
            assert st["tiles_visited"] + st["tiles_skipped"] == st["tiles_pass1"]
            assert st["unions_merged"] >= got["summary"]["core"] - got["summary"]["clusters"]


# 1
@pytest.mark.parametrize("shards,block", LAYOUTS)
def test_the_planted_corpus_equals_the_oracle_and_the_one_table(corpus, single, shards, block):
    t = sharded_of(corpus[0], shards, block)
    check_everything(t, corpus, single, f"{shards} x {block}")
    t.close()


# 2
@pytest.mark.parametrize("options", STAGINGS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_staged_and_chunked_column_sides(corpus, single, options):
    t = sharded_of(corpus[0], 3, 64, **options)
    assert t.shard_rows(2) == 476          # chunks of 256: two, the second ragged
    check_everything(t, corpus, single, str(options))
    t.close()


# 3: S m (m + 1) / 2 + S (S - 1) / 2 m^2 = S m (S m + 1) / 2 when shards are whole tiles
def test_tile_identity(built):
    rows = join_corpus()
    one = EmbeddingTable(DIM, 0)
    one.insert(rows)
    want = one.dbscan(0.05, 2)
    n_pairs = one.near_pairs(0.05)[0].size
    assert want["summary"]["clusters"] >= 10 and n_pairs >= 300
    one.close()
    t = sharded_of(rows, 4, 1024)
    assert [t.shard_rows(s) for s in range(4)] == [1024] * 4
    got = t.dbscan(0.05, 2)
    st = t.dbscan_stats()
    print("4 x 1024:", st)
    same_result(got, want, "4 x 1024")
    assert st["tiles_pass1"] == 528 and st["tiles_visited"] + st["tiles_skipped"] == 528, st
    assert st["pairs"] == n_pairs == t.near_pairs(0.05)[0].size
    t.close()


# 4
def test_copies_across_shards_under_a_small_candidate_buffer(built):
    row = np.random.default_rng(6).standard_normal(DIM).astype(np.float32)
    rows = np.tile(row, (300, 1))
    # 300 rows fill at most one tile per shard when all three shards hold some (a tile's 16 384 candidates always fit): blocks
    # of 192 put 192 rows on shard 0 and 108 on shard 1, so that a self piece (18 336 pairs) and a shard pair (20 736) overflow
    t = sharded_of(rows, 3, 192)
    assert [t.shard_rows(s) for s in range(3)] == [192, 108, 0]
    first = t.dbscan(0.001, 5)
    launches_without = t.dbscan_stats()["launches"]
    t.set_option("join_cap", 16384)                    # 44 850 pairs in all
    assert np.array_equal(t.neighbor_counts(0.001), np.full(300, 299, np.uint32))
    got = t.dbscan(0.001, 5)
    st = t.dbscan_stats()
    print("300 copies:", st)
    assert np.array_equal(got["counts"], np.full(300, 299, np.uint32))
    assert got["summary"] == {"clusters": 1, "core": 300, "border": 0, "noise": 0} and np.all(got["cluster"] == 0)
    assert st["launches"] > launches_without and st["pairs"] == 44850 and st["unions_merged"] >= 299
    same_result(got, first, "with and without the cap")
    same_result(t.dbscan(0.001, 5), got, "a second call")
    t.close()


# 5
@pytest.mark.parametrize("options", ({}, {"join_stage": 1, "join_stage_rows": 256}), ids=("direct", "staged"))
def test_deletions(corpus, options):
    rows, D, pairs, want = corpus
    # (a) at min_pts 3 the bridge's middle is a core that holds A and B together: without it the cluster falls apart
    c, via, vd, deg, s = expected_dbscan(N, *pairs[0.1], 3)
    mid = BRIDGE0 + N_BRIDGE // 2
    assert c[mid] != NO_ID and via[mid] == mid and c[A0] == c[B0]
    # (b) at min_pts 5 RIM (shard 2) joined through COPY_A (shard 1): without COPY_A it joins through COPY_B, in its own shard
    assert want[(0.1, 5)][1][RIM] == COPY_A and shard_of(RIM, 3, 64) != shard_of(COPY_A, 3, 64)
    t = sharded_of(rows, 3, 64, **options)
    check_same(t.dbscan(0.1, 3), (c, via, vd, deg, s), "before")
    assert t.delete(np.array([mid, COPY_A], np.uint64)) == 2
    live = np.ones(N, bool)
    live[[mid, COPY_A]] = False
    gone_pairs = oracle_pairs(D, 0.1, live)
    after3 = expected_dbscan(N, *gone_pairs, 3, live=live)
    after5 = expected_dbscan(N, *gone_pairs, 5, live=live)
    assert after3[0][A0] != after3[0][B0] and after3[4][0] == s[0] + 1
    assert after5[1][RIM] == COPY_B
    got = t.dbscan(0.1, 3)
    check_same(got, after3, "after, min_pts 3")
    check_same(t.dbscan(0.1, 5), after5, "after, min_pts 5")
    for r in (mid, COPY_A):
        assert got["cluster"][r] == NO_ID and got["via"][r] == NO_ID and np.isposinf(got["via_dist"][r]) and got["counts"][r] == 0
    assert np.array_equal(t.neighbor_counts(0.1), after3[3])
    t.close()



# 6
def test_tiny_tables_and_empty_shards(built):
    t = ShardedTable(DIM, [0, 0, 0], 64)
    assert t.neighbor_counts(0.1).size == 0
    got = t.dbscan(0.1, 1)
    assert got["cluster"].size == 0 and got["summary"] == {"clusters": 0, "core": 0, "border": 0, "noise": 0}
    rng = np.random.default_rng(2)
    row = rng.standard_normal((1, DIM)).astype(np.float32)
    t.insert(row)
    assert t.neighbor_counts(0.1).tolist() == [0]
    got = t.dbscan(0.1, 1)
    assert got["cluster"].tolist() == [0] and got["via"].tolist() == [0] and bits(got["via_dist"]).tolist() == [0]
    assert got["summary"] == {"clusters": 1, "core": 1, "border": 0, "noise": 0} and got["labels"].tolist() == [0]
    got = t.dbscan(0.1, 2)
    assert got["cluster"].tolist() == [int(NO_ID)] and got["summary"] == {"clusters": 0, "core": 0, "border": 0, "noise": 1}
    t.close()
    # 100 rows on 4 shards of blocks of 64: shards 2 and 3 hold nothing; a pair across shards 0 and 1, one inside shard 0
    rows = rng.standard_normal((100, DIM)).astype(np.float32)
    rows[90] = rows[10] * np.float32(0.5)
    rows[50] = rows[20]
    one = EmbeddingTable(DIM, 0)
    one.insert(rows)
    t = sharded_of(rows, 4, 64)
    assert [t.shard_rows(s) for s in range(4)] == [64, 36, 0, 0]
    for min_pts in (1, 2, 3):
        want = one.dbscan(0.01, min_pts)
        same_result(t.dbscan(0.01, min_pts), want, f"empty shards {min_pts}")
    assert want["counts"][[10, 90, 20, 50]].tolist() == [1, 1, 1, 1] and int(want["counts"].sum()) == 4
    assert one.dbscan(0.01, 2)["cluster"][[90, 50]].tolist() == [10, 20]
    assert np.array_equal(t.neighbor_counts(0.01), one.neighbor_counts(0.01))
    t.close(); one.close()


def test_zero_and_nan_rows_lie_in_other_shards_than_their_neighbours(built, orc):
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((300, DIM)).astype(np.float32)
    rows[200] = rows[10] = 0.0                                  # a zero row and its copy: NaN, never a pair
    rows[220] = rows[40]; rows[220, 7] = np.nan                 # a row and its copy with a NaN in it
    rows[260] = rows[100] * np.float32(2.0)                     # and an ordinary pair beside them
    for x, y in ((10, 200), (40, 220), (100, 260)):             # blocks of 64 on 2 shards: each pair straddles the shards
        assert shard_of(x, 2, 64) != shard_of(y, 2, 64)
    D = np.stack([orc_cosine_dist(orc, rows[a], rows) for a in range(300)])
    cases = ((0.01, 2), (1.5, 5), (1.5, 400))
    want = {c: expected_dbscan(300, *oracle_pairs(D, c[0]), c[1]) for c in cases}
    assert want[(1.5, 5)][3][[10, 200, 220]].tolist() == [0, 0, 0] and want[(1.5, 5)][3][40] >= 200
    for options in ({}, {"join_stage": 1}):
        t = sharded_of(rows, 2, 64, **options)
        for c in cases:
            got = t.dbscan(*c)
            check_same(got, want[c], (options, c))
            assert got["counts"][[10, 200, 220]].tolist() == [0, 0, 0] and got["cluster"][220] == NO_ID
        assert t.dbscan(0.01, 2)["cluster"][[100, 260]].tolist() == [100, 100]
        t.close()


def test_an_unsupported_dim_fails_as_the_join_does_and_writes_nothing(built):
    t = ShardedTable(192, [0, 0], 64)
    t.insert(np.random.default_rng(3).standard_normal((4, 192)).astype(np.float32))
    n = ctypes.c_uint64()
    code = _lib.lib().mi_knn_sharded_near_pairs(t._h, 0.1, 0, None, None, None, 0, ctypes.byref(n))
    assert code < 0
    cluster, via = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64)
    via_dist, counts, summary = np.full(4, -7.0, np.float32), np.full(4, 7, np.uint32), np.full(4, 7, np.uint64)
    assert _lib.lib().mi_knn_sharded_density(t._h, 0.1, counts.ctypes.data) == code
    assert _lib.lib().mi_knn_sharded_dbscan(t._h, 0.1, 5, cluster.ctypes.data, via.ctypes.data, via_dist.ctypes.data, counts.ctypes.data,
                                            summary.ctypes.data) == code
    assert np.all(cluster == 7) and np.all(via == 7) and np.all(via_dist == -7.0) and np.all(counts == 7) and np.all(summary == 7)
    with pytest.raises(MiError):
        t.dbscan(0.1)
    t.close()


# 7
def test_the_labels_fit_the_group_column_the_best_picture_of_each_theme(corpus, orc):
    rows, D, pairs, want = corpus
    t = sharded_of(rows, 3, 64)
    labels = t.dbscan(0.1, 5)["labels"]
    n_themes = int(labels.max()) + 1
    assert n_themes >= 2
    t.set_groups(labels.astype(np.uint32))
    q = np.random.default_rng(9).standard_normal(DIM).astype(np.float32)
    idx, dist, group, members, totals = t.knn_grouped(q, k=2048)      # every group's best row: the themes and the rows of their own
    d = orc_cosine_dist(orc, q, rows)
    for g in range(n_themes):
        mine = np.flatnonzero(labels == g)
        best = mine[np.lexsort((mine, d[mine]))[0]]                    # nearest, then the smaller id
        at = np.flatnonzero(group == g)
        assert at.size == 1 and idx[at[0]] == best and bits(dist[at[0]]) == bits(d[best]) and members[at[0]] == mine.size, g
    t.close()
