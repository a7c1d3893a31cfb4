"""Density and DBSCAN at several distances in one pass, on the GPU (mi_knn_density_levels, mi_knn_dbscan_levels,
mi_dbscan_levels_tree, ImageIndex.theme_tree): every slice equals the single call at that distance (check_same), the
restatement of tests/test_density_levels_host.py fed by the CPU oracle's pairs, and the same fed by the device's own
near_pairs at the largest distance, thresholded per level.  The corpus is tests/test_density_gpu.py's: 1 500 x 768, 11 full
tiles and one of 92."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd._lib import MiError
from image_search_amd.search import EmbeddingTable, ImageIndex, dbscan_levels_tree, pairs_to_groups
from test_density_gpu import (A0, B0, BRIDGE0, DIM, MAX_DISTS, MIN_PTS, N, N_BRIDGE, blob, distance_matrix, oracle_pairs,
                              planted_corpus)
from test_density_host import check_same
from test_density_levels_host import expected_dbscan_levels
from test_page_host import NO_ID, bits

pytestmark = pytest.mark.gpu

KEYS = ("labels", "cluster", "via", "via_dist", "counts")


def level_slice(got, l):
    """level l of dbscan_levels' dict in dbscan's shape"""
    out = {k: got[k][l] for k in KEYS}
    out["summary"] = got["summary"][l]
    return out


def tree_edges(got, min_pts):
    level, child, parent = dbscan_levels_tree(got["cluster"], got["counts"], min_pts)
    return list(zip(level.tolist(), child.tolist(), parent.tolist()))


def check_levels(got, want, min_pts, what=""):
    """got: dbscan_levels' dict; want: expected_dbscan_levels' (levels, tree)"""
    levels, tree = want
    assert got["cluster"].shape[0] == len(levels), what
    for l, lv in enumerate(levels):
        check_same(level_slice(got, l), lv, f"{what} level {l}")
    assert tree_edges(got, min_pts) == tree, what
    # the dict's tree is the same edges over the dense labels
    for l in range(len(levels) - 1):
        names, up = np.unique(levels[l][0][levels[l][0] != NO_ID]), np.unique(levels[l + 1][0][levels[l + 1][0] != NO_ID])
        mine = [(l, int(names[c]), int(up[p])) for c, p in enumerate(got["tree"][l])]
        assert mine == [e for e in tree if e[0] == l], what
    assert got["dense_labels"] is got["labels"] or np.array_equal(got["dense_labels"], got["labels"])


@pytest.fixture(scope="module")
def corpus(built, orc):
    rows = planted_corpus()
    D = distance_matrix(orc, rows)
    top = oracle_pairs(D, MAX_DISTS[-1])
    want = {mp: expected_dbscan_levels(N, *top, MAX_DISTS, mp) for mp in MIN_PTS}
    # the structure is there before anything runs on the device: >= 2 clusters, a border row and noise at two levels
    for l in (1, 2):
        s = want[5][0][l][4]
        assert s[0] >= 2 and s[2] >= 1 and s[3] >= 1, (l, s)
    assert want[2][0][0][4][0] >= 2 and len(want[5][1]) >= 3 and len(want[2][1]) >= 4
    # the levels differ: a pair that is in W at 0.2 and not at 0.1, one at 0.1 and not at 0.02
    assert (top[2] > np.float32(0.1)).any() and ((top[2] > np.float32(0.02)) & (top[2] <= np.float32(0.1))).any()
    # the bridge fuses A and B at min_pts 2 from 0.1 on, and not at 0.02
    c = [lv[0] for lv in want[2][0]]
    assert c[0][A0] != c[0][B0] and c[1][A0] == c[1][B0] and c[2][A0] == c[2][B0]
    return rows, D, want


@pytest.fixture(scope="module")
def table(corpus):
    t = EmbeddingTable(DIM, 0)
    t.insert(corpus[0])
    yield t
    t.close()


# 1
@pytest.mark.parametrize("min_pts", MIN_PTS)
def test_every_slice_equals_the_single_call_and_the_restatement(corpus, table, min_pts):
    rows, D, want = corpus
    got = table.dbscan_levels(MAX_DISTS, min_pts)
    st = table.dbscan_stats()
    print(min_pts, got["summary"], st)
    check_levels(got, want[min_pts], min_pts, f"oracle {min_pts}")
    pairs = table.near_pairs(MAX_DISTS[-1])
    check_levels(got, expected_dbscan_levels(N, *pairs, MAX_DISTS, min_pts), min_pts, f"near_pairs {min_pts}")
    for l, md in enumerate(MAX_DISTS):
        single = table.dbscan(md, min_pts)
        mine = level_slice(got, l)
        check_same(mine, (single["cluster"], single["via"], single["via_dist"], single["counts"],
                          [single["summary"][k] for k in ("clusters", "core", "border", "noise")]), f"dbscan {md} {min_pts}")
    assert st["pairs"] == pairs[0].size and st["tiles_pass1"] == 12 * 13 // 2
    assert st["tiles_visited"] + st["tiles_skipped"] == 12 * 13 // 2
    assert st["unions_merged"] == sum(s["core"] - s["clusters"] for s in got["summary"])
    if min_pts == 50:
        assert all(s == {"clusters": 0, "core": 0, "border": 0, "noise": N} for s in got["summary"])


def test_neighbor_counts_levels_equal_neighbor_counts(corpus, table):
    rows, D, want = corpus
    counts = table.neighbor_counts_levels(MAX_DISTS)
    assert counts.shape == (3, N) and counts.dtype == np.uint32
    for l, md in enumerate(MAX_DISTS):
        assert np.array_equal(counts[l], table.neighbor_counts(md)), md
        assert np.array_equal(counts[l], want[1][0][l][3]), md
    assert table.dbscan_stats()["pairs"] == int(counts[2].sum()) // 2


# 2
def test_one_level_eight_levels_and_a_level_on_a_pairs_own_bits(corpus, table):
    rows, D, want = corpus
    one = table.dbscan_levels([0.1], 5)
    single = table.dbscan(0.1, 5)
    assert one["cluster"].shape == (1, N) and one["tree"] == []
    check_same(level_slice(one, 0), want[5][0][1], "one level")
    assert all(np.array_equal(bits(one[k][0]) if k == "via_dist" else one[k][0], bits(single[k]) if k == "via_dist" else single[k])
               for k in KEYS) and one["summary"][0] == single["summary"]
    eight = (0.01, 0.02, 0.05, 0.08, 0.1, 0.15, 0.2, 0.25)
    got = table.dbscan_levels(eight, 5)
    check_levels(got, expected_dbscan_levels(N, *oracle_pairs(D, eight[-1]), eight, 5), 5, "eight levels")
    assert np.array_equal(table.neighbor_counts_levels(eight)[4], want[1][0][1][3])
    # a level set to exactly D[a, b] with the float below it as the level before: the pair counts at the upper level only
    a, b = A0, A0 + 1
    d_ab = D[a, b]
    assert np.float32(0.02) < d_ab < np.float32(0.1)
    below = np.nextafter(d_ab, np.float32(0.0))
    levels = (below, d_ab)
    counts = table.neighbor_counts_levels(levels)
    ties = int(np.count_nonzero(np.triu(D == d_ab, 1)))       # the pairs with exactly these bits: (a, b) and any tie
    assert ties >= 1 and int(counts[1].sum()) - int(counts[0].sum()) == 2 * ties
    lo_a, lo_b = oracle_pairs(D, below)[:2]
    assert not np.any((lo_a == a) & (lo_b == b))
    assert counts[1][a] >= counts[0][a] + 1 and counts[1][b] >= counts[0][b] + 1
    assert np.array_equal(counts[0], table.neighbor_counts(below)) and np.array_equal(counts[1], table.neighbor_counts(d_ab))
    check_levels(table.dbscan_levels(levels, 2), expected_dbscan_levels(N, *oracle_pairs(D, d_ab), levels, 2), 2, "on the bits")


# 3
def test_overflow_halvings_count_every_pair_once_at_every_level(built):
    rng = np.random.default_rng(6)
    row = rng.standard_normal(DIM).astype(np.float32)
    t = EmbeddingTable(DIM, 0)
    t.insert(np.tile(row, (300, 1)))
    t.set_option("join_cap", 16384)                    # 44 850 pairs: the strip does not fit
    levels = (0.0005, 0.001, 0.01)
    pairs = t.near_pairs(levels[-1], cap=1 << 16)
    assert pairs[0].size == 44850
    want = expected_dbscan_levels(300, *pairs, levels, 5)
    counts = t.neighbor_counts_levels(levels)
    assert t.dbscan_stats()["launches"] > 1
    for l in range(3):
        assert np.array_equal(counts[l], want[0][l][3]), l
    assert np.array_equal(counts[2], np.full(300, 299, np.uint32))
    got = t.dbscan_levels(levels, 5)
    st = t.dbscan_stats()
    print("300 copies:", st, got["summary"])
    check_levels(got, want, 5, "300 copies")
    assert got["summary"][2] == {"clusters": 1, "core": 300, "border": 0, "noise": 0} and np.all(got["cluster"][2] == 0)
    assert st["pairs"] == 44850 and st["unions_merged"] == sum(s["core"] - s["clusters"] for s in got["summary"])
    assert st["tiles_pass1"] == 6 and st["tiles_visited"] == 6 and st["tiles_skipped"] == 0
    t.close()


# 4
def test_stats_the_tiles_of_blocks_without_planted_rows_are_skipped(corpus, table):
    rows, D, want = corpus
    got = table.dbscan_levels(MAX_DISTS, 5)
    st = table.dbscan_stats()
    check_levels(got, want[5], 5, "skipping")
    # neighbours exist in blocks 0, 1 and 5 only: at most the 6 tiles among them are visited
    assert st["tiles_skipped"] > 0 and st["tiles_visited"] + st["tiles_skipped"] == 78 and 1 <= st["tiles_visited"] <= 6
    assert st["candidates_pass2"] <= st["candidates_pass1"]


# 5
def test_the_tree_and_the_components_at_min_pts_two(corpus, table):
    rows, D, want = corpus
    for min_pts in (2, 5):
        got = table.dbscan_levels(MAX_DISTS, min_pts)
        assert tree_edges(got, min_pts) == want[min_pts][1]
    got = table.dbscan_levels(MAX_DISTS, 2)
    # at min_pts 2 a row is a core as soon as it has a neighbour: every level's clusters are the join's connected components
    for l, md in enumerate(MAX_DISTS):
        pairs = table.near_pairs(md)
        groups = pairs_to_groups(pairs[0], pairs[1])
        cl = got["cluster"][l]
        mine = [np.flatnonzero(cl == c).astype(np.uint64) for c in np.unique(cl[cl != NO_ID])]
        assert len(mine) == len(groups) and all(np.array_equal(x, y) for x, y in zip(mine, groups)), md
    # a child's rows lie inside its parent's (at min_pts 2 there are no border rows)
    for l, c, p in tree_edges(got, 2):
        assert np.all(got["cluster"][l + 1][got["cluster"][l] == c] == p)


# 6
def test_deletions_that_split_a_cluster_at_the_lower_level_only(corpus):
    rows, D, want = corpus
    levels = (0.1, 0.3)
    mid = BRIDGE0 + N_BRIDGE // 2
    live = np.ones(N, bool)
    live[mid] = False
    before = expected_dbscan_levels(N, *oracle_pairs(D, levels[-1]), levels, 3)
    after = expected_dbscan_levels(N, *oracle_pairs(D, levels[-1], live), levels, 3, live=live)
    assert before[0][0][0][A0] == before[0][0][0][B0]                          # the bridge's middle holds A and B together at 0.1
    assert after[0][0][0][A0] != after[0][0][0][B0] and after[0][1][0][A0] == after[0][1][0][B0]   # ... without it only 0.3 does
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    check_levels(t.dbscan_levels(levels, 3), before, 3, "before")
    assert t.delete([mid]) == 1
    got = t.dbscan_levels(levels, 3)
    check_levels(got, after, 3, "after")
    for l in range(2):
        assert got["cluster"][l][mid] == NO_ID and got["via"][l][mid] == NO_ID and np.isposinf(got["via_dist"][l][mid])
        assert got["counts"][l][mid] == 0
    assert np.array_equal(t.neighbor_counts_levels(levels), np.stack([lv[3] for lv in after[0]]))
    t.close()


def test_ids_above_32_bits(corpus):
    rows, D, want = corpus
    base = 2 ** 40
    t = EmbeddingTable(DIM, 0)
    t.set_base(base)
    t.insert(rows)
    ids = np.arange(N, dtype=np.uint64) + np.uint64(base)
    got = t.dbscan_levels(MAX_DISTS, 5)
    check_levels(got, expected_dbscan_levels(N, *oracle_pairs(D, MAX_DISTS[-1]), MAX_DISTS, 5, ids=ids), 5, "base 2^40")
    assert got["cluster"][1][A0] >= base and all(c >= base and p >= base for _, c, p in tree_edges(got, 5))
    t.close()


def test_tiny_tables(built):
    t = EmbeddingTable(DIM, 0)
    levels = (0.001, 0.1)
    assert t.neighbor_counts_levels(levels).shape == (2, 0)
    got = t.dbscan_levels(levels, 1)
    assert got["cluster"].shape == (2, 0) and got["labels"].shape == (2, 0) and got["tree"][0].size == 0
    assert got["summary"] == [{"clusters": 0, "core": 0, "border": 0, "noise": 0}] * 2
    row = np.random.default_rng(2).standard_normal((1, DIM)).astype(np.float32)
    t.insert(row)
    assert t.neighbor_counts_levels(levels).tolist() == [[0], [0]]
    got = t.dbscan_levels(levels, 1)
    assert got["cluster"].tolist() == [[0], [0]] and got["via"].tolist() == [[0], [0]] and bits(got["via_dist"]).tolist() == [[0], [0]]
    assert got["summary"] == [{"clusters": 1, "core": 1, "border": 0, "noise": 0}] * 2 and got["tree"][0].tolist() == [0]
    got = t.dbscan_levels(levels, 2)
    assert got["cluster"].tolist() == [[int(NO_ID)]] * 2 and got["summary"] == [{"clusters": 0, "core": 0, "border": 0, "noise": 1}] * 2
    other = np.random.default_rng(3).standard_normal((1, DIM)).astype(np.float32)
    t.insert((row + np.float32(0.2) * other).astype(np.float32))                # about 0.02 away: a pair at the upper level only
    counts = t.neighbor_counts_levels(levels)
    assert counts.tolist() == [[0, 0], [1, 1]]
    got = t.dbscan_levels(levels, 2)
    assert got["cluster"].tolist() == [[int(NO_ID)] * 2, [0, 0]] and got["via"].tolist() == [[int(NO_ID)] * 2, [0, 1]]
    assert got["summary"] == [{"clusters": 0, "core": 0, "border": 0, "noise": 2}, {"clusters": 1, "core": 2, "border": 0, "noise": 0}]
    assert got["labels"].tolist() == [[-1, -1], [0, 0]] and got["tree"][0].size == 0
    got = t.dbscan_levels(levels, 1)
    assert got["cluster"].tolist() == [[0, 1], [0, 0]] and got["tree"][0].tolist() == [0, 0]
    t.close()


def same_bytes(x, y):
    return all(x[k].tobytes() == y[k].tobytes() for k in KEYS) and x["summary"] == y["summary"]


def test_two_calls_in_a_row_give_identical_bytes(table):
    first, second = table.dbscan_levels(MAX_DISTS, 5), table.dbscan_levels(MAX_DISTS, 5)
    assert same_bytes(first, second)
    assert table.neighbor_counts_levels(MAX_DISTS).tobytes() == table.neighbor_counts_levels(MAX_DISTS).tobytes()


def test_the_tables_own_mirror_and_one_built_for_the_call_agree(corpus):
    rows, D, want = corpus
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    for prefilter in (1, 2):
        t.set_option("prefilter", prefilter)
        for again in range(2):                          # (with 1: the table's mirror, built by the first call)
            check_levels(t.dbscan_levels(MAX_DISTS, 5), want[5], 5, f"prefilter {prefilter}")
            assert np.array_equal(t.neighbor_counts_levels(MAX_DISTS)[2], want[1][0][2][3])
    t.close()


def test_an_unsupported_dim_and_invalid_arguments_write_nothing(corpus):
    t = EmbeddingTable(192, 0)
    t.insert(np.random.default_rng(3).standard_normal((4, 192)).astype(np.float32))
    n = ctypes.c_uint64()
    code = _lib.lib().mi_knn_near_pairs(t._h, 0.1, 0, None, None, None, 0, ctypes.byref(n))
    assert code < 0
    cluster, via = np.full(8, 7, np.uint64), np.full(8, 7, np.uint64)
    via_dist, counts, summary = np.full(8, -7.0, np.float32), np.full(8, 7, np.uint32), np.full(8, 7, np.uint64)
    out = (cluster.ctypes.data, via.ctypes.data, via_dist.ctypes.data, counts.ctypes.data, summary.ctypes.data)
    d = np.array([0.1, 0.2], np.float32)
    assert _lib.lib().mi_knn_density_levels(t._h, d.ctypes.data, 2, counts.ctypes.data) == code
    assert _lib.lib().mi_knn_dbscan_levels(t._h, d.ctypes.data, 2, 5, *out) == code
    with pytest.raises(MiError):
        t.dbscan_levels([0.1, 0.2])
    t.close()
    # a real table, invalid arguments: the code, and the arrays as they were
    small = EmbeddingTable(DIM, 0)
    small.insert(corpus[0][A0:A0 + 4])
    for bad, n_levels, min_pts in (([0.2, 0.1], 2, 5), ([0.1, 0.1], 2, 5), ([0.1, np.nan], 2, 5), ([-0.1, 0.1], 2, 5), ([0.1, 0.2], 0, 5),
                                   ([0.1, 0.2], 2, 0), (list(np.arange(9) * 0.01), 9, 5)):
        d = np.array(bad, np.float32)
        assert _lib.lib().mi_knn_dbscan_levels(small._h, d.ctypes.data, n_levels, min_pts, *out) == -1, bad
        if min_pts:
            assert _lib.lib().mi_knn_density_levels(small._h, d.ctypes.data, n_levels, counts.ctypes.data) == -1, bad
    assert np.all(cluster == 7) and np.all(via == 7) and np.all(via_dist == -7.0) and np.all(counts == 7) and np.all(summary == 7)
    with pytest.raises(MiError):
        small.dbscan_levels([0.2, 0.1])
    with pytest.raises(MiError):
        small.neighbor_counts_levels([])
    assert small.dbscan_levels([0.1, 0.2], 2)["summary"][1]["core"] == 4          # and the table is as good as before
    small.close()


# 7
def test_index_theme_tree(built, tmp_path):
    rng = np.random.default_rng(12)
    media = str(tmp_path / "media") + "/"   # (rows store media_dir + <rel>)
    names = [f"{media}{folder}/{i}.jpg" for folder in ("a", "b", "c") for i in range(40)]
    emb = rng.standard_normal((120, DIM)).astype(np.float32)
    ca, cb = rng.standard_normal(DIM), rng.standard_normal(DIM)
    # one loose theme (0.1) that holds two bursts (0.01) and three looser rows; one burst on its own
    burst1, burst2, loose, alone = list(range(10, 16)), list(range(20, 25)), [30, 31, 32], list(range(50, 58))
    theme = burst1 + burst2 + loose
    c1, c2 = ca + 0.2 * rng.standard_normal(DIM), ca + 0.2 * rng.standard_normal(DIM)
    emb[burst1] = blob(rng, c1, 0.05, len(burst1), 1.0)
    emb[burst2] = blob(rng, c2, 0.05, len(burst2), 3.0)
    emb[loose] = blob(rng, ca, 0.2, len(loose), 1.0)
    emb[alone] = blob(rng, cb, 0.05, len(alone), 5.0)
    ix = ImageIndex(DIM, 0, media)
    ix.insert(names, emb)
    levels = (0.01, 0.1)
    res = ix.table.dbscan_levels(levels, 4)
    assert [s["clusters"] for s in res["summary"]] == [3, 2], res["summary"]     # the structure the test is about is there

    def check(themes, noise, gone):
        keep = lambda rows: [names[r] for r in rows if names[r] not in gone]
        assert [t["paths"] for t in themes] == [keep(theme), keep(alone)]             # the largest first
        assert [t["level"] for t in themes] == [1, 1] and themes[0]["max_dist"] == pytest.approx(0.1)
        assert [c["paths"] for c in themes[0]["children"]] == [keep(burst1), keep(burst2)]
        assert [c["paths"] for c in themes[1]["children"]] == [keep(alone)]
        assert all(c["level"] == 0 and c["children"] == [] for t in themes for c in t["children"])
        assert sorted(noise) == sorted(names[r] for r in range(120) if r not in theme + alone and names[r] not in gone)
        assert not gone & set(noise)

    themes, noise = ix.theme_tree(levels, min_pts=4)
    check(themes, noise, set())
    assert ix.theme_tree(levels, min_pts=4, web=True)[0][0]["paths"][0] == "media/a/10.jpg"
    gone = {names[12], names[52], names[100]}
    ix.remove(sorted(gone))
    themes, noise = ix.theme_tree(levels, min_pts=4)
    check(themes, noise, gone)
    assert len(noise) == 120 - len(theme) - len(alone) - 1
    # one level: themes' clusters, no children
    flat, flat_noise = ix.theme_tree([0.1], min_pts=4)
    plain, plain_noise = ix.themes(0.1, min_pts=4)
    assert [t["paths"] for t in flat] == plain and flat_noise == plain_noise and all(t["children"] == [] for t in flat)
    ix.close()
