"""Density and DBSCAN on the GPU (mi_knn_density, mi_knn_dbscan, mi_index_themes): ids, distance bits, counts and summary
equal the restatement of tests/test_density_host.py (expected_dbscan), fed (i) by the CPU oracle's pairs — the matrix of
orc_cosine_dist with q = row a, thresholded, as tests/test_join_gpu.py builds it — and (ii) by the device's own
table.near_pairs."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd._lib import MiError
from image_search_amd.search import EmbeddingTable, ImageIndex, pairs_to_groups
from oracle.binding import orc_cosine_dist
from test_density_host import check_same, expected_dbscan
from test_page_host import NO_ID, bits

pytestmark = pytest.mark.gpu

DIM = 768
N = 1500                      # 11 full tiles and a ragged one of 92
MAX_DISTS = (0.02, 0.1, 0.2)
MIN_PTS = (1, 2, 5, 50)
# where the planted rows lie: blocks 0 and 1 (blob A straddles row 128) and block 5 — nothing else has a neighbour
A0, B0, C0, BRIDGE0, MINI0, COPY_A, COPY_B, RIM, SPUR, RIM2, ZERO_ROW, NAN_ROW = 100, 640, 660, 670, 680, 700, 720, 750, 755, 760, 1200, 1300
N_BRIDGE = 5


def blob(rng, centre, sigma, n, scale):
    return ((centre + sigma * rng.standard_normal((n, DIM))) * scale).astype(np.float32)


def planted_corpus(seed=11):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((N, DIM)).astype(np.float32)
    ca, cb, cc, v = (rng.standard_normal(DIM) for _ in range(4))
    rows[A0:A0 + 40] = blob(rng, ca, 0.25, 40, 0.1)          # member to member about 0.06: a theme at 0.1, not at 0.02
    rows[B0:B0 + 12] = blob(rng, cb, 0.12, 12, 10.0)         # about 0.014: a burst at 0.02
    rows[C0:C0 + 5] = blob(rng, cc, 0.40, 5, 1.0)            # about 0.14: only at 0.2
    for j in range(N_BRIDGE):                                # evenly spaced between the centres of A and B: steps of about 15 degrees
        t = (j + 1) / (N_BRIDGE + 1)
        rows[BRIDGE0 + j] = ((1 - t) * ca + t * cb).astype(np.float32)
    # one core at two ids, COPY_A < COPY_B, made cores by four rows about 0.056 away; beside them, all at larger rows so that
    # both pairs carry the same bits: a rim row at about 0.09 (0.14 from the four), a spur that only the rim row is near
    # (0.055; 0.14 from the copies), and a second rim row at about 0.18 (0.23 from the four)
    rows[MINI0:MINI0 + 4] = blob(rng, v, 0.35, 4, 1.0)
    rows[COPY_A] = rows[COPY_B] = v.astype(np.float32)
    n_rim = rng.standard_normal(DIM)
    rows[RIM] = ((v + 0.4556 * n_rim) * 3.0).astype(np.float32)
    rows[SPUR] = (v + 0.4556 * n_rim + 0.38 * rng.standard_normal(DIM)).astype(np.float32)
    rows[RIM2] = ((v + 0.76 * rng.standard_normal(DIM)) * 0.5).astype(np.float32)
    rows[ZERO_ROW] = 0.0
    rows[NAN_ROW, 17] = np.nan
    return rows


def distance_matrix(orc, rows):
    """D[a, b] = what the single pass with q = row a reports for row b"""
    return np.stack([orc_cosine_dist(orc, rows[a], rows) for a in range(rows.shape[0])])


def oracle_pairs(D, max_dist, live=None):
    n = D.shape[0]
    ok = np.triu(np.ones((n, n), bool), 1) & (D <= np.float32(max_dist))   # (a NaN compares false: never a pair)
    if live is not None:
        ok &= live[:, None] & live[None, :]
    a, b = np.nonzero(ok)
    return a, b, D[a, b]


@pytest.fixture(scope="module")
def corpus(built, orc):
    rows = planted_corpus()
    D = distance_matrix(orc, rows)
    want = {(md, mp): expected_dbscan(N, *oracle_pairs(D, md), mp) for md in MAX_DISTS for mp in MIN_PTS}
    # the structure is there before anything runs on the device: the tests below cannot pass on an empty one
    for key in ((0.1, 5), (0.2, 5), (0.1, 2)):
        s = want[key][4]
        assert s[0] >= 2 and s[3] >= 1, (key, s)
    assert want[(0.1, 5)][4][2] >= 1 and want[(0.2, 5)][4][2] >= 1          # border rows
    assert want[(0.02, 2)][4][0] >= 2
    c, via, vd, deg, _ = want[(0.1, 5)]
    # the tie of the two copies: equal distance bits, the smaller row wins — for the rim row at 0.1 and the second one at 0.2
    assert via[RIM] == COPY_A and D[COPY_A, RIM].view(np.uint32) == D[COPY_B, RIM].view(np.uint32) and deg[RIM] == 3
    assert want[(0.2, 5)][1][RIM2] == COPY_A and D[COPY_A, RIM2].view(np.uint32) == D[COPY_B, RIM2].view(np.uint32)
    assert c[SPUR] == NO_ID and deg[SPUR] == 1                                  # beside a border row only: noise
    assert deg[ZERO_ROW] == 0 and deg[NAN_ROW] == 0
    assert c[A0] != c[B0] and want[(0.1, 2)][0][A0] == want[(0.1, 2)][0][B0]   # the bridge joins A and B once its rows are cores
    return rows, D, want


@pytest.fixture(scope="module")
def table(corpus):
    t = EmbeddingTable(DIM, 0)
    t.insert(corpus[0])
    yield t
    t.close()


# 1
@pytest.mark.parametrize("max_dist", MAX_DISTS)
def test_density_and_dbscan_equal_the_restatement(corpus, table, max_dist):
    rows, D, want = corpus
    pairs = table.near_pairs(max_dist)
    counts = table.neighbor_counts(max_dist)
    assert np.array_equal(counts, want[(max_dist, 1)][3])
    for min_pts in MIN_PTS:
        got = table.dbscan(max_dist, min_pts)
        print(max_dist, min_pts, got["summary"], table.dbscan_stats())
        check_same(got, want[(max_dist, min_pts)], f"oracle {max_dist} {min_pts}")
        check_same(got, expected_dbscan(N, *pairs, min_pts), f"near_pairs {max_dist} {min_pts}")
        st = table.dbscan_stats()
        assert st["pairs"] == pairs[0].size and st["tiles_pass1"] == 12 * 13 // 2
        assert st["tiles_visited"] + st["tiles_skipped"] == 12 * 13 // 2
        assert st["unions_merged"] == got["summary"]["core"] - got["summary"]["clusters"]
    s = table.dbscan(max_dist, 50)["summary"]
    assert s == {"clusters": 0, "core": 0, "border": 0, "noise": N}
    # at min_pts 2 a row is a core as soon as it has a neighbour: the clusters are the join's connected components
    got = table.dbscan(max_dist, 2)
    groups = pairs_to_groups(pairs[0], pairs[1])
    mine = [np.flatnonzero(got["cluster"] == c).astype(np.uint64) for c in np.unique(got["cluster"][got["cluster"] != NO_ID])]
    assert len(mine) == len(groups) and all(np.array_equal(x, y) for x, y in zip(mine, groups))


# 2
def test_via_dist_carries_the_bits_of_the_search(corpus, table):
    rows, D, want = corpus
    got = table.dbscan(0.2, 5)
    border = np.flatnonzero((got["via"] != NO_ID) & (got["via"] != np.arange(N, dtype=np.uint64)))
    assert border.size >= 1
    pick = border if border.size <= 16 else np.random.default_rng(1).choice(border, 16, replace=False)
    for r in pick:
        c = int(got["via"][r])
        q, other = (c, r) if c < r else (r, c)         # the pair's distance is the one the smaller row's search reports
        idx, dist = table.knn(rows[q], 128)
        at = np.flatnonzero(idx == other)
        assert at.size == 1, (r, c)
        assert bits(dist[at[0]]) == bits(got["via_dist"][r])


# 3
def test_overflow_halving_counts_every_pair_once(built):
    row = np.random.default_rng(6).standard_normal(DIM).astype(np.float32)
    t = EmbeddingTable(DIM, 0)
    t.insert(np.tile(row, (300, 1)))
    t.set_option("join_cap", 16384)                    # 44 850 pairs: the strip does not fit
    assert np.array_equal(t.neighbor_counts(0.001), np.full(300, 299, np.uint32))
    launches_density = t.dbscan_stats()["launches"]
    assert launches_density > 1
    got = t.dbscan(0.001, 5)
    st = t.dbscan_stats()
    print("300 copies:", st)
    assert np.array_equal(got["counts"], np.full(300, 299, np.uint32))
    assert got["summary"] == {"clusters": 1, "core": 300, "border": 0, "noise": 0} and np.all(got["cluster"] == 0)
    assert st["launches"] == 2 * launches_density and st["pairs"] == 44850 and st["unions_merged"] == 299
    assert st["tiles_pass1"] == 6 and st["tiles_visited"] == 6 and st["tiles_skipped"] == 0
    t.close()


# 4
def test_tiles_without_a_core_or_a_neighbour_are_skipped(corpus, table):
    rows, D, want = corpus
    got = table.dbscan(0.1, 5)
    st = table.dbscan_stats()
    check_same(got, want[(0.1, 5)], "skipping")
    # neighbours exist in blocks 0, 1 and 5 only: at most the 6 tiles among them are visited
    assert st["tiles_skipped"] > 0 and st["tiles_visited"] + st["tiles_skipped"] == 78 and 1 <= st["tiles_visited"] <= 6
    assert st["candidates_pass2"] <= st["candidates_pass1"]


# 5
def test_deletions(corpus, orc):
    rows, D, want = corpus
    c, via, vd, deg, s = expected_dbscan(N, *oracle_pairs(D, 0.1), 3)
    mid = BRIDGE0 + N_BRIDGE // 2
    rows_idx = np.arange(N, dtype=np.uint64)
    is_border = (via != NO_ID) & (via != rows_idx)
    assert c[mid] != NO_ID and via[mid] == mid and c[A0] == c[B0]            # the bridge's middle is a core that holds A and B together
    assert is_border.any() and (c == NO_ID).any()
    border, noise = int(np.flatnonzero(is_border)[0]), int(np.flatnonzero(c == NO_ID)[0])
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    check_same(t.dbscan(0.1, 3), (c, via, vd, deg, s), "before")
    assert t.delete([mid, border, noise]) == 3
    live = np.ones(N, bool)
    live[[mid, border, noise]] = False
    after = expected_dbscan(N, *oracle_pairs(D, 0.1, live), 3, live=live)
    assert after[0][A0] != after[0][B0] and after[4][0] == s[0] + 1          # the cluster fell apart
    got = t.dbscan(0.1, 3)
    check_same(got, after, "after")
    for r in (mid, border, noise):
        assert got["cluster"][r] == NO_ID and got["via"][r] == NO_ID and np.isposinf(got["via_dist"][r]) and got["counts"][r] == 0
    assert np.array_equal(t.neighbor_counts(0.1), after[3])
    t.close()


# 6
def test_ids_above_32_bits(corpus):
    rows, D, want = corpus
    base = 2 ** 40
    t = EmbeddingTable(DIM, 0)
    t.set_base(base)
    t.insert(rows)
    ids = np.arange(N, dtype=np.uint64) + np.uint64(base)
    check_same(t.dbscan(0.1, 5), expected_dbscan(N, *oracle_pairs(D, 0.1), 5, ids=ids), "base 2^40")
    assert t.dbscan(0.1, 5)["cluster"][A0] >= base
    t.close()


# 7
def test_tiny_tables(built):
    t = EmbeddingTable(DIM, 0)
    assert t.neighbor_counts(0.1).size == 0
    got = t.dbscan(0.1, 1)
    assert got["cluster"].size == 0 and got["summary"] == {"clusters": 0, "core": 0, "border": 0, "noise": 0}
    row = np.random.default_rng(2).standard_normal((1, DIM)).astype(np.float32)
    t.insert(row)
    assert t.neighbor_counts(0.1).tolist() == [0]
    got = t.dbscan(0.1, 1)
    assert got["cluster"].tolist() == [0] and got["via"].tolist() == [0] and bits(got["via_dist"]).tolist() == [0]
    assert got["summary"] == {"clusters": 1, "core": 1, "border": 0, "noise": 0} and got["labels"].tolist() == [0]
    got = t.dbscan(0.1, 2)
    assert got["cluster"].tolist() == [int(NO_ID)] and got["summary"] == {"clusters": 0, "core": 0, "border": 0, "noise": 1}
    t.insert(row * np.float32(2.0))
    assert t.neighbor_counts(0.001).tolist() == [1, 1]
    got = t.dbscan(0.001, 2)
    assert got["cluster"].tolist() == [0, 0] and got["via"].tolist() == [0, 1] and got["counts"].tolist() == [1, 1]
    assert got["summary"] == {"clusters": 1, "core": 2, "border": 0, "noise": 0}
    got = t.dbscan(0.001, 3)
    assert got["summary"] == {"clusters": 0, "core": 0, "border": 0, "noise": 2} and got["labels"].tolist() == [-1, -1]
    t.close()


def same_arrays(x, y):
    return (all(np.array_equal(x[k], y[k]) for k in ("labels", "cluster", "via", "counts"))
            and np.array_equal(bits(x["via_dist"]), bits(y["via_dist"])) and x["summary"] == y["summary"])


# 8
def test_two_calls_in_a_row_agree(table):
    first, second = table.dbscan(0.2, 5), table.dbscan(0.2, 5)
    assert same_arrays(first, second)
    assert np.array_equal(table.neighbor_counts(0.2), table.neighbor_counts(0.2))


# 9
def test_the_tables_own_mirror_and_one_built_for_the_call_agree(corpus):
    rows, D, want = corpus
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    for prefilter in (1, 2):
        t.set_option("prefilter", prefilter)
        for again in range(2):                          # (with 1: the table's mirror, built by the first call)
            check_same(t.dbscan(0.1, 5), want[(0.1, 5)], f"prefilter {prefilter}")
            assert np.array_equal(t.neighbor_counts(0.2), want[(0.2, 1)][3])
    t.close()


# 10
def test_an_unsupported_dim_fails_as_the_join_does_and_writes_nothing(built):
    t = EmbeddingTable(192, 0)
    t.insert(np.random.default_rng(3).standard_normal((4, 192)).astype(np.float32))
    n = ctypes.c_uint64()
    code = _lib.lib().mi_knn_near_pairs(t._h, 0.1, 0, None, None, None, 0, ctypes.byref(n))
    assert code < 0
    cluster, via = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64)
    via_dist, counts, summary = np.full(4, -7.0, np.float32), np.full(4, 7, np.uint32), np.full(4, 7, np.uint64)
    assert _lib.lib().mi_knn_density(t._h, 0.1, counts.ctypes.data) == code
    assert _lib.lib().mi_knn_dbscan(t._h, 0.1, 5, cluster.ctypes.data, via.ctypes.data, via_dist.ctypes.data, counts.ctypes.data,
                                    summary.ctypes.data) == code
    assert np.all(cluster == 7) and np.all(via == 7) and np.all(via_dist == -7.0) and np.all(counts == 7) and np.all(summary == 7)
    with pytest.raises(MiError):
        t.dbscan(0.1)
    t.close()


# 11
def test_index_themes(built, tmp_path):
    rng = np.random.default_rng(12)
    media = str(tmp_path / "media") + "/"   # (rows store media_dir + <rel>)
    names = [f"{media}{folder}/{i}.jpg" for folder in ("a", "b", "c") for i in range(40)]
    emb = rng.standard_normal((120, DIM)).astype(np.float32)
    ca, cb = rng.standard_normal(DIM), rng.standard_normal(DIM)
    small, large = list(range(10, 16)), list(range(50, 59))
    emb[small] = blob(rng, ca, 0.2, len(small), 1.0)
    emb[large] = blob(rng, cb, 0.2, len(large), 5.0)
    ix = ImageIndex(DIM, 0, media)
    ix.insert(names, emb)
    themes, noise = ix.themes(0.1, min_pts=4)
    assert themes == [[names[r] for r in large], [names[r] for r in small]]        # the largest first
    assert sorted(noise) == sorted(names[r] for r in range(120) if r not in small + large)
    assert ix.themes(0.1, min_pts=4, web=True)[0][1][0] == "media/a/10.jpg"
    ix.remove([names[52], names[11], names[100]])
    themes, noise = ix.themes(0.1, min_pts=4)
    gone = {names[52], names[11], names[100]}
    assert themes == [[names[r] for r in large if r != 52], [names[r] for r in small if r != 11]]
    assert not gone & set(noise) and len(noise) == 120 - 15 - 1
    # the labels fit the group column: the best picture of each theme
    got = ix.table.dbscan(0.1, 4)
    assert got["labels"][50] == 1 and got["labels"][10] == 0 and got["labels"][52] == -1 and got["labels"][0] == -1
    ix.table.set_groups(got["labels"].astype(np.uint32))
    idx, dist, group, members, totals = ix.table.knn_grouped(emb[55], k=3, max_dist=0.1)
    assert idx[0] == 55 and group[0] == 1 and members[0] == 8
    ix.close()
