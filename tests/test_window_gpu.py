"""The windowed pair calls on the GPU (mi_knn_near_pairs_window, mi_knn_density_window, mi_knn_dbscan_window,
mi_knn_window_stats, mi_index_bursts, mi_index_events): ids, distance bits, counts and summary equal the restatement of
tests/test_window_host.py — expected_dbscan or a filtered pair list over the CPU oracle's distance matrix (orc_cosine_dist
with q = row a, as tests/test_density_gpu.py builds it), the stamp test taken on Python integers."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd._lib import MiError
from image_search_amd.search import EmbeddingTable, ImageIndex, pairs_to_groups
from test_density_gpu import (A0, B0, COPY_A, COPY_B, DIM, MINI0, N, NAN_ROW, RIM, RIM2, SPUR, ZERO_ROW, blob, distance_matrix, oracle_pairs,
                              planted_corpus, same_arrays)
from test_density_host import check_same, expected_dbscan
from test_page_host import NO_ID, bits
from test_window_host import I64_MAX, I64_MIN, U64_MAX, stamp_within, window_pairs

pytestmark = pytest.mark.gpu

MAX_DISTS = (0.02, 0.1, 0.2)
MIN_PTS = (1, 2, 5)
WINDOW = 3600                                     # the planted value: an hour of seconds
WINDOWS = (0, WINDOW, U64_MAX)
TRIANGLE = 12 * 13 // 2                           # 1 500 rows: 11 full tiles and a ragged one
# planted on top of tests/test_density_gpu.py's corpus (blob A of 40 rows from 100 straddles row 128, the burst of 12 from 640,
# the two copies 700 / 720 with their rim row 750): three near pairs in block 7 and a clique in block 8, whose rows are all deleted
EDGE, NEXT, EXTREME, GONE0, DEAD_BLOCK = 900, 910, 920, 1030, 8
T_A1, T_A2, T_BURST, T_MINI, T_EDGE, T_NEXT = 1_560_000_000, 1_690_000_000, 1_600_000_000, 1_650_000_000, 1_700_000_000, 1_710_000_000


def window_corpus():
    rows = planted_corpus()
    rng = np.random.default_rng(23)
    for r0 in (EDGE, NEXT, EXTREME):
        rows[r0:r0 + 2] = blob(rng, rng.standard_normal(DIM), 0.05, 2, 1.0)        # about 0.0025 apart: a pair at every max_dist
    rows[GONE0:GONE0 + 6] = blob(rng, rng.standard_normal(DIM), 0.12, 6, 1.0)      # a clique nobody may see: its block is deleted
    stamps = 1_000_000_000 + 100_000 * np.arange(N, dtype=np.int64)               # the background: far apart, no neighbours anyway
    stamps[A0:A0 + 20] = T_A1 + np.arange(20)                                       # the blob: one look, two periods four years apart;
    stamps[A0 + 20:A0 + 40] = T_A2 + np.arange(20)                                  # the second period lies on both sides of row 128
    stamps[B0:B0 + 12] = T_BURST + np.arange(12)                                    # the burst: consecutive seconds
    # the copies' neighbourhood was all taken in one second, but for copy A: the rim rows' tie between the two copies (equal
    # distance bits, the smaller row wins) is decided by the window
    stamps[[*range(MINI0, MINI0 + 4), COPY_B, RIM, SPUR, RIM2]] = T_MINI
    stamps[COPY_A] = T_MINI + 10_000_000
    stamps[EDGE:EDGE + 2] = T_EDGE, T_EDGE + WINDOW                                 # exactly the window apart
    stamps[NEXT:NEXT + 2] = T_NEXT + WINDOW + 1, T_NEXT                             # one more
    stamps[EXTREME:EXTREME + 2] = I64_MIN, I64_MAX
    live = np.ones(N, bool)
    live[DEAD_BLOCK * 128:(DEAD_BLOCK + 1) * 128] = False
    return rows, stamps, live


def make_table(rows, stamps=None, live=None, base=0):
    t = EmbeddingTable(DIM, 0)
    if base:
        t.set_base(base)
    t.insert(rows)
    ids = np.arange(rows.shape[0], dtype=np.uint64) + np.uint64(base)
    if stamps is not None:
        t.set_attrs(ids, stamps=stamps)
    if live is not None and not live.all():
        assert t.delete(ids[~live]) == int((~live).sum())
    return t


def has_pair(p, x, y):
    return bool(np.any((p[0] == x) & (p[1] == y)))


def same_pairs(got, want, what=""):
    assert np.array_equal(got[0], np.asarray(want[0], np.uint64)) and np.array_equal(got[1], np.asarray(want[1], np.uint64)), what
    assert np.array_equal(bits(got[2]), bits(np.asarray(want[2], np.float32))), what


@pytest.fixture(scope="module")
def corpus(built, orc):
    rows, stamps, live = window_corpus()
    D = distance_matrix(orc, rows)
    W = {md: oracle_pairs(D, md, live) for md in MAX_DISTS}
    Wwin = {(md, w): window_pairs(*W[md], stamps, w) for md in MAX_DISTS for w in WINDOWS}
    want = {(md, w, mp): expected_dbscan(N, *Wwin[(md, w)], mp, live=live) for md in MAX_DISTS for w in WINDOWS for mp in MIN_PTS}
    # ---- asserted before the device runs ----
    plain = expected_dbscan(N, *W[0.1], 5, live=live)
    c, via = want[(0.1, WINDOW, 5)][:2]
    assert len(set(plain[0][A0:A0 + 40].tolist())) == 1 and plain[0][A0] != NO_ID          # the blob: one cluster ...
    assert len(set(c[A0:A0 + 20].tolist())) == 1 and len(set(c[A0 + 20:A0 + 40].tolist())) == 1   # ... two under the window
    assert NO_ID not in (c[A0], c[A0 + 20]) and c[A0] != c[A0 + 20]
    for md in MAX_DISTS:
        p = Wwin[(md, WINDOW)]
        assert has_pair(p, EDGE, EDGE + 1) and not has_pair(p, NEXT, NEXT + 1) and has_pair(W[md], NEXT, NEXT + 1)
        assert has_pair(W[md], EXTREME, EXTREME + 1) and has_pair(Wwin[(md, U64_MAX)], EXTREME, EXTREME + 1)
        assert not has_pair(p, EXTREME, EXTREME + 1) and not has_pair(Wwin[(md, 0)], EXTREME, EXTREME + 1)
        assert Wwin[(md, U64_MAX)][0].size == W[md][0].size
        assert not np.any((W[md][0] >= DEAD_BLOCK * 128) & (W[md][0] < (DEAD_BLOCK + 1) * 128))   # the deleted block is in no pair
    assert has_pair(oracle_pairs(D, 0.1), GONE0, GONE0 + 1)                                    # ... though its rows look alike
    assert Wwin[(0.2, 0)][0].size >= 4 and Wwin[(0.02, WINDOW)][0].size > Wwin[(0.02, 0)][0].size   # window 0 is not empty
    # the tie of the two copies: equal bits, so copy A wins without the window and copy B, alone within it, with it
    assert D[COPY_A, RIM].view(np.uint32) == D[COPY_B, RIM].view(np.uint32)
    assert plain[1][RIM] == COPY_A and via[RIM] == COPY_B and via[COPY_B] == COPY_B
    border = (via != NO_ID) & (via != np.arange(N, dtype=np.uint64))
    assert np.any(border & (via != plain[1]))
    assert want[(0.1, WINDOW, 1)][3][ZERO_ROW] == 0 and want[(0.1, WINDOW, 1)][3][NAN_ROW] == 0
    return rows, stamps, live, D, W, Wwin, want


@pytest.fixture(scope="module")
def table(corpus):
    rows, stamps, live = corpus[:3]
    t = make_table(rows, stamps, live)
    yield t
    t.close()


# 1
@pytest.mark.parametrize("max_dist", MAX_DISTS)
def test_the_windowed_calls_equal_the_restatement(corpus, table, max_dist):
    rows, stamps, live, D, W, Wwin, want = corpus
    plain_pairs = table.near_pairs(max_dist)
    same_pairs(plain_pairs, W[max_dist], "near_pairs itself")
    join_stats, candidates = table.near_pairs_stats(), table.near_pairs_stats()["candidates"]
    for window in WINDOWS:
        got = table.near_pairs_window(max_dist, window)
        st = table.window_stats()
        print(max_dist, window, "near_pairs_window", st)
        same_pairs(got, Wwin[(max_dist, window)], f"pairs {max_dist} {window}")
        assert st["pairs"] == got[0].size and st["candidates_pass1"] <= candidates
        assert st["tiles_pass1"] + st["tiles_skipped_pass1"] == TRIANGLE
        assert (st["candidates_pass2"], st["tiles_pass2"], st["tiles_skipped_pass2"]) == (0, 0, 0)
        counts = table.neighbor_counts_window(max_dist, window)
        st = table.window_stats()
        assert np.array_equal(counts, want[(max_dist, window, 1)][3])
        assert st["pairs"] == got[0].size and st["tiles_pass1"] + st["tiles_skipped_pass1"] == TRIANGLE
        assert (st["candidates_pass2"], st["tiles_pass2"], st["tiles_skipped_pass2"]) == (0, 0, 0)
        for min_pts in MIN_PTS:
            res = table.dbscan_window(max_dist, window, min_pts)
            st = table.window_stats()
            print(max_dist, window, min_pts, res["summary"], st)
            check_same(res, want[(max_dist, window, min_pts)], f"oracle {max_dist} {window} {min_pts}")
            check_same(res, expected_dbscan(N, *got, min_pts, live=live), f"own pairs {max_dist} {window} {min_pts}")
            assert st["pairs"] == got[0].size
            assert st["tiles_pass1"] + st["tiles_skipped_pass1"] == TRIANGLE
            assert st["tiles_pass2"] + st["tiles_skipped_pass2"] == TRIANGLE
            assert st["candidates_pass2"] <= st["candidates_pass1"]
    # the widest window restricts nothing: the unwindowed calls themselves
    same_pairs(table.near_pairs_window(max_dist, U64_MAX), plain_pairs, "U64_MAX")
    assert np.array_equal(table.neighbor_counts_window(max_dist, U64_MAX), table.neighbor_counts(max_dist))
    for min_pts in MIN_PTS:
        assert same_arrays(table.dbscan_window(max_dist, U64_MAX, min_pts), table.dbscan(max_dist, min_pts))
    # the windowed calls kept their words to themselves
    dbscan_stats = table.dbscan_stats()
    table.dbscan_window(max_dist, WINDOW, 5)
    table.near_pairs_window(max_dist, WINDOW)
    assert table.near_pairs_stats() == join_stats and table.dbscan_stats() == dbscan_stats


# 2
def test_the_extremes_of_int64_are_a_pair_only_at_the_widest_window(corpus, table):
    for window in (0, 1, 2, WINDOW, 2 ** 63 - 1, 2 ** 63, U64_MAX - 1):
        a, b, _ = table.near_pairs_window(0.02, window)
        assert not has_pair((a, b), EXTREME, EXTREME + 1), window
        assert table.neighbor_counts_window(0.02, window)[EXTREME] == 0, window
    a, b, _ = table.near_pairs_window(0.02, U64_MAX)
    assert has_pair((a, b), EXTREME, EXTREME + 1) and table.neighbor_counts_window(0.02, U64_MAX)[EXTREME] == 1
    # and the boundary: exactly the window apart is within, one more is not
    for window, edge, nxt in ((WINDOW - 1, False, False), (WINDOW, True, False), (WINDOW + 1, True, True)):
        a, b, _ = table.near_pairs_window(0.02, window)
        assert has_pair((a, b), EDGE, EDGE + 1) == edge and has_pair((a, b), NEXT, NEXT + 1) == nxt, window


# 3
def test_a_table_that_never_set_attrs_ignores_the_window(corpus):
    rows, stamps, live = corpus[:3]
    t = make_table(rows, None, live)
    for window in (0, WINDOW, U64_MAX):
        same_pairs(t.near_pairs_window(0.1, window), t.near_pairs(0.1), f"no attrs {window}")
        assert np.array_equal(t.neighbor_counts_window(0.1, window), t.neighbor_counts(0.1))
        assert same_arrays(t.dbscan_window(0.1, window, 5), t.dbscan(0.1, 5))
        st = t.window_stats()
        # every live block's range is 0 .. 0: only the deleted block's tiles are skipped by the ranges
        assert st["tiles_skipped_pass1"] == 12 and st["tiles_pass1"] == TRIANGLE - 12
    t.close()


# 4
@pytest.mark.parametrize("first_new", (A0 + 30, COPY_A + 1, N - 1, N))
def test_first_new(corpus, table, first_new):
    rows, stamps, live, D, W, Wwin, want = corpus
    for window in (WINDOW, U64_MAX):
        a, b, d = Wwin[(0.1, window)]
        keep = b >= first_new
        same_pairs(table.near_pairs_window(0.1, window, first_new=first_new), (a[keep], b[keep], d[keep]), f"first_new {first_new} {window}")
        st = table.window_stats()
        # the triangle the pass covers: the columns from first_new's block on (one past the last row: no pass at all)
        covered = 0 if first_new == N else sum(12 - max(first_new // 128, bi) for bi in range(12))
        assert st["tiles_pass1"] + st["tiles_skipped_pass1"] == covered


# 5
def test_ids_above_32_bits(corpus):
    rows, stamps, live, D, W, Wwin, want = corpus
    base = 2 ** 40
    t = make_table(rows, stamps, live, base=base)
    ids = np.arange(N, dtype=np.uint64) + np.uint64(base)
    check_same(t.dbscan_window(0.1, WINDOW, 5), expected_dbscan(N, *Wwin[(0.1, WINDOW)], 5, live=live, ids=ids), "base 2^40")
    a, b, d = Wwin[(0.1, WINDOW)]
    same_pairs(t.near_pairs_window(0.1, WINDOW), (a + base, b + base, d), "base 2^40")
    same_pairs(t.near_pairs_window(0.1, WINDOW, first_new=base + COPY_A + 1), (a[b > COPY_A] + base, b[b > COPY_A] + base, d[b > COPY_A]), "first_new")
    t.close()


# 6
def test_deletions(corpus):
    rows, stamps, live, D, W, Wwin, want = corpus
    t = make_table(rows, stamps, live)
    check_same(t.dbscan_window(0.1, WINDOW, 5), want[(0.1, WINDOW, 5)], "before")
    gone = [A0 + 25, COPY_B, B0 + 3, EDGE]            # a core of the blob's second period, the copy the rim rows joined through, ...
    assert t.delete(gone) == 4
    live2 = live.copy()
    live2[gone] = False
    pairs = window_pairs(*oracle_pairs(D, 0.1, live2), stamps, WINDOW)
    after = expected_dbscan(N, *pairs, 5, live=live2)
    assert after[1][RIM] == NO_ID and want[(0.1, WINDOW, 5)][1][RIM] == COPY_B        # copy A is outside the window: the rim row is noise now
    got = t.dbscan_window(0.1, WINDOW, 5)
    check_same(got, after, "after")
    for r in gone:
        assert got["cluster"][r] == NO_ID and got["via"][r] == NO_ID and np.isposinf(got["via_dist"][r]) and got["counts"][r] == 0
    assert np.array_equal(t.neighbor_counts_window(0.1, WINDOW), after[3])
    same_pairs(t.near_pairs_window(0.1, WINDOW), pairs, "pairs after")
    t.close()


# 7
def test_two_calls_in_a_row_agree(table):
    assert same_arrays(table.dbscan_window(0.2, WINDOW, 5), table.dbscan_window(0.2, WINDOW, 5))
    assert np.array_equal(table.neighbor_counts_window(0.2, WINDOW), table.neighbor_counts_window(0.2, WINDOW))
    x, y = table.near_pairs_window(0.2, WINDOW), table.near_pairs_window(0.2, WINDOW)
    same_pairs(x, y)


# 8
def test_the_tables_own_mirror_and_one_built_for_the_call_agree(corpus):
    rows, stamps, live, D, W, Wwin, want = corpus
    t = make_table(rows, stamps, live)
    for prefilter in (1, 2):
        t.set_option("prefilter", prefilter)
        for again in range(2):                          # (with 1: the table's mirror, built by the first call)
            check_same(t.dbscan_window(0.1, WINDOW, 5), want[(0.1, WINDOW, 5)], f"prefilter {prefilter}")
            assert np.array_equal(t.neighbor_counts_window(0.2, WINDOW), want[(0.2, WINDOW, 1)][3])
            same_pairs(t.near_pairs_window(0.02, WINDOW), Wwin[(0.02, WINDOW)], f"prefilter {prefilter}")
    t.close()


# 9
@pytest.mark.parametrize("deal", ("ascending", "shuffled"))
def test_the_same_stamps_dealt_in_row_order_and_shuffled(corpus, deal):
    """ascending with the row index only a band of tiles along the diagonal survives the stamp ranges, shuffled nearly every
    tile does: the skip changes what is computed, never what comes out"""
    rows, stamps, live, D, W, Wwin, want = corpus
    # the planted stamps but for the two extremes (their tile would span everything), spread so that a block covers about a day
    values = np.sort(np.where(np.abs(stamps) > 2 ** 62, 0, stamps))
    values = (np.arange(N, dtype=np.int64) * 700 + values % 300).astype(np.int64)
    dealt = values if deal == "ascending" else np.random.default_rng(31).permutation(values)
    window = 50_000                                    # about 70 rows: the diagonal and the tile beside it
    t = make_table(rows, dealt, live)
    seen = {}
    for max_dist in (0.1, 0.2):
        pairs = window_pairs(*W[max_dist], dealt, window)
        same_pairs(t.near_pairs_window(max_dist, window), pairs, f"{deal} {max_dist}")
        seen[max_dist] = t.window_stats()
        assert np.array_equal(t.neighbor_counts_window(max_dist, window), expected_dbscan(N, *pairs, 1, live=live)[3])
        for min_pts in (2, 5):
            check_same(t.dbscan_window(max_dist, window, min_pts), expected_dbscan(N, *pairs, min_pts, live=live), f"{deal} {max_dist} {min_pts}")
    assert W[0.2][0].size > window_pairs(*W[0.2], dealt, window)[0].size > 0        # the window took pairs away, and left some
    t.near_pairs(0.2)
    plain = t.near_pairs_stats()
    t.dbscan_window(0.2, window, 5)
    st = t.window_stats()
    print(deal, seen, st, plain)
    for s in (seen[0.1], seen[0.2], st):
        assert s["tiles_pass1"] + s["tiles_skipped_pass1"] == TRIANGLE
        assert s["candidates_pass1"] <= plain["candidates"]
    assert st["tiles_pass2"] + st["tiles_skipped_pass2"] == TRIANGLE
    if deal == "ascending":
        # blocks 0 .. 11 minus the deleted one: the diagonal tiles and the neighbours on it, nothing further out
        assert st["tiles_skipped_pass1"] > 0 and 11 <= st["tiles_pass1"] <= 11 + 10
        assert st["tiles_skipped_pass1"] >= TRIANGLE - 21
    t.close()


# 10
def test_with_all_stamps_equal_nothing_is_skipped(corpus):
    rows = corpus[0]
    t = make_table(rows, np.full(N, -42, np.int64))
    same_pairs(t.near_pairs_window(0.1, 0), t.near_pairs(0.1), "equal stamps")
    st = t.window_stats()
    assert st["tiles_skipped_pass1"] == 0 and st["tiles_pass1"] == TRIANGLE and st["candidates_pass1"] == t.near_pairs_stats()["candidates"]
    assert same_arrays(t.dbscan_window(0.1, 0, 5), t.dbscan(0.1, 5))
    st, plain = t.window_stats(), t.dbscan_stats()
    assert st["tiles_skipped_pass1"] == 0 and st["tiles_pass1"] == TRIANGLE
    assert (st["tiles_pass2"], st["tiles_skipped_pass2"]) == (plain["tiles_visited"], plain["tiles_skipped"])   # the activity bytes alone
    t.close()


# 11
def test_overflow_halving_counts_every_pair_once(built):
    row = np.random.default_rng(6).standard_normal(DIM).astype(np.float32)
    t = EmbeddingTable(DIM, 0)
    t.insert(np.tile(row, (200, 1)))
    t.set_attrs(np.arange(200, dtype=np.uint64), stamps=np.full(200, 77, np.int64))
    t.set_option("join_cap", 16384)                    # 19 900 pairs: more than one buffer holds
    assert np.array_equal(t.neighbor_counts_window(0.001, 0), np.full(200, 199, np.uint32))
    st = t.window_stats()
    print("200 copies:", st)
    assert st["pairs"] == 19900 and st["launches"] > 1 and st["tiles_pass1"] == 3 and st["tiles_skipped_pass1"] == 0
    launches = st["launches"]
    got = t.dbscan_window(0.001, 0, 5)
    st = t.window_stats()
    assert np.array_equal(got["counts"], np.full(200, 199, np.uint32))
    assert got["summary"] == {"clusters": 1, "core": 200, "border": 0, "noise": 0} and np.all(got["cluster"] == 0)
    assert st["pairs"] == 19900 and st["launches"] == 2 * launches and (st["tiles_pass2"], st["tiles_skipped_pass2"]) == (3, 0)
    a, b, d = t.near_pairs_window(0.001, 0)
    assert a.size == 19900 and t.window_stats()["pairs"] == 19900
    assert np.array_equal(np.bincount(a.astype(np.int64), minlength=200) + np.bincount(b.astype(np.int64), minlength=200), np.full(200, 199))
    # one row a second later drops out of everything at window 0
    t.set_attrs([57], stamps=[78])
    want = np.full(200, 198, np.uint32)
    want[57] = 0
    assert np.array_equal(t.neighbor_counts_window(0.001, 0), want)
    assert np.array_equal(t.neighbor_counts_window(0.001, 1), np.full(200, 199, np.uint32))
    t.close()


# 12
def test_tiny_tables(built):
    t = EmbeddingTable(DIM, 0)
    assert t.neighbor_counts_window(0.1, 5).size == 0 and t.near_pairs_window(0.1, 5)[0].size == 0
    got = t.dbscan_window(0.1, 5, 1)
    assert got["cluster"].size == 0 and got["summary"] == {"clusters": 0, "core": 0, "border": 0, "noise": 0}
    assert t.window_stats()["launches"] == 0
    row = np.random.default_rng(2).standard_normal((1, DIM)).astype(np.float32)
    t.insert(row)
    assert t.neighbor_counts_window(0.1, 5).tolist() == [0] and t.near_pairs_window(0.1, 5)[0].size == 0
    got = t.dbscan_window(0.1, 5, 1)
    assert got["cluster"].tolist() == [0] and got["via"].tolist() == [0] and bits(got["via_dist"]).tolist() == [0]
    assert got["summary"] == {"clusters": 1, "core": 1, "border": 0, "noise": 0}
    assert t.dbscan_window(0.1, 5, 2)["summary"] == {"clusters": 0, "core": 0, "border": 0, "noise": 1}
    t.insert(row * np.float32(2.0))
    t.set_attrs([0, 1], stamps=[-3, 3])
    assert t.neighbor_counts_window(0.001, 6).tolist() == [1, 1] and t.neighbor_counts_window(0.001, 5).tolist() == [0, 0]
    assert t.near_pairs_window(0.001, 6)[0].tolist() == [0] and t.near_pairs_window(0.001, 5)[0].size == 0
    got = t.dbscan_window(0.001, 6, 2)
    assert got["cluster"].tolist() == [0, 0] and got["via"].tolist() == [0, 1] and got["counts"].tolist() == [1, 1]
    got = t.dbscan_window(0.001, 5, 2)
    assert got["summary"] == {"clusters": 0, "core": 0, "border": 0, "noise": 2} and got["labels"].tolist() == [-1, -1]
    assert t.dbscan_window(0.001, 5, 1)["cluster"].tolist() == [0, 1]
    t.close()


# 13
def test_dim_128_on_101_rows(built, orc):
    rng = np.random.default_rng(41)
    rows = rng.standard_normal((101, 128)).astype(np.float32)
    centre = rng.standard_normal(128)
    rows[10:30] = (centre + 0.2 * rng.standard_normal((20, 128))).astype(np.float32)
    stamps = rng.integers(-500, 500, 101).astype(np.int64)
    D = distance_matrix(orc, rows)
    t = EmbeddingTable(128, 0)
    t.insert(rows)
    t.set_attrs(np.arange(101, dtype=np.uint64), stamps=stamps)
    W = oracle_pairs(D, 0.1)
    assert W[0].size >= 100
    for window in (0, 100, 400, U64_MAX):
        pairs = window_pairs(*W, stamps, window)
        same_pairs(t.near_pairs_window(0.1, window), pairs, f"dim 128 {window}")
        check_same(t.dbscan_window(0.1, window, 4), expected_dbscan(101, *pairs, 4), f"dim 128 {window}")
    assert 0 < window_pairs(*W, stamps, 100)[0].size < W[0].size
    t.close()


# 14
def test_an_unsupported_dim_fails_as_the_join_does_and_writes_nothing(built):
    t = EmbeddingTable(64, 0)
    t.insert(np.random.default_rng(3).standard_normal((4, 64)).astype(np.float32))
    n = ctypes.c_uint64()
    code = _lib.lib().mi_knn_near_pairs(t._h, 0.1, 0, None, None, None, 0, ctypes.byref(n))
    assert code < 0
    cluster, via = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64)
    via_dist, counts, summary = np.full(4, -7.0, np.float32), np.full(4, 7, np.uint32), np.full(4, 7, np.uint64)
    a, b, d = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64), np.full(4, -7.0, np.float32)
    assert _lib.lib().mi_knn_near_pairs_window(t._h, 0.1, 5, 0, a.ctypes.data, b.ctypes.data, d.ctypes.data, 4, ctypes.byref(n)) == code
    assert _lib.lib().mi_knn_density_window(t._h, 0.1, 5, counts.ctypes.data) == code
    assert _lib.lib().mi_knn_dbscan_window(t._h, 0.1, 5, 5, cluster.ctypes.data, via.ctypes.data, via_dist.ctypes.data, counts.ctypes.data,
                                           summary.ctypes.data) == code
    assert np.all(cluster == 7) and np.all(via == 7) and np.all(via_dist == -7.0) and np.all(counts == 7) and np.all(summary == 7)
    assert np.all(a == 7) and np.all(b == 7) and np.all(d == -7.0) and n.value == 0
    with pytest.raises(MiError):
        t.dbscan_window(0.1, 5)
    t.close()


# 15
def test_error_codes_leave_the_outputs_untouched(table):
    mi, h = _lib.lib(), table._h
    cluster, via = np.full(N, 7, np.uint64), np.full(N, 7, np.uint64)
    via_dist, counts, summary = np.full(N, -7.0, np.float32), np.full(N, 7, np.uint32), np.full(4, 7, np.uint64)
    out = (cluster.ctypes.data, via.ctypes.data, via_dist.ctypes.data, counts.ctypes.data, summary.ctypes.data)
    a, b, d = np.full(8, 7, np.uint64), np.full(8, 7, np.uint64), np.full(8, -7.0, np.float32)
    pairs = (a.ctypes.data, b.ctypes.data, d.ctypes.data)
    n = ctypes.c_uint64(7)
    INVALID, UNSUPPORTED = -1, mi.mi_knn_near_pairs(h, 0.2, 0, *pairs, 8, ctypes.byref(n))     # more than cap pairs, as the join reports it
    assert UNSUPPORTED < 0 and n.value == 9
    before = table.window_stats()
    for max_dist in (float("nan"), -0.1):
        assert mi.mi_knn_near_pairs_window(h, max_dist, WINDOW, 0, *pairs, 8, ctypes.byref(n)) == INVALID and n.value == 0
        assert mi.mi_knn_density_window(h, max_dist, WINDOW, counts.ctypes.data) == INVALID
        assert mi.mi_knn_dbscan_window(h, max_dist, WINDOW, 5, *out) == INVALID
    assert mi.mi_knn_dbscan_window(h, 0.1, WINDOW, 0, *out) == INVALID
    assert mi.mi_knn_dbscan_window(None, 0.1, WINDOW, 5, *out) == INVALID
    assert mi.mi_knn_density_window(None, 0.1, WINDOW, counts.ctypes.data) == INVALID
    assert mi.mi_knn_near_pairs_window(None, 0.1, WINDOW, 0, *pairs, 8, ctypes.byref(n)) == INVALID
    assert mi.mi_knn_density_window(h, 0.1, WINDOW, None) == INVALID
    assert mi.mi_knn_dbscan_window(h, 0.1, WINDOW, 5, None, *out[1:]) == INVALID
    assert mi.mi_knn_dbscan_window(h, 0.1, WINDOW, 5, *out[:4], None) == INVALID
    assert mi.mi_knn_near_pairs_window(h, 0.1, WINDOW, 0, *pairs, 8, None) == INVALID
    assert mi.mi_knn_near_pairs_window(h, 0.1, WINDOW, 0, None, b.ctypes.data, d.ctypes.data, 8, ctypes.byref(n)) == INVALID
    assert table.window_stats() == before                                                            # refused in front of the table
    assert mi.mi_knn_near_pairs_window(h, 0.1, WINDOW, N + 5, *pairs, 8, ctypes.byref(n)) == INVALID    # first_new is no row
    assert np.all(cluster == 7) and np.all(via == 7) and np.all(via_dist == -7.0) and np.all(counts == 7) and np.all(summary == 7)
    assert np.all(a == 7) and np.all(b == 7) and np.all(d == -7.0)
    # more than cap pairs: the cap protocol of mi_knn_near_pairs
    n.value = 7
    assert mi.mi_knn_near_pairs_window(h, 0.2, WINDOW, 0, *pairs, 8, ctypes.byref(n)) == UNSUPPORTED and n.value == 9
    assert mi.mi_knn_near_pairs_window(h, 0.2, WINDOW, 0, None, None, None, 0, ctypes.byref(n)) == UNSUPPORTED and n.value == 1
    with pytest.raises(MiError):
        table.near_pairs_window(0.2, WINDOW, cap=8)


# 16
def test_index_bursts_and_events(built, tmp_path):
    rng = np.random.default_rng(12)
    media = str(tmp_path / "media") + "/"   # (rows store media_dir + <rel>)
    names = [f"{media}{folder}/{i}.jpg" for folder in ("a", "b", "c") for i in range(40)]
    emb = rng.standard_normal((120, DIM)).astype(np.float32)
    ca, cb = rng.standard_normal(DIM), rng.standard_normal(DIM)
    beach, jump = list(range(10, 22)), list(range(50, 59))
    emb[beach] = blob(rng, ca, 0.2, len(beach), 1.0)                # one look: six pictures in 2019, six in 2023
    emb[jump] = blob(rng, cb, 0.05, len(jump), 5.0)                 # nine shots of one jump, a second apart
    stamps = 1_500_000_000 + 50_000 * np.arange(120, dtype=np.int64)
    stamps[beach[:6]] = T_A1 + 600 * np.arange(6)
    stamps[beach[6:]] = T_A2 + 600 * np.arange(6)
    stamps[jump] = T_BURST + np.arange(9)
    ix = ImageIndex(DIM, 0, media)
    ix.insert(names, emb)
    ix.set_attrs(names, stamps=stamps)
    paths = lambda rows: [names[r] for r in rows]
    themes, _ = ix.themes(0.1, min_pts=4)
    assert themes == [paths(beach), paths(jump)]
    events, noise = ix.events(0.1, WINDOW, min_pts=4)
    assert events == [paths(jump), paths(beach[:6]), paths(beach[6:])]             # the largest first, equal sizes by their first row
    assert sorted(noise) == sorted(names[r] for r in range(120) if r not in beach + jump)
    got = ix.table.dbscan_window(0.1, WINDOW, 4)
    assert [np.flatnonzero(got["labels"] == l).tolist() for l in range(3)] == [beach[:6], beach[6:], jump]
    assert ix.events(0.1, WINDOW, min_pts=4, web=True)[0][0][0] == "media/b/10.jpg"     # row 50: the eleventh picture of folder b
    assert ix.events(0.1, U64_MAX, min_pts=4) == ix.themes(0.1, min_pts=4)
    # bursts: the components of W_win, against pairs_to_groups over the table call
    for window in (0, 3, WINDOW, U64_MAX):
        a, b, _ = ix.table.near_pairs_window(0.1, window)
        groups = [paths(int(i) for i in g) for g in pairs_to_groups(a, b)]
        assert ix.bursts(0.1, window) == groups, window
    assert ix.bursts(0.1, WINDOW) == [paths(beach[:6]), paths(beach[6:]), paths(jump)]
    assert ix.bursts(0.1, 3) == [paths(jump)] and ix.bursts(0.1, 0) == []        # three seconds chain the nine shots; nothing is simultaneous
    assert ix.bursts(0.1, U64_MAX) == ix.duplicates(0.1) == [paths(beach), paths(jump)]
    assert ix.bursts(0.1, 3, web=True)[0][0] == "media/b/10.jpg"     # row 50: the eleventh picture of folder b
    with pytest.raises(MiError):
        ix.bursts(0.1, WINDOW, max_pairs=4)
    ix.remove([names[52], names[11]])
    events, noise = ix.events(0.1, WINDOW, min_pts=4)
    assert events == [paths(r for r in jump if r != 52), paths(beach[6:]), paths(r for r in beach[:6] if r != 11)]
    assert names[52] not in noise and names[11] not in noise
    assert ix.bursts(0.1, WINDOW) == [paths(r for r in beach[:6] if r != 11), paths(beach[6:]), paths(r for r in jump if r != 52)]
    ix.close()
