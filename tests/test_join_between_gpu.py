"""The join of two row sets on the GPU: mi_knn_near_pairs_between (two tables), mi_knn_sharded_near_pairs (the pairs of a
sharded table, those that cross shards included) and mi_index_matches.  Expected values are the oracle's single pass
(oracle.c: orc_cosine_dist) with the stated row as the query — the row of the first table between two tables, the row with the
smaller id inside a sharded table — thresholded on that fp32 value; ids and distance bits are compared for equality."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd._lib import MiError
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable
from oracle.binding import orc_cosine_dist

pytestmark = pytest.mark.gpu

DIM = 768
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
SPLIT, BASE_B = 2637, 10_000          # table A = rows[:SPLIT] under ids 0 .., table B = rows[SPLIT:] under ids BASE_B ..
# (shards, block rows).  The third layout was meant to be (2, 1000): mi_knn_sharded_create takes only blocks of whole scan
# tiles (multiples of 64; tests/test_sharded_gpu.py pins the refusal), so it is the nearest block that is no multiple of the
# join's 128-row tile, and test_block_rows_of_1000_are_refused says why.
LAYOUTS = ((3, 256), (4, 128), (2, 960))


def planted_corpus(n=4096, seed=7):
    """tests/test_join_gpu.py's corpus, restated: 320 noisy, rescaled copies of rows below 2048 at rows 3000 .. 3319"""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, DIM)).astype(np.float32)
    src = rng.integers(0, 2048, 320)
    scale = rng.uniform(0.1, 10.0, 320)
    sigma = np.concatenate([np.zeros(20), np.linspace(0.02, 0.32, 300)])
    noise = rng.standard_normal((320, DIM))
    rows[3000:3320] = ((rows[src] + sigma[:, None] * noise) * scale[:, None]).astype(np.float32)
    return rows


def distance_matrix(orc, qs, rows):
    """D[a, b] = what the single pass with q = qs[a] reports for rows[b]"""
    return np.stack([orc_cosine_dist(orc, q, rows) for q in qs])


def oracle_self(D, max_dist, live=None, first_new=0):
    """pairs a < b of one id space, the smaller id the query; first_new: only b >= first_new"""
    n = D.shape[0]
    ok = np.triu(np.ones((n, n), bool), 1) & (D <= np.float32(max_dist))   # (a NaN compares false: never a pair)
    if live is not None:
        ok &= live[:, None] & live[None, :]
    ok[:, :first_new] = False
    a, b = np.nonzero(ok)   # row-major: ascending by (a, b)
    return a.astype(np.uint64), b.astype(np.uint64), D[a, b]


def oracle_between(D, max_dist, base_a=0, base_b=0, live_a=None, live_b=None):
    """D [rows of A][rows of B] with A's row as the query -> (id in A, id in B, dist), ascending by (a, b)"""
    ok = D <= np.float32(max_dist)
    if live_a is not None:
        ok = ok & live_a[:, None]
    if live_b is not None:
        ok = ok & live_b[None, :]
    a, b = np.nonzero(ok)
    return a.astype(np.uint64) + np.uint64(base_a), b.astype(np.uint64) + np.uint64(base_b), D[a, b]


def same(got, want, what=""):
    ga, gb, gd = got
    wa, wb, wd = want
    assert ga.size == wa.size, (what, ga.size, wa.size)
    assert np.array_equal(ga, wa) and np.array_equal(gb, wb), what
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what


def keep_of(res, keep):
    return res[0][keep], res[1][keep], res[2][keep]


def raw_call(fn, lead, cap):
    a, b, d = np.empty(max(cap, 1), np.uint64), np.empty(max(cap, 1), np.uint64), np.empty(max(cap, 1), np.float32)
    n = ctypes.c_uint64()
    rc = fn(*lead, a.ctypes.data, b.ctypes.data, d.ctypes.data, cap, ctypes.byref(n))
    return rc, n.value


def sharded_of(rows, shards, block, **options):
    t = ShardedTable(DIM, [0] * shards, block)
    t.insert(rows)
    for k, v in options.items():
        t.set_option(k, v)
    return t


def two_tables(rows_a, rows_b, base_b=BASE_B, **options):
    ta, tb = EmbeddingTable(DIM, 0), EmbeddingTable(DIM, 0)
    if len(rows_a):
        ta.insert(rows_a)
    tb.set_base(base_b)
    if len(rows_b):
        tb.insert(rows_b)
    for k, v in options.items():
        ta.set_option(k, v)
    return ta, tb


@pytest.fixture(scope="module")
def corpus(built, orc):
    rows = planted_corpus()
    return rows, distance_matrix(orc, rows, rows)


@pytest.fixture(scope="module")
def single(corpus):
    """one table with every row, and its own join at the three thresholds: what a sharded table must equal"""
    t = EmbeddingTable(DIM, 0)
    t.insert(corpus[0])
    full = {max_dist: t.near_pairs(max_dist) for max_dist in (0.0, 0.02, 0.05)}
    tiles = t.near_pairs_stats()["tiles"]
    yield t, full, tiles
    t.close()


# 1: the sharded table equals the single table, pairs across shards and the query rule included
@pytest.mark.parametrize("shards,block", LAYOUTS)
def test_sharded_equals_single(corpus, single, shards, block):
    rows, D = corpus
    _, full, _ = single
    t = sharded_of(rows, shards, block)
    for max_dist in (0.0, 0.02, 0.05):
        got = t.near_pairs(max_dist)
        same(got, full[max_dist], (shards, block, max_dist))
        st = t.near_pairs_stats()
        assert st["pairs"] == got[0].size and st["candidates"] >= st["pairs"]
        sa, sb = (got[0] // np.uint64(block)) % np.uint64(shards), (got[1] // np.uint64(block)) % np.uint64(shards)
        print(f"{shards} x {block}, max_dist {max_dist}: {got[0].size} pairs, {int((sa != sb).sum())} cross shards, "
              f"{int((sa > sb).sum())} with the smaller id on the higher shard, {st}")
    same(got, oracle_self(D, 0.05), "the oracle at 0.05")
    # the inputs do exercise what they are meant to (a float64 restatement of this corpus gives the same counts)
    assert [full[m][0].size for m in (0.0, 0.02, 0.05)] == [21, 209, 337]
    if (shards, block) == (3, 256):
        assert int((sa != sb).sum()) == 225 and int((sa > sb).sum()) == 164
    t.close()


def test_block_rows_of_1000_are_refused(built):
    with pytest.raises(MiError, match="multiple of 64") as e:
        ShardedTable(DIM, [0, 0], 1000)
    assert e.value.code == MI_ERR_INVALID


def test_sharded_duplicates_are_the_groups_of_the_pairs(corpus, single):
    from image_search_amd.search import pairs_to_groups
    rows, _ = corpus
    _, full, _ = single
    t = sharded_of(rows, 3, 256)
    want = pairs_to_groups(full[0.02][0], full[0.02][1])
    got = t.duplicates(0.02)
    assert [g.tolist() for g in got] == [g.tolist() for g in want] and len(got) > 10
    t.close()


# 2: the tile identity — derived: S m (m + 1) / 2 + S (S - 1) / 2 m^2 = S m (S m + 1) / 2 when shards are whole tiles
def test_tile_identity(corpus, single):
    rows, _ = corpus
    _, full, single_tiles = single
    assert single_tiles == 32 * 33 // 2 == 528
    t = sharded_of(rows, 4, 128)
    same(t.near_pairs(0.05), full[0.05])
    st = t.near_pairs_stats()
    assert st["tiles"] == 528, st
    assert st["launches"] == 4 + 6, st        # no overflow at this threshold: one launch per shard and per shard pair
    t.close()


# 3: first_new
def test_sharded_first_new(corpus, single):
    rows, _ = corpus
    _, full, _ = single
    t = sharded_of(rows, 3, 256)
    same(t.near_pairs(0.05), full[0.05])
    tiles_all = t.near_pairs_stats()["tiles"]
    for first_new in (1077, 3000, 4095):
        same(t.near_pairs(0.05, first_new=first_new), keep_of(full[0.05], full[0.05][1] >= first_new), first_new)
        if first_new == 3000:
            assert t.near_pairs_stats()["tiles"] < tiles_all
    assert t.near_pairs(0.05, first_new=4096)[0].size == 0
    with pytest.raises(MiError) as e:
        t.near_pairs(0.05, first_new=4097)
    assert e.value.code == MI_ERR_INVALID
    t.close()


# 4: between two tables, both row counts ragged
@pytest.fixture(scope="module")
def between_want(corpus):
    _, D = corpus
    want = oracle_between(D[:SPLIT, SPLIT:], 0.05, 0, BASE_B)
    assert want[0].size == 320 and int((np.bincount(want[0].astype(np.int64)) > 1).sum()) == 19
    return want


def test_between_two_tables(corpus, between_want):
    rows, _ = corpus
    ta, tb = two_tables(rows[:SPLIT], rows[SPLIT:])
    before = [t.knn(rows[5], 10) for t in (ta, tb)]
    got = ta.near_pairs_with(tb, 0.05)
    same(got, between_want, "between")
    st = ta.near_pairs_with_stats()
    assert st["pairs"] == 320 and st["candidates"] >= 320 and st["tiles"] == 21 * 12 and st["launches"] == 1, st
    assert len(ta) == SPLIT and len(tb) == 4096 - SPLIT
    for t, (idx, dist) in zip((ta, tb), before):
        idx2, dist2 = t.knn(rows[5], 10)
        assert np.array_equal(idx, idx2) and np.array_equal(dist.view(np.uint32), dist2.view(np.uint32))
    # the bits of a search of B with A's row as the query
    a, b, d = got
    for j in np.random.default_rng(1).choice(a.size, 32, replace=False):
        idx, dist = tb.knn(rows[int(a[j])], 64)
        at = np.nonzero(idx == b[j])[0]
        assert at.size == 1, (int(a[j]), int(b[j]))
        assert dist[at[0]].view(np.uint32) == d[j].view(np.uint32)
    # the other way round B's row is the query: same pairs, each distance the oracle's with the roles swapped
    back = tb.near_pairs_with(ta, 0.02)
    assert back[0].size > 100 and np.all(back[0] >= BASE_B) and np.all(back[1] < SPLIT)
    with pytest.raises(MiError) as e:
        ta.near_pairs_with(ta, 0.05)
    assert e.value.code == MI_ERR_INVALID
    other_dim = EmbeddingTable(512, 0)
    with pytest.raises(MiError) as e:
        ta.near_pairs_with(other_dim, 0.05)
    assert e.value.code == MI_ERR_INVALID
    other_dim.close(); ta.close(); tb.close()


# 5: the staged column side: what runs between devices, on one device
def test_staged_path_equals_the_direct_one(corpus, single, between_want):
    rows, _ = corpus
    _, full, _ = single
    for options in ({"join_stage": 1}, {"join_stage": 1, "join_stage_rows": 512}):
        for shards, block in ((3, 256), (2, 960)):       # chunks of 512: every shard spans >= 3, the last one short at 2 x 960
            t = sharded_of(rows, shards, block, **options)
            for max_dist in (0.0, 0.02, 0.05):
                same(t.near_pairs(max_dist), full[max_dist], (options, shards, block, max_dist))
            same(t.near_pairs(0.05, first_new=3000), keep_of(full[0.05], full[0.05][1] >= 3000), (options, "first_new"))
            t.close()
    # B = 1459 rows: 640 + 640 + 179, staged and (the same chunks by pointer) read where it lies
    for options in ({"join_stage": 1}, {"join_stage": 1, "join_stage_rows": 640}, {"join_stage_rows": 640}):
        ta, tb = two_tables(rows[:SPLIT], rows[SPLIT:], **options)
        same(ta.near_pairs_with(tb, 0.05), between_want, options)
        st = ta.near_pairs_with_stats()
        assert st["launches"] == (3 if "join_stage_rows" in options else 1) and st["tiles"] == 21 * 12, st
        ta.close(); tb.close()


# 6: shapes
def test_shapes(built, orc):
    rng = np.random.default_rng(2)
    row = rng.standard_normal((1, DIM)).astype(np.float32)
    ta, tb = two_tables(row, np.zeros((0, DIM), np.float32))
    assert ta.near_pairs_with(tb, 0.1)[0].size == 0 and tb.near_pairs_with(ta, 0.1)[0].size == 0     # an empty side
    tb.insert(row)
    a, b, d = ta.near_pairs_with(tb, 0.001)
    assert a.tolist() == [0] and b.tolist() == [BASE_B] and d.view(np.uint32)[0] == orc_cosine_dist(orc, row[0], row).view(np.uint32)[0]
    ta.close(); tb.close()
    # 129 x 127 rows: A's last row (alone in its second tile) is B's last row, rescaled
    ra, rb = rng.standard_normal((129, DIM)).astype(np.float32), rng.standard_normal((127, DIM)).astype(np.float32)
    ra[128] = rb[126] * np.float32(3.0)
    for options in ({}, {"join_stage": 1}):
        ta, tb = two_tables(ra, rb, **options)
        want = oracle_between(distance_matrix(orc, ra, rb), 0.01, 0, BASE_B)
        assert list(zip(want[0].tolist(), want[1].tolist())) == [(128, BASE_B + 126)]
        same(ta.near_pairs_with(tb, 0.01), want, options)
        assert ta.near_pairs_with_stats()["tiles"] == 2
        ta.close(); tb.close()
    # a sharded table with fewer rows than shards x block: shards 2 and 3 hold nothing
    rows = rng.standard_normal((300, DIM)).astype(np.float32)
    rows[290] = rows[10] * np.float32(0.5)            # shard 0 x shard 1
    rows[255] = rows[200]                             # inside shard 0
    one = EmbeddingTable(DIM, 0)
    one.insert(rows)
    want = one.near_pairs(0.01)
    assert list(zip(want[0].tolist(), want[1].tolist())) == [(10, 290), (200, 255)]
    t = sharded_of(rows, 4, 256)
    assert [t.shard_rows(s) for s in range(4)] == [256, 44, 0, 0]
    same(t.near_pairs(0.01), want, "empty shards")
    same(t.near_pairs(0.01, first_new=256), keep_of(want, want[1] >= 256), "empty shards, first_new")
    t.close(); one.close()


# 7: deleted rows, between and sharded
def test_deleted_rows_are_left_out(corpus, single, between_want):
    rows, D = corpus
    _, full, _ = single
    rng = np.random.default_rng(4)
    planted = rng.choice(np.arange(3000, 3320), 50, replace=False)
    sources = np.unique(full[0.05][0][np.isin(full[0.05][1], np.arange(3000, 3320)) & (full[0.05][0] < 2048)])
    sources = rng.choice(sources, 50, replace=False)
    gone = np.concatenate([planted, sources]).astype(np.uint64)
    live = np.ones(4096, bool)
    live[gone.astype(np.int64)] = False
    want = oracle_self(D, 0.05, live=live)
    same(want, keep_of(full[0.05], ~np.isin(full[0.05][0], gone) & ~np.isin(full[0.05][1], gone)), "the full result minus the deleted ids")
    assert want[0].size < full[0.05][0].size
    for options in ({}, {"join_stage": 1, "join_stage_rows": 512}, {"join_stage_rows": 512}):
        t = sharded_of(rows, 3, 256, **options)
        assert t.delete(gone) == 100
        same(t.near_pairs(0.05), want, ("sharded, deleted", options))
        t.close()
        # between: the planted rows lie in B, their sources in A
        ta, tb = two_tables(rows[:SPLIT], rows[SPLIT:], **options)
        assert ta.delete(sources.astype(np.uint64)) == 50
        assert tb.delete((planted - SPLIT + BASE_B).astype(np.uint64)) == 50
        got = ta.near_pairs_with(tb, 0.05)
        same(got, oracle_between(D[:SPLIT, SPLIT:], 0.05, 0, BASE_B, live[:SPLIT], live[SPLIT:]), ("between, deleted", options))
        keep = ~np.isin(between_want[0], sources.astype(np.uint64)) & ~np.isin(between_want[1], (planted - SPLIT + BASE_B).astype(np.uint64))
        same(got, keep_of(between_want, keep), "the full result minus the deleted ids")
        ta.close(); tb.close()


# 7: special rows, every pair straddling the two tables / the two shards
def test_special_rows(built, orc):
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((300, DIM)).astype(np.float32)
    rows[10] = 0.0; rows[200] = 0.0                              # a zero row and its copy: NaN, never a pair
    rows[20, 5] = np.float32(3.2e38); rows[210] = rows[20]       # marked: an element bf16 would round to inf
    rows[30, 7] = np.inf                                         # marked: an inf
    direction = rng.standard_normal(DIM).astype(np.float32)
    rows[40] = direction * np.float32(1e-17)                     # squared norms 7.7e-32 and 7.7e34: both marked,
    rows[220] = direction * np.float32(1e16)                     # both finite in fp32: a pair the join must find
    rows[260] = rows[100] * np.float32(2.0)                      # and an ordinary pair beside them
    D = distance_matrix(orc, rows, rows)
    assert D[40, 220] <= np.float32(0.01) and not (D[10, 200] <= np.float32(2.0))
    for options in ({}, {"join_stage": 1}):
        ta, tb = two_tables(rows[:150], rows[150:], base_b=150, **options)
        t = sharded_of(rows, 2, 64, **options)     # blocks of 64: 10 | 200, 20 | 210, 40 | 220 and 100 | 260 lie on different shards
        for max_dist in (0.01, 1.5):
            got = ta.near_pairs_with(tb, max_dist)
            same(got, oracle_between(D[:150, 150:], max_dist, 0, 150), ("between", max_dist, options))
            pairs = set(zip(got[0].tolist(), got[1].tolist()))
            assert (40, 220) in pairs and (100, 260) in pairs and (10, 200) not in pairs
            got = t.near_pairs(max_dist)
            same(got, oracle_self(D, max_dist), ("sharded", max_dist, options))
            pairs = set(zip(got[0].tolist(), got[1].tolist()))
            assert (40, 220) in pairs and (100, 260) in pairs and (10, 200) not in pairs
        ta.close(); tb.close(); t.close()


# 8: the cap
def test_cap_stops_the_call_and_leaves_the_handles_usable(corpus, single, between_want):
    rows, _ = corpus
    _, full, _ = single
    mi = _lib.lib()
    ta, tb = two_tables(rows[:SPLIT], rows[SPLIT:])
    rc, n = raw_call(mi.mi_knn_near_pairs_between, (ta._h, tb._h, ctypes.c_float(0.05)), 100)
    assert rc == MI_ERR_UNSUPPORTED and n == 101 and b"cap" in mi.mi_last_error()
    rc, n = raw_call(mi.mi_knn_near_pairs_between, (ta._h, tb._h, ctypes.c_float(0.05)), 320)      # exactly enough
    assert rc == 0 and n == 320
    same(ta.near_pairs_with(tb, 0.05), between_want, "after the refused call")
    ta.close(); tb.close()
    t = sharded_of(rows, 3, 256)
    for cap in (10, 200, 336):   # stops inside the self-joins, inside the shard pairs, one short
        rc, n = raw_call(mi.mi_knn_sharded_near_pairs, (t._h, ctypes.c_float(0.05), 0), cap)
        assert rc == MI_ERR_UNSUPPORTED and n == cap + 1, (cap, rc, n)
    rc, n = raw_call(mi.mi_knn_sharded_near_pairs, (t._h, ctypes.c_float(0.05), 0), 337)
    assert rc == 0 and n == 337
    same(t.near_pairs(0.05), full[0.05], "after the refused calls")
    t.close()


# 8: the overflow path
def test_everything_matches_everything(built, orc):
    n = 1500
    row = np.random.default_rng(6).standard_normal(DIM).astype(np.float32)
    ta, tb = two_tables(np.tile(row, (n, 1)), np.tile(row, (n, 1)), join_cap=1 << 16)   # one tile row holds 128 x 1500 candidates
    a, b, d = ta.near_pairs_with(tb, 0.001, cap=1 << 22)
    st = ta.near_pairs_with_stats()
    print("all matches:", st)
    assert a.size == n * n == st["pairs"] == st["candidates"]
    assert np.array_equal(a, np.repeat(np.arange(n, dtype=np.uint64), n))
    assert np.array_equal(b, np.tile(np.arange(n, dtype=np.uint64) + np.uint64(BASE_B), n))
    assert np.all(d.view(np.uint32) == orc_cosine_dist(orc, row, row[None]).view(np.uint32)[0])
    assert st["launches"] > (n + 127) // 128    # more launches than tile rows: tile rows were cut into column ranges
    ta.close(); tb.close()


# 9: the index
def test_index_matches(built, tmp_path):
    rng = np.random.default_rng(12)
    mine, card = str(tmp_path / "library") + "/", str(tmp_path / "card") + "/"
    names_a = [f"{mine}{folder}/{i}.jpg" for folder in ("a", "b") for i in range(40)]
    names_b = [f"{card}DCIM/{i}.jpg" for i in range(30)]
    ea, eb = rng.standard_normal((80, DIM)).astype(np.float32), rng.standard_normal((30, DIM)).astype(np.float32)
    eb[4] = ea[45] * np.float32(2.0)      # b/5 is on the card, rescaled
    eb[20] = ea[3]                        # a/3 twice
    eb[21] = ea[3]
    ia, ib = ImageIndex(DIM, 0, mine), ImageIndex(DIM, 0, card)
    ia.insert(names_a, ea)
    ib.insert(names_b, eb)
    got = ia.matches(ib, 0.01)
    assert [(x, y) for x, y, _ in got] == [(names_a[3], names_b[20]), (names_a[3], names_b[21]), (names_a[45], names_b[4])]
    assert all(0.0 <= d <= 0.01 for _, _, d in got)
    assert [(x, y) for x, y, _ in ia.matches(ib, 0.01, web=True)][0] == ("media/a/3.jpg", "media/DCIM/20.jpg")   # the client's names: media_dir -> media/
    assert [(x, y) for x, y, _ in ib.matches(ia, 0.01)] == [(names_b[4], names_a[45]), (names_b[20], names_a[3]), (names_b[21], names_a[3])]
    ib.remove([names_b[20]])
    assert [(x, y) for x, y, _ in ia.matches(ib, 0.01)] == [(names_a[3], names_b[21]), (names_a[45], names_b[4])]
    ia.remove([names_a[45]])
    assert [(x, y) for x, y, _ in ia.matches(ib, 0.01)] == [(names_a[3], names_b[21])]
    with pytest.raises(MiError):
        ia.matches(ib, 2.0, max_pairs=5)
    assert len(ia) == 80 and len(ib) == 30
    ia.close(); ib.close()
