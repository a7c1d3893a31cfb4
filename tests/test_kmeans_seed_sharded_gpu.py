"""mi_knn_sharded_kmeans_seed on the GPU: k-means++ seeding across the shards, compared TO THE BIT with
EmbeddingTable.kmeans_seed on ONE table holding the same rows — the picked rows in pick order, the centroids, the potential
(equality of the double) and the stats — on every layout, and once with the numpy restatement of the contract
(tests/test_kmeans_seed_host.py) fed by the CPU oracle's distances.  Every shard is on device 0.  There is no tolerance
anywhere in this file."""
import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ShardedTable
from test_kmeans_seed_host import oracle_dist_from, planted_unequal, restate_seed

pytestmark = pytest.mark.gpu

MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
LAYOUTS = [(1, 4096), (3, 64), (2, 128), (4, 64), (2, 960)]   # (shards, block)
CHUNK = 256


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f64_bits(x):
    return np.float64(x).view(np.uint64)


def gaussian(seed, n, dim):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    return rows * rng.uniform(0.1, 10.0, (n, 1)).astype(np.float32)


def table_of(rows):
    t = EmbeddingTable(rows.shape[1], 0)
    t.insert(rows)
    return t


def sharded_of(rows, shards, block):
    t = ShardedTable(rows.shape[1], [0] * shards, block)
    t.insert(rows)
    return t


def expected_bytes(shards, block, cand, C, dim):
    """the closed form of include/mi355clip.h: K = the chunks of shards 1 .. (at most 256 candidates of one block each)"""
    if shards <= 1:
        return 0
    blocks, counts = np.unique(np.asarray(cand, np.int64) // block, return_counts=True)
    K = int(sum(-(-int(n) // CHUNK) for b, n in zip(blocks, counts) if b % shards != 0))
    return (C + 1) * 8 * (K + shards - 1) + C * (shards - 1) * (32 + 8 * dim)


def same_seeding(one, many, C, seed, among=None, what=""):
    """many.kmeans_seed == one.kmeans_seed, by bits, with the first three stats words; -> the sharded result"""
    want, got = one.kmeans_seed(C, seed, among), many.kmeans_seed(C, seed, among)
    sw, sg = one.kmeans_seed_stats(), many.kmeans_seed_stats()
    print(f"{what} C {C} seed {seed}: potential {got['potential']:.6f} (one table {want['potential']:.6f}), stats {sg}")
    assert got["rows"].tolist() == want["rows"].tolist(), what
    assert np.array_equal(bits(got["centroids"]), bits(want["centroids"])), what
    assert f64_bits(got["potential"]) == f64_bits(want["potential"]), (what, got["potential"], want["potential"])
    assert {k: sg[k] for k in ("candidates", "passes", "fallbacks")} == sw, (what, sg, sw)
    return got


def rc_of(t, C, seed=0, among=None, n_among=0):
    out = np.zeros(max(C, 1), np.uint64)
    return _lib.lib().mi_knn_sharded_kmeans_seed(t._h, C, seed, among, n_among, out.ctypes.data, None, None)


# ---- 1: every layout, ragged against the 16-lane groups, the chunks and the blocks --------------------------------------------

@pytest.fixture(scope="module")
def ragged(built):
    rows = gaussian(31, 3001, 768)
    one = table_of(rows)
    want = {}   # the one table's answers, computed once per (C, seed)
    tables = {}
    yield rows, one, want, tables
    one.close()
    for t in tables.values():
        t.close()


def ragged_layout(ragged, layout):
    rows, one, want, tables = ragged
    if layout not in tables:
        tables[layout] = sharded_of(rows, *layout)
    return tables[layout]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("C", [1, 16, 64])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l[0]}x{l[1]}")
def test_all_layouts_equal_one_table(ragged, layout, C, seed):
    rows, one, want, _ = ragged
    t = ragged_layout(ragged, layout)
    if (C, seed) not in want:
        want[(C, seed)] = (one.kmeans_seed(C, seed), one.kmeans_seed_stats())
    w, sw = want[(C, seed)]
    got, sg = t.kmeans_seed(C, seed), t.kmeans_seed_stats()
    assert got["rows"].tolist() == w["rows"].tolist()
    assert np.array_equal(bits(got["centroids"]), bits(w["centroids"]))
    assert np.array_equal(bits(got["centroids"]), bits(rows[got["rows"].astype(np.int64)]))
    assert f64_bits(got["potential"]) == f64_bits(w["potential"])
    assert (sg["candidates"], sg["passes"], sg["fallbacks"]) == (3001, C + 1, sw["fallbacks"])
    assert sg["bytes_exchanged"] == expected_bytes(*layout, np.arange(3001), C, 768)


def test_restatement_fed_by_the_oracle(ragged, orc):
    rows, _, _, _ = ragged
    t = ragged_layout(ragged, (3, 64))
    dist_from, usable = oracle_dist_from(orc, rows)
    picks, potential, fallbacks = restate_seed(rows.shape[0], 16, 0, dist_from, usable)
    got = t.kmeans_seed(16, 0)
    assert got["rows"].tolist() == picks
    assert np.array_equal(bits(got["centroids"]), bits(rows[picks]))
    assert f64_bits(got["potential"]) == f64_bits(potential)
    assert t.kmeans_seed_stats()["fallbacks"] == fallbacks


# ---- 2: the shortest and the longest row ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [128, 1024])
def test_other_dims(built, dim):
    rows = gaussian(32 + dim, 300, dim)
    one, many = table_of(rows), sharded_of(rows, 3, 64)
    same_seeding(one, many, 8, 1, what=f"dim {dim}")
    one.close()
    many.close()


# ---- 3: shards without rows; C == S ---------------------------------------------------------------------------------------

def test_empty_shards_and_every_candidate_picked(built):
    rows = gaussian(40, 100, 128)
    one, many = table_of(rows), sharded_of(rows, 4, 64)          # blocks 0 and 1 only: shards 2 and 3 hold nothing
    got = same_seeding(one, many, 100, 3, what="C == S")
    assert sorted(got["rows"].tolist()) == list(range(100))
    assert many.kmeans_seed_stats()["bytes_exchanged"] == expected_bytes(4, 64, np.arange(100), 100, 128)
    assert rc_of(many, 101) == MI_ERR_INVALID
    one.close()
    many.close()


# ---- 4: among and deletions ---------------------------------------------------------------------------------------------------

def test_among_and_deletions(built):
    rng = np.random.default_rng(33)
    rows = gaussian(34, 800, 128)
    one, many = table_of(rows), sharded_of(rows, 3, 64)
    ids = rng.integers(0, 800, 500).astype(np.uint64)           # unsorted, with duplicates
    assert np.unique(ids).size < ids.size
    dead = np.union1d(np.unique(ids)[::9], np.array([1, 2, 3], np.uint64))   # deleted rows among them (and beside them)
    one.delete(dead)
    many.delete(dead)
    cand = np.setdiff1d(np.unique(ids), dead)
    for C, seed in ((1, 0), (12, 5), (40, 6)):
        got = same_seeding(one, many, C, seed, among=ids, what="among")
        assert np.all(np.isin(got["rows"], cand))
        assert many.kmeans_seed_stats()["candidates"] == cand.size
        assert many.kmeans_seed_stats()["bytes_exchanged"] == expected_bytes(3, 64, cand, C, 128)
    same_seeding(one, many, 30, 2, what="every live row, rows deleted")
    # shard 1's blocks only: shards 0 and 2 take part with zero chunks
    mine = np.flatnonzero((np.arange(800) // 64) % 3 == 1).astype(np.uint64)
    got = same_seeding(one, many, 20, 4, among=rng.permutation(mine), what="one shard's blocks")
    assert np.all((got["rows"].astype(np.int64) // 64) % 3 == 1)
    beyond = np.append(ids, np.uint64(800))
    assert rc_of(many, 4, among=beyond.ctypes.data, n_among=beyond.size) == MI_ERR_INVALID
    assert b"not a row" in _lib.lib().mi_last_error()
    assert rc_of(many, 1, among=ids.ctypes.data, n_among=0) == MI_ERR_INVALID
    with pytest.raises(_lib.MiError):
        many.kmeans_seed(1, 0, among=[])
    assert rc_of(many, 1, among=None, n_among=3) == MI_ERR_INVALID
    assert rc_of(many, 65537) == MI_ERR_UNSUPPORTED
    one.close()
    many.close()


# ---- 5: deletions, before and after an append ---------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [(3, 64), (2, 128)], ids=lambda l: f"{l[0]}x{l[1]}")
def test_deletions_after_an_append(built, layout):
    rng = np.random.default_rng(35)
    rows = gaussian(36, 900, 128)
    one, many = table_of(rows[:600]), sharded_of(rows[:600], *layout)
    dead = rng.choice(600, 60, replace=False).astype(np.uint64)
    one.delete(dead)
    many.delete(dead)
    got = same_seeding(one, many, 24, 7, what="600 rows, 60 deleted")
    assert not np.isin(got["rows"], dead).any()
    one.insert(rows[600:])
    many.insert(rows[600:])
    more = rng.choice(np.arange(600, 900), 30, replace=False).astype(np.uint64)
    one.delete(more)
    many.delete(more)
    got = same_seeding(one, many, 24, 7, what="900 rows, 90 deleted")
    assert not np.isin(got["rows"], np.concatenate([dead, more])).any()
    assert many.kmeans_seed_stats()["candidates"] == 810
    one.close()
    many.close()


# ---- 6: fallbacks at the lowest global positions, within one shard's block and from shard to shard --------------------------------

@pytest.mark.parametrize("layout", [(4, 64), (2, 128)], ids=lambda l: f"{l[0]}x{l[1]}")
def test_copies_fall_back_to_the_lowest_unpicked_global_positions(built, layout):
    """40 copies each of 3 distinct rows whose squared norms (4, 9, 1/4) and their roots are exact in fp32 (the rows of
    test_copies_fall_back_to_the_lowest_unpicked_positions): a copy is at distance exactly 0 from its original, so after
    three picks nothing has weight, wherever the copies lie"""
    distinct = np.zeros((3, 128), np.float32)
    distinct[0, 0], distinct[1, 1], distinct[2, 2] = 2.0, 3.0, 0.5
    own = np.random.default_rng(37).permutation(np.repeat(np.arange(3), 40))
    rows = distinct[own]
    one, many = table_of(rows), sharded_of(rows, *layout)
    got = same_seeding(one, many, 8, 2, what="copies")
    picks = got["rows"].tolist()
    assert sorted(own[picks[:3]].tolist()) == [0, 1, 2]
    rest = [p for p in range(120) if p not in picks[:3]]
    assert picks[3:] == rest[:5] and got["potential"] == 0.0
    assert many.kmeans_seed_stats()["fallbacks"] == 5
    one.close()
    many.close()


def test_fallbacks_pass_from_shard_to_shard_and_back(built):
    """200 copies of the same three rows on (2, 64) with C = 150: after three picks the 147 fallbacks run through block 0
    (shard 0), block 1 (shard 1) and on into block 2 (shard 0 again), so the lowest-unpicked word changes owner twice"""
    distinct = np.zeros((3, 128), np.float32)
    distinct[0, 0], distinct[1, 1], distinct[2, 2] = 2.0, 3.0, 0.5
    own = np.random.default_rng(37).permutation(np.arange(200) % 3)
    rows = distinct[own]
    one, many = table_of(rows), sharded_of(rows, 2, 64)
    got = same_seeding(one, many, 150, 2, what="copies, C = 150")
    picks = got["rows"].tolist()
    assert sorted(own[picks[:3]].tolist()) == [0, 1, 2]
    rest = [p for p in range(200) if p not in picks[:3]]
    assert picks[3:] == rest[:147] and got["potential"] == 0.0
    owners = [(p // 64) % 2 for p in picks[3:]]
    changes = [o for i, o in enumerate(owners) if i == 0 or o != owners[i - 1]]
    assert changes == [0, 1, 0], changes
    assert many.kmeans_seed_stats()["fallbacks"] == 147
    one.close()
    many.close()


# ---- 7: rows that cannot be drawn -----------------------------------------------------------------------------------------

def test_unusable_rows_are_picked_only_as_fallbacks(built):
    rows = gaussian(38, 200, 128)
    rows[0] = 0.0
    rows[70, 3] = np.nan
    rows[150, 2] = np.inf
    bad = {0, 70, 150}                                            # one on each shard of (3, 64)
    one, many = table_of(rows), sharded_of(rows, 3, 64)
    for seed in range(3):
        got = same_seeding(one, many, 20, seed, what="unusable rows")
        assert not bad & set(got["rows"].tolist()) and many.kmeans_seed_stats()["fallbacks"] == 0
    got = same_seeding(one, many, 200, 4, what="C = S")
    picks = got["rows"].tolist()
    assert picks[0] not in bad and picks[197:] == [0, 70, 150] and many.kmeans_seed_stats()["fallbacks"] == 3
    one.close()
    many.close()


# ---- 8: the same bits every time -----------------------------------------------------------------------------------------

def test_same_bits_across_calls_and_handles(ragged):
    rows, _, _, _ = ragged
    t = ragged_layout(ragged, (4, 64))
    a = t.kmeans_seed(16, 9)
    fresh = sharded_of(rows, 4, 64)
    others = [t.kmeans_seed(16, 9), fresh.kmeans_seed(16, 9)]
    fresh.close()
    for b in others:
        assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(bits(a["centroids"]), bits(b["centroids"]))
        assert f64_bits(a["potential"]) == f64_bits(b["potential"])
    assert not np.array_equal(a["rows"], t.kmeans_seed(16, 10)["rows"])


# ---- 9: end to end ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1])
def test_kmeans_seeded_equals_one_table_from_kmeans_plus_plus(built, seed):
    rows, _ = planted_unequal()
    one, many = table_of(rows), sharded_of(rows, 3, 64)
    want = one.kmeans(16, seed=seed, init="kmeans++", fixed_sum=True)
    got = many.kmeans_seeded(16, seed=seed)
    print(f"seed {seed}: objective {got['objective']:.3f} after {got['iters']} iterations")
    assert np.array_equal(bits(got["centroids"]), bits(want["centroids"]))
    assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(bits(got["dist"]), bits(want["dist"]))
    assert got["iters"] == want["iters"] and f64_bits(got["objective"]) == f64_bits(want["objective"])
    # a sample smaller than the table: the seeded subset of the one-table rule
    want = one.kmeans(16, seed=seed, init="kmeans++", sample=500, fixed_sum=True)
    got = many.kmeans_seeded(16, seed=seed, sample=500)
    assert many.kmeans_seed_stats()["candidates"] == 500
    assert np.array_equal(bits(got["centroids"]), bits(want["centroids"])) and np.array_equal(got["labels"], want["labels"])
    assert f64_bits(got["objective"]) == f64_bits(want["objective"])
    with pytest.raises(ValueError, match="across shards"):
        many.kmeans(16, init="kmeans++")
    one.close()
    many.close()
