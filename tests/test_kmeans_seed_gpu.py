"""mi_knn_kmeans_seed on the GPU: k-means++ seeding, compared TO THE BIT with the numpy restatement of the contract
(tests/test_kmeans_seed_host.py) fed by the CPU oracle's distances: the picked rows in pick order, the centroids, the
potential (equality of the double) and the count of fallback picks.  There is no tolerance anywhere in this file."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable, initial_centroid_rows
from test_kmeans_seed_host import oracle_dist_from, planted_unequal, restate_seed

pytestmark = pytest.mark.gpu

MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f64_bits(x):
    return np.float64(x).view(np.uint64)


def gaussian(seed, n, dim):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    return rows * rng.uniform(0.1, 10.0, (n, 1)).astype(np.float32)


def table_of(rows, base=0):
    t = EmbeddingTable(rows.shape[1], 0, base)
    t.insert(rows)
    return t


def check_seeding(t, C, seed, cand_rows, cand_ids, oracle, among=None, what=""):
    """kmeans_seed(C, seed, among) == the restatement over the candidates (cand_rows under the ids cand_ids, ascending)"""
    dist_from, usable = oracle
    picks, potential, fallbacks = restate_seed(cand_rows.shape[0], C, seed, dist_from, usable)
    got = t.kmeans_seed(C, seed, among)
    st = t.kmeans_seed_stats()
    print(f"{what} C {C} seed {seed}: potential {got['potential']:.6f} (want {potential:.6f}), stats {st}")
    assert got["rows"].tolist() == [int(cand_ids[p]) for p in picks], what
    assert np.array_equal(bits(got["centroids"]), bits(cand_rows[picks])), what
    assert f64_bits(got["potential"]) == f64_bits(potential), (what, got["potential"], potential)
    assert st == {"candidates": cand_rows.shape[0], "passes": C + 1, "fallbacks": fallbacks}, (what, st)
    return got, picks, fallbacks


def rc_of(t, C, seed=0, among=None, n_among=0, rows=True):
    out = np.zeros(max(C, 1), np.uint64)
    return _lib.lib().mi_knn_kmeans_seed(t._h, C, seed, among, n_among, out.ctypes.data if rows else None, None, None)


# ---- 1: ragged against the 16-lane groups and the chunk ------------------------------------------------------------------

@pytest.fixture(scope="module")
def ragged(built, orc):
    rows = gaussian(31, 3001, 768)
    t = table_of(rows)
    yield rows, t, oracle_dist_from(orc, rows)
    t.close()


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("C", [1, 2, 16, 64])
def test_gaussian_rows_equal_the_restatement(ragged, C, seed):
    rows, t, oracle = ragged
    check_seeding(t, C, seed, rows, np.arange(rows.shape[0]), oracle, what="dim 768")


# ---- 2: the shortest and the longest row ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [128, 1024])
def test_other_dims(built, orc, dim):
    rows = gaussian(32 + dim, 300, dim)
    t = table_of(rows)
    check_seeding(t, 8, 1, rows, np.arange(300), oracle_dist_from(orc, rows), what=f"dim {dim}")
    t.close()


# ---- 3: among ---------------------------------------------------------------------------------------------------------------

def test_among(built, orc):
    rng = np.random.default_rng(33)
    rows = gaussian(34, 800, 128)
    t = table_of(rows)
    ids = rng.integers(0, 800, 500).astype(np.uint64)          # unsorted, with duplicates
    assert np.unique(ids).size < ids.size
    dead = np.union1d(np.unique(ids)[::9], np.array([1, 2, 3], np.uint64))   # deleted rows among them (and beside them)
    t.delete(dead)
    cand = np.setdiff1d(np.unique(ids), dead)
    assert cand.size < np.unique(ids).size
    oracle = oracle_dist_from(orc, rows[cand.astype(np.int64)])
    for C, seed in ((1, 0), (12, 5), (40, 6)):
        check_seeding(t, C, seed, rows[cand.astype(np.int64)], cand, oracle, among=ids, what="among")
    beyond = np.append(ids, np.uint64(800))
    assert rc_of(t, 4, among=beyond.ctypes.data, n_among=beyond.size) == MI_ERR_INVALID
    assert b"not a row" in _lib.lib().mi_last_error()
    assert rc_of(t, 1, among=ids.ctypes.data, n_among=0) == MI_ERR_INVALID
    with pytest.raises(_lib.MiError):
        t.kmeans_seed(1, 0, among=[])
    assert rc_of(t, 1, among=None, n_among=3) == MI_ERR_INVALID
    t.close()


# ---- 4: deletions, before and after an append, ids from 2^40 ------------------------------------------------------------------

def test_deleted_rows_are_never_picked(built, orc):
    base = 1 << 40
    rng = np.random.default_rng(35)
    rows = gaussian(36, 900, 128)
    t = table_of(rows[:600], base)
    dead = rng.choice(600, 60, replace=False)
    t.delete(dead.astype(np.uint64) + np.uint64(base))
    live = np.setdiff1d(np.arange(600), dead)
    for n, more_dead in ((600, None), (900, rng.choice(np.arange(600, 900), 30, replace=False))):
        if more_dead is not None:
            t.insert(rows[600:900])
            t.delete(more_dead.astype(np.uint64) + np.uint64(base))
            live = np.setdiff1d(np.arange(900), np.concatenate([dead, more_dead]))
        ids = live.astype(np.uint64) + np.uint64(base)
        got, picks, _ = check_seeding(t, 24, 7, rows[live], ids, oracle_dist_from(orc, rows[live]), what=f"{n} rows, deleted")
        assert np.all(np.isin(got["rows"], ids))
        fresh = table_of(rows[live])                       # a table that holds only the live rows: position = id
        same = fresh.kmeans_seed(24, 7)
        fresh.close()
        assert np.array_equal(ids[same["rows"].astype(np.int64)], got["rows"])
        assert np.array_equal(bits(same["centroids"]), bits(got["centroids"]))
        assert f64_bits(same["potential"]) == f64_bits(got["potential"])
    t.close()


# ---- 5: degenerate corpora and the errors -----------------------------------------------------------------------------------

def test_copies_fall_back_to_the_lowest_unpicked_positions(built, orc):
    """40 copies each of 3 distinct rows whose squared norms (4, 9, 1/4) and their roots are exact in fp32: a copy is at
    distance exactly 0 from its original, so after three picks nothing has weight"""
    distinct = np.zeros((3, 128), np.float32)
    distinct[0, 0], distinct[1, 1], distinct[2, 2] = 2.0, 3.0, 0.5
    own = np.random.default_rng(37).permutation(np.repeat(np.arange(3), 40))
    rows = distinct[own]
    t = table_of(rows)
    got, picks, fallbacks = check_seeding(t, 8, 2, rows, np.arange(120), oracle_dist_from(orc, rows), what="copies")
    assert sorted(own[picks[:3]].tolist()) == [0, 1, 2]
    rest = [p for p in range(120) if p not in picks[:3]]
    assert picks[3:] == rest[:5] and fallbacks == 5 and got["potential"] == 0.0
    assert t.kmeans_seed_stats()["fallbacks"] == 5
    t.close()


def test_unusable_rows_and_the_errors(built, orc):
    rows = gaussian(38, 60, 128)
    rows[0] = 0.0
    rows[5, 3] = np.nan
    rows[7, 2] = np.inf
    bad = {0, 5, 7}
    t = table_of(rows)
    oracle = oracle_dist_from(orc, rows)
    assert set(np.flatnonzero(~oracle[1]).tolist()) == bad
    for seed in range(3):
        got, picks, fallbacks = check_seeding(t, 20, seed, rows, np.arange(60), oracle, what="unusable rows")
        assert not bad & set(picks) and fallbacks == 0
    # C = S: the unusable rows come last, as fallback picks, once no usable candidate is left
    got, picks, fallbacks = check_seeding(t, 60, 4, rows, np.arange(60), oracle, what="C = S")
    assert picks[0] not in bad and picks[57:] == [0, 5, 7] and fallbacks == 3
    assert rc_of(t, 61) == MI_ERR_INVALID                        # C > S
    assert rc_of(t, 0) == MI_ERR_INVALID
    assert rc_of(t, 4, rows=False) == MI_ERR_INVALID
    assert rc_of(t, 65537) == MI_ERR_UNSUPPORTED
    t.close()
    st = ShardedTable(128, [0, 0], 64)
    st.insert(rows)
    shard = EmbeddingTable.__new__(EmbeddingTable)               # a shard borrowed from the sharded table
    shard._h, shard.dim = ctypes.c_void_p(_lib.lib().mi_knn_sharded_shard(st._h, 0)), 128
    assert rc_of(shard, 4) == MI_ERR_UNSUPPORTED
    shard._h = ctypes.c_void_p()
    st.close()


# ---- 6: the same bits every time -----------------------------------------------------------------------------------------

def test_same_bits_across_calls_handles_and_prefilter(ragged):
    rows, t, _ = ragged
    a = t.kmeans_seed(16, 9)
    others = [t.kmeans_seed(16, 9)]
    for prefilter in (0, 1, 2):
        t2 = table_of(rows)
        t2.set_option("prefilter", prefilter)
        if prefilter:
            t2.knn(rows[0], 10)                                  # (the mirror exists)
        others.append(t2.kmeans_seed(16, 9))
        t2.close()
    for b in others:
        assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(bits(a["centroids"]), bits(b["centroids"]))
        assert f64_bits(a["potential"]) == f64_bits(b["potential"])
    assert not np.array_equal(a["rows"], t.kmeans_seed(16, 10)["rows"])


# ---- 7: end to end ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted_table(built):
    rows, own = planted_unequal()
    t = table_of(rows)
    yield rows, own, t
    t.close()


@pytest.mark.parametrize("seed", range(4))
def test_kmeans_from_the_seeds_beats_the_uniform_start(planted_table, seed):
    """Checked first on the CPU (a float64 Lloyd, 20 iterations, from the restatement's seeds and from the uniform rows):
    objective from k-means++ 18.75, 31.71, 6.16, 32.01 for seeds 0 .. 3 against 91.27, 159.67, 104.14, 141.01 from the
    uniform start.  The gap (72.5 at the least) is more than eleven times the within-cluster total (6.16, what seed 2
    reaches with every planted cluster covered), so all four seeds stay in the list."""
    rows, own, t = planted_table
    pp = t.kmeans(16, seed=seed, init="kmeans++")
    uni = t.kmeans(16, seed=seed)
    print(f"seed {seed}: objective {pp['objective']:.3f} from k-means++, {uni['objective']:.3f} from the uniform start")
    assert pp["objective"] < uni["objective"]
    lab, d = t.assign(pp["centroids"])
    assert np.array_equal(lab, pp["labels"]) and np.array_equal(bits(d), bits(pp["dist"]))
    # the default is unchanged: the rows initial_centroid_rows picks, bit for bit
    start = rows[initial_centroid_rows(rows.shape[0], [], 16, seed).astype(np.int64)]
    same = t.kmeans(start.copy())
    assert np.array_equal(bits(same["centroids"]), bits(uni["centroids"])) and np.array_equal(same["labels"], uni["labels"])
    assert np.array_equal(bits(same["dist"]), bits(uni["dist"])) and f64_bits(same["objective"]) == f64_bits(uni["objective"])
    # fewer live rows than the default sample: the seeds are kmeans_seed's over every live row
    assert np.array_equal(bits(t.kmeans(16, max_iters=0, seed=seed, init="kmeans++")["centroids"]),
                          bits(t.kmeans_seed(16, seed)["centroids"]))


def test_kmeans_sample_and_image_index(planted_table):
    rows, own, t = planted_table
    among = np.sort(np.random.default_rng(3).choice(np.arange(rows.shape[0], dtype=np.uint64), size=500, replace=False))
    a = t.kmeans(16, max_iters=0, seed=3, init="kmeans++", sample=500)
    assert np.array_equal(bits(a["centroids"]), bits(t.kmeans_seed(16, 3, among)["centroids"]))
    assert t.kmeans_seed_stats()["candidates"] == 500
    paths = [f"/media/p{r}.jpg" for r in range(200)]
    ix = ImageIndex(256, 0, "/media")
    ix.insert(paths, rows[:200])
    groups = ix.clusters(4, seed=1, init="kmeans++")
    assert sorted(p for g in groups for p in g) == sorted(paths) and len(groups) >= 2
    ix.close()
