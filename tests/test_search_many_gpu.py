"""mi_knn_search_many / mi_knn_neighbors / mi_knn_sharded_search_many on the GPU: for each of many queries the entries of
knn(query, k) without those whose distance is NaN — the same ids and the same distance bits, NO_ID / +inf behind them; for
neighbors the same with k + 1 and the row's own entry removed.  Oracle: orc_cosine_dist(query, rows) (oracle.c) followed by
the search's order (distance key ascending, then id, NaN last), as tests/test_assign_multi_gpu.py whose planted corpus is
re-created here.  Ids are compared for equality and distances on their bits: there is no tolerance anywhere in this file."""
import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable, drop_self
from oracle.binding import orc_cosine_dist

pytestmark = pytest.mark.gpu

DIM = 768
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
NO_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
N_PLANTED, N_CLUSTERS = 3072, 16
N_ROWS, N_QUERIES = 4133, 300   # 32 full column tiles + a ragged one; two full query tiles + a ragged one


def planted_corpus(seed=11):
    """tests/test_assign_multi_gpu.py's: 4 096 rows, 3 072 = vectors[i % 16] + sigma x noise (sigma 0.1 .. 1.5) under row
    scales 0.1 .. 10, then 1 024 plain Gaussian rows; and 1 024 Gaussian vectors"""
    rng = np.random.default_rng(seed)
    vectors = rng.standard_normal((1024, DIM)).astype(np.float32)
    sigma = rng.uniform(0.1, 1.5, N_PLANTED)
    scale = rng.uniform(0.1, 10.0, N_PLANTED)
    own = np.arange(N_PLANTED) % N_CLUSTERS
    planted = (vectors[own] + sigma[:, None] * rng.standard_normal((N_PLANTED, DIM))) * scale[:, None]
    rows = np.concatenate([planted.astype(np.float32), rng.standard_normal((1024, DIM)).astype(np.float32)])
    return rows, vectors, own


def corpus_and_queries():
    """(rows [4133, 768], queries [300, 768]): the planted corpus + 37 Gaussian rows, in a seeded random order; the planted
    corpus' first 16 centre vectors, then 284 Gaussian queries.  Why shuffled: the planted corpus puts cluster c at the rows
    r with r % 16 == c, so for every m that divides 16 all of a centre's near rows share ONE residue slot of stage 1 and its
    threshold comes from the unrelated rows alone — tests/test_search_many_host.py's emulation counted 826 candidates for the
    first centre at k = 16 on the unshuffled rows, beyond the eighth of the table that test 1 allows."""
    rows, vectors, _ = planted_corpus()
    rng = np.random.default_rng(21)
    rows = np.concatenate([rows, rng.standard_normal((N_ROWS - rows.shape[0], DIM)).astype(np.float32)])
    rows = rows[rng.permutation(N_ROWS)]
    queries = np.concatenate([vectors[:N_CLUSTERS], rng.standard_normal((N_QUERIES - N_CLUSTERS, DIM)).astype(np.float32)])
    return rows, queries


def dist_keys(d):
    """the search's 32-bit distance key (knn_kernels.h dist_to_u32): ascending key = ascending distance, NaN last"""
    b = np.ascontiguousarray(d, np.float32).view(np.uint32)
    k = np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))
    return np.where(np.isnan(d), np.uint32(0xFFFFFFFF), k)


def oracle_matrix(orc, queries, rows):
    return np.stack([orc_cosine_dist(orc, queries[q], rows) for q in range(queries.shape[0])])


def oracle_many(D, k, live=None, base=0):
    """the first k of every row of D under the search's order, the deleted columns and the NaN distances left out (they
    are last: a suffix); ids = base + column"""
    D = np.array(D, np.float32)
    if live is not None:
        D[:, ~live] = np.nan
    nq, n = D.shape
    key = (dist_keys(D).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    d = np.take_along_axis(D, order, axis=1)
    ok = ~np.isnan(d)
    idx = np.full((nq, k), NO_ID, np.uint64)
    dd = np.full((nq, k), np.inf, np.float32)
    idx[:, :order.shape[1]] = np.where(ok, order.astype(np.uint64) + np.uint64(base), NO_ID)
    dd[:, :order.shape[1]] = np.where(ok, d, np.float32(np.inf))
    return idx, dd


def strip_nan(idx, dist):
    """knn()'s lists without their NaN entries (they are last), padded"""
    idx, dist = idx.copy(), dist.copy()
    bad = np.isnan(dist)
    idx[bad], dist[bad] = NO_ID, np.inf
    return idx, dist


def same(got, want, what=""):
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:8])
    assert not np.any(np.isnan(gd)), what
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what


@pytest.fixture(scope="module")
def corpus(built, orc):
    rows, queries = corpus_and_queries()
    return rows, queries, oracle_matrix(orc, queries, rows)


@pytest.fixture(scope="module")
def table(corpus):
    t = EmbeddingTable(DIM, 0)
    t.insert(corpus[0])
    yield t
    t.close()


@pytest.fixture(scope="module")
def self_matrix(corpus, orc):
    """the corpus' first 300 rows as queries against the corpus"""
    rows = corpus[0]
    return oracle_matrix(orc, rows[:300], rows)


# 1: the corpus against the oracle; stage 1 really filters
@pytest.mark.parametrize("k", [1, 4, 16])
@pytest.mark.parametrize("nq", [1, 127, 129, 300])
def test_equals_the_oracle(corpus, table, nq, k):
    rows, queries, D = corpus
    want = oracle_many(D[:nq], k)
    got = table.knn_many(queries[:nq], k)
    st = table.search_many_stats()
    print(f"nq {nq} k {k}: stats {st}, {st['candidates'] / nq:.1f} candidates per query ({st['candidates'] / (nq * N_ROWS):.4f} of all pairs)")
    same(got, want, f"nq {nq} k {k}")
    assert st["hits"] == int(np.sum(want[0] != NO_ID)) == nq * k
    # a stage 1 that passes everything must not hide behind a correct stage 2
    assert st["hits"] <= st["candidates"] <= nq * N_ROWS // 8, st
    assert st["launches"] >= 2 and st["tiles"] >= 2 * 33 * ((nq + 127) // 128)


@pytest.mark.parametrize("k", [4, 16])
def test_equals_a_loop_of_searches(corpus, table, k):
    rows, queries, D = corpus
    got = table.knn_many(queries, k)
    for q0 in range(0, N_QUERIES, 16):
        same((got[0][q0:q0 + 16], got[1][q0:q0 + 16]), strip_nan(*table.knn(queries[q0:q0 + 16], k)), f"queries from {q0}")


# 2: the segments and the sampled threshold pass change nothing
def test_segments_and_sampling_give_identical_results(corpus):
    rows, queries, D = corpus
    want = oracle_many(D[:129], 4)
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    seen = []
    for segments, sample in ((1, 1), (2, 1), (5, 1), (33, 1), (1000, 1), (5, 2), (5, 8), (1, 33), (0, 0)):
        t.set_option("many_segments", segments)
        t.set_option("many_sample", sample)
        same(t.knn_many(queries[:129], 4), want, f"segments {segments} sample {sample}")
        seen.append(t.search_many_stats())
        print(f"segments {segments} sample {sample}: {seen[-1]}")
    # the threshold pass of a sparser sample visits fewer tiles and hands over more candidates
    assert seen[6]["tiles"] < seen[5]["tiles"] < seen[2]["tiles"]
    assert seen[2]["candidates"] <= seen[5]["candidates"] <= seen[6]["candidates"] <= seen[7]["candidates"]
    with pytest.raises(RuntimeError):
        t.set_option("many_segments", -1)
    t.close()


# 3: bounded memory — the buffer at its floor, 300 x 600 pairs that no threshold can separate
def test_overflow_pieces(built, orc):
    rng = np.random.default_rng(7)
    v = rng.standard_normal(DIM).astype(np.float32)
    t = EmbeddingTable(DIM, 0)
    t.insert(np.concatenate([np.tile(v, (600, 1)), rng.standard_normal((400, DIM)).astype(np.float32)]))
    t.set_option("join_cap", 1 << 14)
    k = 4
    idx, d = t.knn_many(np.tile(v, (300, 1)), k)
    st = t.search_many_stats()
    print("300 x 600 tied pairs:", st)
    want = orc_cosine_dist(orc, v, v[None, :])[0]
    assert np.array_equal(idx, np.tile(np.arange(k, dtype=np.uint64), (300, 1)))
    assert np.all(d.view(np.uint32) == np.float32(want).view(np.uint32))
    assert st["launches"] > 2 and st["candidates"] >= 300 * 600 and st["hits"] == 300 * k
    t.close()


# 4: ties and specials
def test_ties_and_specials(built, orc):
    rng = np.random.default_rng(4)
    rows = rng.standard_normal((300, DIM)).astype(np.float32)
    rows[40] = rows[20]                  # identical rows: the lower id first
    rows[7] = 0.0                        # a zero-norm row and a NaN-holding row are never returned
    rows[9, 5] = np.nan
    rows[11, 3] = 3.2e38                 # marked by the mirror (an element > 3e38)
    rows[13] *= np.float32(1e-17)        # marked: norm^2 below 1e-30
    queries = rng.standard_normal((20, DIM)).astype(np.float32)
    queries[0] = rows[20] * np.float32(2.0)
    queries[1] = 0.0                     # a zero-norm query: only padding
    queries[2] = rows[13]                # a marked query
    queries[3, 0] = np.inf
    D = oracle_matrix(orc, queries, rows)
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    for k in (1, 4, 16):
        got = t.knn_many(queries, k)
        same(got, oracle_many(D, k), f"specials k {k}")
        same(got, strip_nan(*t.knn(queries, k)), f"specials against knn, k {k}")
        assert not np.any(np.isin(got[0], (7, 9)))
        assert np.all(got[0][1] == NO_ID) and np.all(np.isposinf(got[1][1]))
    idx, d = t.knn_many(queries, 4)
    assert idx[0, 0] == 20 and idx[0, 1] == 40 and d[0, 0].view(np.uint32) == d[0, 1].view(np.uint32)
    t.close()
    # k = 16 on a table of 5 live rows: 5 hits, then padding
    t = EmbeddingTable(DIM, 0)
    t.insert(rows[100:108])
    t.delete([1, 4, 6])
    live = np.ones(8, bool)
    live[[1, 4, 6]] = False
    got = t.knn_many(queries[4:9], 16)
    same(got, oracle_many(D[4:9, 100:108], 16, live), "5 live rows")
    assert np.all(np.sum(got[0] != NO_ID, axis=1) == 5) and np.all(got[0][:, 5:] == NO_ID) and np.all(np.isposinf(got[1][:, 5:]))
    t.close()


# 5: deleted rows are left out, before and after more appends; every mirror route gives the same bits
def test_deleted_rows_appends_and_mirror_routes(corpus):
    rows, queries, D = corpus
    k = 4
    dead = np.unique(np.random.default_rng(6).integers(0, 3000, 300))
    dead = np.union1d(dead, oracle_many(D[:40], 2)[0].reshape(-1).astype(np.int64))   # the nearest rows of 40 queries among them
    dead = dead[dead < 3000]
    live = np.ones(N_ROWS, bool)
    live[dead] = False
    results = []
    for prefilter in (0, 1, 2):
        t = EmbeddingTable(DIM, 0)
        t.insert(rows[:3000])
        if prefilter:
            t.set_option("prefilter", prefilter)
        t.delete(dead)
        got = t.knn_many(queries, k)
        same(got, oracle_many(D[:, :3000], k, live[:3000]), f"deleted, prefilter {prefilter}")
        assert not np.any(np.isin(got[0], dead.astype(np.uint64)))
        t.insert(rows[3000:])   # (with "prefilter" = 1 the table's mirror catches up)
        got = t.knn_many(queries, k)
        same(got, oracle_many(D, k, live), f"deleted + appended, prefilter {prefilter}")
        assert t.search_many_stats()["hits"] == N_QUERIES * k
        nb = t.neighbors(3, 2900, 200)
        results.append(got + nb)
        t.close()
    for got in results[1:]:
        for a, b in zip(got, results[0]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# 6: ids carry the base
def test_ids_carry_the_base(corpus, self_matrix):
    rows, queries, D = corpus
    base = 1 << 40
    t = EmbeddingTable(DIM, 0, base=base)
    t.insert(rows[:300])
    same(t.knn_many(queries[:40], 4), oracle_many(D[:40, :300], 4, base=base), "base")
    want = drop_self(*oracle_many(self_matrix[:300, :300], 4, base=base), np.arange(300, dtype=np.uint64) + np.uint64(base))
    same(t.neighbors(3, first=base), want, "neighbors with a base")
    same(t.neighbors(3, first=base + 100, n=50), (want[0][100:150], want[1][100:150]), "a slice with a base")
    mi = _lib.lib()
    idx, d = np.zeros((4, 3), np.uint64), np.zeros((4, 3), np.float32)
    assert mi.mi_knn_neighbors(t._h, 0, 4, 3, idx.ctypes.data, d.ctypes.data) == MI_ERR_INVALID   # ids below the base
    t.close()


# 7: the kNN graph
@pytest.mark.parametrize("k", [1, 5, 15])
def test_neighbors_equal_searches_minus_self(corpus, table, self_matrix, k):
    rows = corpus[0]
    got = table.neighbors(k, 0, 256)
    ids = np.arange(256, dtype=np.uint64)
    same(got, drop_self(*oracle_many(self_matrix[:256], k + 1), ids), f"neighbors k {k} against the oracle")
    knn = [table.knn(rows[r0:r0 + 16], k + 1) for r0 in range(0, 256, 16)]
    same(got, drop_self(*strip_nan(np.concatenate([a for a, _ in knn]), np.concatenate([b for _, b in knn])), ids), f"neighbors k {k} against knn")
    assert not np.any(got[0] == ids[:, None])


def test_neighbors_slices_ends_and_errors(corpus, table, self_matrix):
    rows = corpus[0]
    k = 5
    whole = table.neighbors(k)
    ids = np.arange(N_ROWS, dtype=np.uint64)
    same((whole[0][:300], whole[1][:300]), drop_self(*oracle_many(self_matrix, k + 1), ids[:300]), "the graph's first rows")
    knn = [table.knn(rows[r0:r0 + 16], k + 1) for r0 in range(0, N_ROWS, 16)]   # (no distance of this corpus is NaN)
    same(whole, drop_self(np.concatenate([a for a, _ in knn]), np.concatenate([b for _, b in knn]), ids), "the whole graph")
    a, b = table.neighbors(k, 0, 2000), table.neighbors(k, 2000, 2133)
    same((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), whole, "two slices")
    tail = table.neighbors(k, N_ROWS - 7, 7)   # first + n at the table's end
    same(tail, (whole[0][-7:], whole[1][-7:]), "the last rows")
    same(table.neighbors(k, N_ROWS - 7), tail, "n = None")
    e = table.neighbors(k, 100, 0)
    assert e[0].shape == (0, k) and e[1].shape == (0, k)
    mi = _lib.lib()
    idx, d = np.full((8, k), 7, np.uint64), np.full((8, k), 7.0, np.float32)
    assert mi.mi_knn_neighbors(table._h, N_ROWS, 0, k, None, None) == 0             # n = 0 succeeds, also at the end
    for first, n in ((N_ROWS + 1, 0), (N_ROWS, 1), (N_ROWS - 3, 8), (1 << 50, 1)):   # outside the table: nothing runs
        assert mi.mi_knn_neighbors(table._h, first, n, k, idx.ctypes.data, d.ctypes.data) == MI_ERR_INVALID, (first, n)
        assert len(mi.mi_last_error()) > 0
    assert np.all(idx == 7) and np.all(d == 7.0)


def test_neighbors_copies_at_lower_ids_and_deleted_rows(built, orc):
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((200, DIM)).astype(np.float32)
    rows[11] = rows[12] = rows[13] = rows[10]   # row 13 has 3 exact copies at lower ids
    rows[30] = 0.0                              # every distance NaN: only padding
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    t.delete([50, 10 + 100])
    live = np.ones(200, bool)
    live[[50, 110]] = False
    S = oracle_matrix(orc, rows, rows)
    ids = np.arange(200, dtype=np.uint64)
    for k in (2, 15):
        want = drop_self(*oracle_many(S, k + 1, live), ids)
        want[0][~live], want[1][~live] = NO_ID, np.inf
        got = t.neighbors(k)
        same(got, want, f"copies and deleted rows, k {k}")
    idx, d = t.neighbors(2)
    assert idx[13].tolist() == [10, 11]         # self absent among its first 3: the last entry went
    assert idx[10].tolist() == [11, 12] and idx[12].tolist() == [10, 11]
    assert np.all(idx[[50, 110, 30]] == NO_ID) and np.all(np.isposinf(d[[50, 110, 30]]))
    assert not np.any(np.isin(idx, (50, 110, 30)))
    t.close()


# 8: the errors
def test_errors(corpus, table):
    rows, queries, D = corpus
    mi = _lib.lib()
    idx, d = np.full((4, 17), 7, np.uint64), np.full((4, 17), 7.0, np.float32)
    q = queries.ctypes.data

    def err(rc, code):
        assert rc == code
        assert len(mi.mi_last_error()) > 0

    err(mi.mi_knn_search_many(table._h, q, 4, 17, idx.ctypes.data, d.ctypes.data), MI_ERR_UNSUPPORTED)
    err(mi.mi_knn_search_many(table._h, q, 4, 0, idx.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_search_many(table._h, q, 0, 4, idx.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_search_many(table._h, None, 4, 4, idx.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_search_many(table._h, q, 4, 4, None, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_search_many(table._h, q, 4, 4, idx.ctypes.data, None), MI_ERR_INVALID)
    err(mi.mi_knn_neighbors(table._h, 0, 4, 16, idx.ctypes.data, d.ctypes.data), MI_ERR_UNSUPPORTED)
    err(mi.mi_knn_neighbors(table._h, 0, 4, 0, idx.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_neighbors(table._h, 0, 4, 4, None, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_search_many_stats(table._h, None), MI_ERR_INVALID)
    odd = EmbeddingTable(192, 0)
    odd.insert(np.ones((4, 192), np.float32))
    err(mi.mi_knn_search_many(odd._h, q, 4, 4, idx.ctypes.data, d.ctypes.data), MI_ERR_UNSUPPORTED)
    odd.close()
    assert np.all(idx == 7) and np.all(d == 7.0)   # no error wrote anything
    empty = EmbeddingTable(DIM, 0)                  # an empty table: all padding
    i2, d2 = empty.knn_many(queries[:3], 4)
    assert np.all(i2 == NO_ID) and np.all(np.isposinf(d2))
    assert empty.neighbors(4)[0].shape == (0, 4)
    empty.close()


# 9: two shards on one device
def test_sharded_equals_the_single_table(corpus, table):
    rows, queries, D = corpus
    st = ShardedTable(DIM, (0, 0), 64)
    st.insert(rows)
    for k in (1, 16):
        same(st.knn_many(queries, k), table.knn_many(queries, k), f"sharded k {k}")
    same(st.neighbors(5, 1000, 300), table.neighbors(5, 1000, 300), "sharded neighbors")
    same(st.neighbors(5, N_ROWS - 33), table.neighbors(5, N_ROWS - 33), "sharded neighbors to the end")
    # rows of the second shard (blocks 1, 3, ...) deleted through the sharded handle, the nearest rows of the first queries among them
    near = oracle_many(D[:60], 4)[0].reshape(-1)
    dead = np.unique(near[(near // np.uint64(64)) % np.uint64(2) == 1]).astype(np.int64)
    assert dead.size >= 20
    st.delete(dead)
    live = np.ones(N_ROWS, bool)
    live[dead] = False
    got = st.knn_many(queries, 4)
    same(got, oracle_many(D, 4, live), "sharded, deleted")
    assert not np.any(np.isin(got[0], dead.astype(np.uint64)))
    nb = st.neighbors(3, int(dead[0]), 10)
    assert np.all(nb[0][0] == NO_ID) and np.all(np.isposinf(nb[1][0])) and not np.any(np.isin(nb[0], dead.astype(np.uint64)))
    st.close()


# 10: the index
def test_index_related_and_best_per_label(built):
    rng = np.random.default_rng(12)
    themes = rng.standard_normal((3, DIM)).astype(np.float32)
    names = ["dog", "receipt", "beach"]
    emb = (themes[np.arange(64) % 3] + 0.5 * rng.standard_normal((64, DIM))).astype(np.float32)
    paths = [f"/media/{'trip' if i % 2 else 'home'}/p{i}.jpg" for i in range(64)]
    ix = ImageIndex(DIM, 0, "/media")
    ix.insert(paths, emb)
    gone = [paths[5], paths[33]]
    ix.remove(gone)
    idx, dist = ix.table.neighbors(4)
    rel = ix.related(k=4)
    assert set(rel) == set(paths) - set(gone)
    for r, p in enumerate(paths):
        if p in gone:
            continue
        assert [q for q, _ in rel[p]] == [paths[int(i)] for i in idx[r]] and [d for _, d in rel[p]] == [float(x) for x in dist[r]]
        assert p not in [q for q, _ in rel[p]] and not set(gone) & set(q for q, _ in rel[p])
        assert all(int(i) % 3 == r % 3 for i in idx[r])   # the same theme
    bi, bd = ix.table.knn_many(themes, 6)
    best = ix.best_per_label(themes, names=names, k=6)
    assert list(best) == names
    for c, name in enumerate(names):
        assert [p for p, _ in best[name]] == [paths[int(i)] for i in bi[c]] and not set(gone) & set(p for p, _ in best[name])
        assert all(int(i) % 3 == c for i in bi[c]) and [d for _, d in best[name]] == sorted(d for _, d in best[name])
    assert list(ix.best_per_label(themes, k=2)) == [0, 1, 2]
    web = ix.related(k=2, web=True)
    assert all(p.startswith("media/") for p in web) and all(q.startswith("media/") for hits in web.values() for q, _ in hits)
    ix.close()
