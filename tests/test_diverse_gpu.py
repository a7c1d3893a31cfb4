"""mi_knn_search_diverse on the GPU: ids, distance bits, hidden counts, rep, n_kept and the hidden total for equality with the
numpy restatement (tests/test_diverse_host.py), which is fed by the CPU oracle alone: the pool is orc_knn's list and
G[a, b] = orc_cosine_dist(row a, rows)[b], read at (min, max)."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex
from oracle.binding import orc_cosine_dist, orc_knn, orc_refine
from test_diverse_host import NO_ID, NO_LABEL, distance_matrix, expected, planted_bursts, planted_queries

pytestmark = pytest.mark.gpu

MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5


def eps2(dim):
    return 2.0 ** -7 + 2.0 ** -16 + 4.1 * (dim + 8) * 2.0 ** -24 + 2e-6


def call(t, q, k, pool, gap, within=None):
    """the C call with every output -> (rc, idx, dist, hidden, rep, n_kept); the arrays keep a sentinel where nothing was written"""
    q = np.ascontiguousarray(q, np.float32)
    idx, dist = np.full(max(k, 1), 7, np.uint64), np.full(max(k, 1), -7.0, np.float32)
    hidden, rep = np.full(max(k, 1), 7, np.uint32), np.full(max(pool, 1), 7, np.uint32)
    n = ctypes.c_uint32(7)
    ids, n_ids = None, 0
    if within is not None:
        a = np.ascontiguousarray(within, np.uint64)
        n_ids = a.size
        ids = (a if a.size else np.zeros(1, np.uint64)).ctypes.data
    rc = _lib.lib().mi_knn_search_diverse(t._h, q.ctypes.data, k, pool, float(gap), ids, n_ids, idx.ctypes.data, dist.ctypes.data,
                                          hidden.ctypes.data, rep.ctypes.data, ctypes.byref(n))
    return rc, idx[:k], dist[:k], hidden[:k], rep[:pool], n.value


def oracle_pool(orc, q, rows, pool, ids=None):
    """the search's list of `pool` entries over `rows` (held under `ids`, default 0 .. n-1), padded"""
    n = rows.shape[0]
    idx, dist = np.full(pool, NO_ID, np.uint64), np.full(pool, np.inf, np.float32)
    if n:
        i, d = orc_knn(orc, q, rows, min(pool, n))
        idx[:i.size] = i if ids is None else np.asarray(ids, np.uint64)[i.astype(np.int64)]
        dist[:d.size] = d
    return idx, dist


def check(t, got, want, what=""):
    rc, idx, dist, hidden, rep, n_kept = got
    w_idx, w_dist, w_hidden, w_rep, w_n, w_nh = want
    assert rc == 0, (what, _lib.lib().mi_last_error())
    assert n_kept == w_n, (what, n_kept, w_n)
    assert np.array_equal(idx, w_idx), what
    assert np.array_equal(dist.view(np.uint32), w_dist.view(np.uint32)), what
    assert np.array_equal(hidden, w_hidden), what
    assert np.array_equal(rep, w_rep), what
    st = t.knn_diverse_stats()
    assert st["hidden"] == w_nh, (what, st, w_nh)
    return st


def pairs_within(G, coords, bound):
    s = np.sort(np.asarray(coords, np.int64))
    return int(np.count_nonzero(np.triu(G[np.ix_(s, s)] <= np.float32(bound), 1)))


@pytest.fixture(scope="module")
def corpus(built, orc):
    rows = planted_bursts()
    return rows, distance_matrix(orc, rows), planted_queries(rows)


@pytest.fixture(scope="module")
def table(corpus):
    t = EmbeddingTable(768, 0)
    t.insert(corpus[0])
    yield t
    t.close()


# P = 2304 is ragged against the 128-row tile (18 tile rows); 130 and 300 cross one and two tile edges and the 64-bit word edge
@pytest.mark.parametrize("pool,k,gap", [(4096, 2304, 0.05), (300, 50, 0.05), (1000, 100, 0.08), (130, 130, 0.02), (64, 1, 0.05),
                                        (1, 1, 0.05)])
def test_planted_corpus_equals_the_restatement_and_stage1_filters(orc, corpus, table, pool, k, gap):
    rows, G, queries = corpus
    for qi, q in enumerate(queries):
        ids, dists = oracle_pool(orc, q, rows, pool)
        want = expected(ids, dists, G, int, k, pool, gap)
        st = check(table, call(table, q, k, pool, gap), want, (pool, k, gap, qi))
        live = ids[ids != NO_ID].astype(np.int64)
        conflicts, in_band = pairs_within(G, live, gap), pairs_within(G, live, gap + 2 * eps2(768))
        print(f"pool {pool} k {k} gap {gap} query {qi}: kept {want[4]} hidden {want[5]} stats {st} conflicts {conflicts} band {in_band}")
        assert st["pool"] == live.size and st["conflicts"] == conflicts
        # a candidate has coarse <= gap + eps2 and |coarse - exact| <= eps2: a consequence of the bound, not a tuned number
        assert conflicts <= st["candidates"] <= in_band, (st, conflicts, in_band)
    if pool == 4096:
        assert want[5] >= 100 and in_band < 2304 * 2303 // 2 // 100   # bursts are hidden; stage 1 hands on under 1 % of the pairs


@pytest.mark.parametrize("dim", [128, 1024])
def test_other_dims(built, orc, dim):
    rng = np.random.default_rng(dim)
    rows = rng.standard_normal((300, dim)).astype(np.float32)
    rows[200:] = ((rows[:100] + rng.uniform(0.05, 0.4, (100, 1)) * rng.standard_normal((100, dim))) * rng.uniform(0.1, 10, (100, 1))).astype(np.float32)
    G = distance_matrix(orc, rows)
    t = EmbeddingTable(dim, 0)
    t.insert(rows)
    for q in (rows[250], rng.standard_normal(dim).astype(np.float32)):
        for pool, k, gap in ((300, 100, 0.05), (300, 300, 0.1), (150, 20, 0.05)):
            ids, dists = oracle_pool(orc, q, rows, pool)
            want = expected(ids, dists, G, int, k, pool, gap)
            check(t, call(t, q, k, pool, gap), want, (dim, pool, k, gap))
    assert want[5] > 0
    t.close()


def test_exact_copies(built, orc):
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((400, 768)).astype(np.float32)
    where = rng.choice(400, 200, replace=False)
    rows[where] = rows[where[0]]
    G = distance_matrix(orc, rows)
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    for q in (rows[where[0]], rng.standard_normal(768).astype(np.float32)):
        for gap in (0.0, 1e-6, np.inf):
            ids, dists = oracle_pool(orc, q, rows, 400)
            want = expected(ids, dists, G, int, 400, 400, gap)
            check(t, call(t, q, 400, 400, gap), want, gap)
            if gap == np.inf:
                assert want[4] == 1 and want[2][0] == 399
    assert want[5] >= 199
    t.close()


def test_4096_copies_overflow_the_smallest_buffer(built, orc):
    row = np.random.default_rng(4).standard_normal((1, 768)).astype(np.float32)
    g = orc_cosine_dist(orc, row[0], row)[0]
    assert g <= np.float32(0.01)
    t = EmbeddingTable(768, 0)
    t.insert(np.repeat(row, 4096, axis=0))
    t.set_option("join_cap", 1 << 14)   # a tile of copies fills the buffer: every strip overflows and is redone
    rc, idx, dist, hidden, rep, n_kept = call(t, row[0], 10, 4096, 0.01)
    assert rc == 0 and n_kept == 1 and idx[0] == 0 and hidden[0] == 4095
    assert np.all(idx[1:] == NO_ID) and np.all(np.isinf(dist[1:])) and not hidden[1:].any() and not rep.any()
    assert dist[0].view(np.uint32) == g.view(np.uint32)
    st = t.knn_diverse_stats()
    assert st == {"pool": 4096, "candidates": 4096 * 4095 // 2, "conflicts": 4096 * 4095 // 2, "hidden": 4095}
    t.close()


def test_unusable_rows_never_appear(built, orc):
    rows = planted_bursts()[1900:2304].copy()   # 404 rows, the bursts among them
    rows[5] = 0.0
    rows[130, 7] = np.nan
    rows[260, 700] = np.inf
    rows[399] = 0.0
    G = distance_matrix(orc, rows)
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    for q in (rows[200], rows[10]):
        ids, dists = oracle_pool(orc, q, rows, 404)
        want = expected(ids, dists, G, int, 404, 404, 0.05)
        got = call(t, q, 404, 404, 0.05)
        st = check(t, got, want)
        assert st["pool"] == 400 and want[4] + want[5] == 400
        assert not np.isin(got[1], [5, 130, 260, 399]).any() and np.all(got[4][400:] == NO_LABEL)
    t.close()


def test_deleted_rows_and_a_base(built, orc):
    base = 1 << 40
    rows = planted_bursts()[1700:2304]
    G = distance_matrix(orc, rows)
    rng = np.random.default_rng(5)
    t = EmbeddingTable(768, 0)
    t.set_base(base)
    t.insert(rows[:500])
    dead = rng.choice(500, 50, replace=False)
    t.delete((dead + base).astype(np.uint64))
    q = rows[480]
    for n in (500, 604):
        if n == 604:
            t.insert(rows[500:])
        live = np.setdiff1d(np.arange(n), dead)
        for pool, k, gap in ((604, 604, 0.05), (200, 30, 0.08)):
            ids, dists = oracle_pool(orc, q, rows[live], pool, ids=live + base)   # a table of the live rows under the same ids
            want = expected(ids, dists, G, lambda i: i - base, k, pool, gap)
            got = call(t, q, k, pool, gap)
            check(t, got, want, (n, pool))
            assert not np.isin(got[1], dead + base).any()
        assert want[5] > 0
    t.close()


def test_among(orc, corpus, table):
    rows, G, queries = corpus
    rng = np.random.default_rng(6)
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    dead = np.arange(2000, 2304, 7)
    t.delete(dead.astype(np.uint64))
    among = rng.choice(np.arange(1500, 2304), 500)          # unsorted, with duplicates, deleted rows among them
    assert np.unique(among).size < 500 and np.isin(among, dead).any()
    live = np.setdiff1d(np.unique(among), dead)
    for q in queries[:2]:
        for pool, k, gap in ((500, 500, 0.05), (100, 10, 0.08)):
            ids, dists = oracle_pool(orc, q, rows[live], pool, ids=live)
            want = expected(ids, dists, G, int, k, pool, gap)
            check(t, call(t, q, k, pool, gap, within=among), want, (pool, k))
    assert want[5] > 0
    rc, idx, dist, hidden, rep, n_kept = call(t, queries[0], 5, 64, 0.05, within=np.zeros(0, np.uint64))
    assert rc == 0 and n_kept == 0 and np.all(idx == NO_ID) and np.all(np.isinf(dist)) and not hidden.any() and np.all(rep == NO_LABEL)
    rc, idx, dist, hidden, rep, n_kept = call(t, queries[0], 5, 64, 0.05, within=np.array([3, 2304], np.uint64))
    assert rc == MI_ERR_INVALID and n_kept == 7 and np.all(idx == 7) and np.all(rep == 7)
    t.close()


def test_same_bits_across_calls_handles_and_options(orc, corpus, table):
    rows, G, queries = corpus
    q = queries[1]
    ids, dists = oracle_pool(orc, q, rows, 1000)
    want = expected(ids, dists, G, int, 100, 1000, 0.08)
    check(table, call(table, q, 100, 1000, 0.08), want, "again")
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    for prefilter in (0, 1, 2):
        for cap in (1 << 14, 1 << 22):
            t.set_option("prefilter", prefilter)
            t.set_option("join_cap", cap)
            check(t, call(t, q, 100, 1000, 0.08), want, (prefilter, cap))
    t.close()


def test_the_pool_of_a_two_stage_search(built, orc):
    n, dim, pool = 1 << 18, 256, 300
    t = EmbeddingTable(dim, 0)
    t.insert_synthetic(9, 0, n)
    t.set_option("prefilter", 1)
    rows = t.rows(0, n)
    q = (rows[12345] + 0.5 * np.random.default_rng(7).standard_normal(dim)).astype(np.float32)
    ids, dists = oracle_pool(orc, q, rows, pool)
    coords = np.sort(ids.astype(np.int64))
    G = distance_matrix(orc, rows[coords])          # over the pool's rows only, in id order
    gap = float(np.sort(G[np.triu_indices(pool, 1)])[40])   # the 41 closest pairs of the pool conflict
    want = expected(ids, dists, G, lambda i: int(np.searchsorted(coords, i)), 100, pool, gap)
    st = check(t, call(t, q, 100, pool, gap), want)
    cand, fell_back = t.prefilter_stats()
    assert not fell_back and cand >= pool          # the pool did come through the two stages
    assert st["conflicts"] == 41 and want[5] > 0
    t.close()


def test_errors_and_untouched_outputs(corpus, table):
    rows, G, queries = corpus
    q = queries[0]
    lib = _lib.lib()

    def untouched(got, code):
        rc, idx, dist, hidden, rep, n_kept = got
        assert rc == code, (rc, code)
        assert np.all(idx == 7) and np.all(dist == -7.0) and np.all(hidden == 7) and np.all(rep == 7) and n_kept == 7

    untouched(call(table, q, 0, 64, 0.05), MI_ERR_INVALID)
    untouched(call(table, q, 1, 0, 0.05), MI_ERR_INVALID)
    untouched(call(table, q, 4, 64, np.nan), MI_ERR_INVALID)
    untouched(call(table, q, 4, 64, -0.01), MI_ERR_INVALID)
    untouched(call(table, q, 4, 4097, 0.05), MI_ERR_UNSUPPORTED)
    untouched(call(table, q, 65, 64, 0.05), MI_ERR_UNSUPPORTED)
    idx, dist = np.zeros(4, np.uint64), np.zeros(4, np.float32)
    args = (4, 64, ctypes.c_float(0.05), None, 0)
    assert lib.mi_knn_search_diverse(None, q.ctypes.data, *args, idx.ctypes.data, dist.ctypes.data, None, None, None) == MI_ERR_INVALID
    assert lib.mi_knn_search_diverse(table._h, None, *args, idx.ctypes.data, dist.ctypes.data, None, None, None) == MI_ERR_INVALID
    assert lib.mi_knn_search_diverse(table._h, q.ctypes.data, *args, None, dist.ctypes.data, None, None, None) == MI_ERR_INVALID
    assert lib.mi_knn_search_diverse(table._h, q.ctypes.data, *args, idx.ctypes.data, None, None, None, None) == MI_ERR_INVALID
    assert lib.mi_knn_search_diverse(table._h, q.ctypes.data, 4, 64, ctypes.c_float(0.05), None, 3, idx.ctypes.data, dist.ctypes.data,
                                     None, None, None) == MI_ERR_INVALID
    assert lib.mi_knn_search_diverse_stats(table._h, None) == MI_ERR_INVALID
    # hidden, rep and n_kept may be NULL
    assert lib.mi_knn_search_diverse(table._h, q.ctypes.data, *args, idx.ctypes.data, dist.ctypes.data, None, None, None) == 0
    assert np.array_equal(idx, call(table, q, 4, 64, 0.05)[1])
    # a dim the mirror is not built for; an empty table; a pool larger than the table; a borrowed shard
    t = EmbeddingTable(192, 0)
    t.insert(np.ones((4, 192), np.float32))
    untouched(call(t, np.ones(192, np.float32), 2, 4, 0.05), MI_ERR_UNSUPPORTED)
    t.close()
    t = EmbeddingTable(768, 0)
    rc, idx, dist, hidden, rep, n_kept = call(t, q, 3, 8, 0.05)
    assert rc == 0 and n_kept == 0 and np.all(idx == NO_ID) and np.all(np.isinf(dist)) and not hidden.any() and np.all(rep == NO_LABEL)
    assert t.knn_diverse_stats() == {"pool": 0, "candidates": 0, "conflicts": 0, "hidden": 0}
    t.insert(rows[:3])
    rc, idx, dist, hidden, rep, n_kept = call(t, q, 8, 8, 0.0)
    assert rc == 0 and n_kept == 3 and np.all(idx[3:] == NO_ID) and np.all(rep[3:] == NO_LABEL) and sorted(rep[:3]) == [0, 1, 2]
    t.close()
    from image_search_amd.search import ShardedTable
    sh = ShardedTable(768, (0, 0), 64)
    sh.insert(rows[:256])
    borrowed = EmbeddingTable.__new__(EmbeddingTable)
    borrowed._h, borrowed.dim, borrowed.device = ctypes.c_void_p(lib.mi_knn_sharded_shard(sh._h, 0)), 768, 0
    untouched(call(borrowed, q, 2, 4, 0.05), MI_ERR_UNSUPPORTED)
    borrowed._h = ctypes.c_void_p()
    sh.close()


def test_a_gap_below_every_pair_distance_is_the_plain_search(orc, corpus, table):
    rows, G, queries = corpus
    for q in queries[::2]:
        ids, dists = oracle_pool(orc, q, rows, 200)
        s = np.sort(ids.astype(np.int64))
        smallest = np.min(G[np.ix_(s, s)][np.triu_indices(200, 1)])
        gap = np.nextafter(np.float32(smallest), np.float32(-1.0))
        assert 0.0 <= gap < smallest
        idx, dist, hidden, rep = table.knn_diverse(q, 50, float(gap), pool=200)
        p_idx, p_dist = table.knn(q, 50)
        assert np.array_equal(idx, p_idx) and np.array_equal(dist.view(np.uint32), p_dist.view(np.uint32))
        assert not hidden.any() and np.array_equal(rep[:50], np.arange(50, dtype=np.uint32)) and np.all(rep[50:] == NO_LABEL)
        assert table.knn_diverse_stats()["conflicts"] == 0
        # ... and one ulp up the closest pair conflicts
        table.knn_diverse(q, 200, float(smallest), pool=200)
        assert table.knn_diverse_stats()["conflicts"] >= 1 and table.knn_diverse_stats()["hidden"] >= 1


def test_image_index_web_search_diverse(orc, corpus):
    rows, G, queries = corpus
    sub = np.arange(1800, 2304)
    paths = [f"/srv/media/{'trip' if i % 3 else 'home'}/{i:04d}.jpg" for i in sub]
    ix = ImageIndex(768, 0, "/srv/media/")
    ix.insert(paths, rows[sub])
    gone = [paths[j] for j in range(210, 504, 11)]
    ix.remove(gone)
    live = np.array([j for j in range(504) if paths[j] not in set(gone)])
    text = queries[0]
    marked = ["media/trip/2002.jpg", "media/home/2004.jpg", "media/nowhere.jpg"]
    refined = orc_refine(orc, text, [rows[2002], rows[2004]])
    for refs, qv in (((), text), (marked, refined)):
        for folders, keep in (((), live), (("media/trip",), np.array([j for j in live if j % 3]))):
            ids, dists = oracle_pool(orc, qv, rows[sub][keep], 256, ids=keep)
            want = expected(ids, dists, G[np.ix_(sub, sub)], int, 40, 256, 0.05)
            got = ix.web_search_diverse(text, refs, k=40, min_gap=0.05, pool=256, folders=folders, web=True)
            assert len(got) == want[4]
            assert [g[0] for g in got] == [int(i) for i in want[0][:want[4]]]
            assert np.array_equal(np.array([g[2] for g in got], np.float32).view(np.uint32), want[1][:want[4]].view(np.uint32))
            assert [g[3] for g in got] == [int(h) for h in want[2][:want[4]]]
            assert all(g[1] == "media/" + paths[g[0]][len("/srv/media/"):] for g in got)
            assert not {paths[g[0]] for g in got} & set(gone)
            assert sum(g[3] for g in got) > 0
    assert ix.web_search_diverse(text, k=5, min_gap=0.05, folders=("media/none",)) == []
    ix.close()
