"""mi_knn_search_compound on the GPU: ids and distance BITS for equality with the numpy restatement
(tests/test_compound_host.py: expected), which is fed by the CPU oracle alone — D[j] = orc_cosine_dist(term j, rows), what the
single pass with q = term j reports.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable
from oracle.binding import orc_cosine_dist
from test_compound_host import NO_ID, bits, dist_key, expected, expected_term_dist, key_dist

pytestmark = pytest.mark.gpu

MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
MODES = {"all": 0, "any": 1}


def call(t, pos, mode, neg=None, within=None, k=10, among=None, want_td=True, n_pos=None, n_neg=None, mode_code=None):
    """the C call with every output -> (rc, idx, dist, term_dist); the arrays keep a sentinel where nothing was written"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, t.dim)
    neg = np.zeros((0, t.dim), np.float32) if neg is None else np.ascontiguousarray(neg, np.float32).reshape(-1, t.dim)
    w = np.ascontiguousarray([] if within is None else within, np.float32).reshape(-1)
    n_pos = pos.shape[0] if n_pos is None else n_pos
    n_neg = neg.shape[0] if n_neg is None else n_neg
    T = max(pos.shape[0] + neg.shape[0], 1)
    idx, dist = np.full(max(k, 1), 7, np.uint64), np.full(max(k, 1), -7.0, np.float32)
    td = np.full((max(k, 1), T), -7.0, np.float32)
    ids, n_ids = None, 0
    if among is not None:
        a = np.ascontiguousarray(among, np.uint64)
        n_ids = a.size
        ids = (a if a.size else np.zeros(1, np.uint64)).ctypes.data
    rc = _lib.lib().mi_knn_search_compound(t._h, pos.ctypes.data if pos.size else None, n_pos, MODES.get(mode, 0) if mode_code is None else mode_code,
                                           neg.ctypes.data if neg.size else None, w.ctypes.data if w.size else None, n_neg, k, ids, n_ids,
                                           idx.ctypes.data, dist.ctypes.data, td.ctypes.data if want_td else None)
    return rc, idx, dist, td


def per_term(orc, terms, rows):
    terms = np.asarray(terms, np.float32).reshape(-1, rows.shape[1])
    if terms.shape[0] == 0 or rows.shape[0] == 0:
        return np.zeros((terms.shape[0], rows.shape[0]), np.float32)
    return np.stack([orc_cosine_dist(orc, q, rows) for q in terms])


def same_bits(a, b):
    """equal bit for bit, a NaN compared as a NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.where(np.isnan(a), np.uint32(0x7FC00000), bits(a)),
                                                 np.where(np.isnan(b), np.uint32(0x7FC00000), bits(b)))


def check(t, orc, rows, ids, pos, mode, neg=None, within=None, k=10, among=None, what="", scanned=None):
    """one call against the restatement over the candidate rows `rows` held under `ids`; returns the want"""
    ids = np.asarray(ids, np.uint64)
    neg_ = np.zeros((0, rows.shape[1]), np.float32) if neg is None else np.asarray(neg, np.float32).reshape(-1, rows.shape[1])
    w_ = [] if within is None else within
    D_pos, D_neg = per_term(orc, pos, rows), per_term(orc, neg_, rows)
    w_idx, w_dist, order, w_ex, w_nan = expected(D_pos, D_neg, w_, mode, k, ids)
    rc, idx, dist, td = call(t, pos, mode, neg, within, k, among)
    assert rc == 0, (what, _lib.lib().mi_last_error())
    assert np.array_equal(idx[:k], w_idx), (what, idx[:8], w_idx[:8])
    assert np.array_equal(bits(dist[:k]), bits(w_dist)), what
    w_td = expected_term_dist(D_pos, D_neg, order, k)
    assert same_bits(td[:k], w_td), what
    # dist is the fold of that row of term_dist
    n_pos, n = D_pos.shape[0], order.size
    if n:
        keys = dist_key(td[:n, :n_pos])
        fold = keys.max(axis=1) if mode == "all" else keys.min(axis=1)
        assert np.array_equal(bits(key_dist(fold)), bits(dist[:n])), what
    st = t.knn_compound_stats()
    assert st == {"scanned": rows.shape[0] if scanned is None else scanned, "excluded": w_ex, "nan": w_nan, "results": n}, (what, st, w_ex, w_nan, n)
    return w_idx, w_dist, order, w_ex, w_nan


@pytest.fixture(scope="module")
def corpus(built):
    rng = np.random.default_rng(2026)
    rows = rng.standard_normal((5000, 768)).astype(np.float32)
    # eight terms near rows on both sides of tile edges
    terms = (rows[[3, 70, 500, 64, 999, 1, 63, 65]] + 0.7 * rng.standard_normal((8, 768))).astype(np.float32)
    return rows, terms


@pytest.fixture(scope="module")
def table5000(corpus):
    t = EmbeddingTable(768, 0)
    t.insert(corpus[0])
    yield t
    t.close()


@pytest.fixture(scope="module")
def table1000(corpus):
    t = EmbeddingTable(768, 0)
    t.insert(corpus[0][:1000])
    yield t
    t.close()


def mid(orc, term, rows):
    """a threshold that excludes about half of the rows"""
    return float(np.median(orc_cosine_dist(orc, term, rows)))


# ---- tile edges, every padding of the term count, both modes ---------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_tile_edges_and_term_counts(orc, corpus, N):
    rows, terms = corpus
    rows = rows[:N]
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    ids = np.arange(N)
    for T in (1, 2, 3, 5, 8):
        for mode in ("all", "any"):
            for k in (1, 10, 64):
                check(t, orc, rows, ids, terms[:T], mode, k=k, what=("pos", N, T, mode, k))
        if T >= 3:   # the same count with a negative term among them
            check(t, orc, rows, ids, terms[:T - 1], "all", terms[T - 1:T], [mid(orc, terms[T - 1], rows)], k=10, what=("neg", N, T))
    t.close()


# ---- several tiles per wave and both merge depths -----------------------------------------------------------------------------

def test_two_level_merge_default_grid(orc, corpus, table5000):
    rows, terms = corpus
    for mode in ("all", "any"):
        for k in (1, 10, 64):
            check(table5000, orc, rows, np.arange(5000), terms[:3], mode, terms[3:5], [0.9, mid(orc, terms[4], rows)], k=k, what=(mode, k))


def test_compound_blocks_changes_no_answer(orc, corpus, table1000):
    rows, terms = corpus
    rows = rows[:1000]
    try:
        for blocks in (1, 3, 0, 1000):
            table1000.set_option("compound_blocks", blocks)
            for k in (10, 64, 100):
                check(table1000, orc, rows, np.arange(1000), terms[:2], "all", terms[2:3], [mid(orc, terms[2], rows)], k=k, what=(blocks, k))
                check(table1000, orc, rows, np.arange(1000), terms[:5], "any", k=k, what=(blocks, k, "any"))
    finally:
        table1000.set_option("compound_blocks", 0)
    with pytest.raises(_lib.MiError):
        table1000.set_option("compound_blocks", -1)


# ---- the select path ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [65, 1000, 4096])
def test_select_path(orc, corpus, table5000, k):
    rows, terms = corpus
    ids = np.arange(5000)
    check(table5000, orc, rows, ids, terms[:2], "all", k=k, what=("all", k))
    check(table5000, orc, rows, ids, terms[:4], "any", k=k, what=("any", k))
    # about half of the rows excluded: at k = 4096 fewer rows qualify than k, the tail (term_dist too) is padding
    want = check(table5000, orc, rows, ids, terms[:2], "all", terms[2:3], [mid(orc, terms[2], rows)], k=k, what=("neg", k))
    if k == 4096:
        assert want[2].size < k and want[0][-1] == NO_ID


@pytest.mark.parametrize("dim", [128, 1024])
def test_other_dims(orc, built, dim):
    rng = np.random.default_rng(dim)
    rows = rng.standard_normal((300, dim)).astype(np.float32)
    terms = (rows[[3, 70, 200, 64, 299, 1, 63, 65]] + 0.7 * rng.standard_normal((8, dim))).astype(np.float32)
    t = EmbeddingTable(dim, 0)
    t.insert(rows)
    for T in (1, 2, 4, 8):
        for mode in ("all", "any"):
            for k in (10, 100):
                check(t, orc, rows, np.arange(300), terms[:T], mode, k=k, what=(dim, T, mode, k))
    check(t, orc, rows, np.arange(300), terms[:3], "all", terms[3:6], [0.0, mid(orc, terms[4], rows), np.inf], k=10, what=(dim, "neg"))
    check(t, orc, rows, np.arange(300), terms[:3], "any", terms[3:5], [mid(orc, terms[3], rows), 0.5], k=300, what=(dim, "neg select"))
    t.close()


# ---- negatives ------------------------------------------------------------------------------------------------------------------

def test_negative_terms_and_thresholds(orc, corpus, table1000):
    rows, terms = corpus
    rows = rows[:1000]
    ids = np.arange(1000)
    m = [mid(orc, terms[j], rows) for j in range(8)]
    for k in (10, 100):
        for w in (0.0, m[5], np.inf):
            want = check(table1000, orc, rows, ids, terms[:2], "all", terms[5:6], [w], k=k, what=(1, w, k))
            assert want[3] == (0 if w == 0.0 else 1000 if w == np.inf else want[3])
        want = check(table1000, orc, rows, ids, terms[:2], "any", terms[5:8], [m[5], 0.0, m[7]], k=k, what=(3, k))
        assert 0 < want[3] < 1000
        check(table1000, orc, rows, ids, terms[:1], "all", terms[5:8], [np.inf, 0.0, 0.0], k=k, what=("all gone", k))
    # a threshold at the oracle's exact bits of a chosen row excludes it; one ulp below returns it
    d_neg = orc_cosine_dist(orc, terms[5], rows)
    best = int(expected(per_term(orc, terms[:2], rows), [], [], "all", 1, ids)[0][0])
    at = np.float32(d_neg[best])
    want = check(table1000, orc, rows, ids, terms[:2], "all", terms[5:6], [at], k=10, what="at the threshold")
    assert best not in want[0].tolist()
    want = check(table1000, orc, rows, ids, terms[:2], "all", terms[5:6], [np.nextafter(at, np.float32(0))], k=10, what="one below")
    assert int(want[0][0]) == best


# ---- NaN ------------------------------------------------------------------------------------------------------------------------

def test_nan_rows_and_zero_terms(orc, corpus):
    rows, terms = corpus
    rows = rows[:200].copy()
    rows[17] = 0.0                       # x.x = 0: every distance to it is NaN
    rows[130, 5] = np.inf                # an inf element: NaN too
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    ids = np.arange(200)
    zero = np.zeros((1, 768), np.float32)
    for k in (10, 200):
        want = check(t, orc, rows, ids, terms[:2], "all", k=k, what=("nan rows all", k))
        assert want[4] == 2 and 17 not in want[0].tolist() and 130 not in want[0].tolist()
        assert check(t, orc, rows, ids, terms[:2], "any", k=k, what=("nan rows any", k))[4] == 2
        # a zero positive term: ignored under ANY, poisons ALL (an empty result, MI_OK)
        with_zero = np.concatenate([terms[:1], zero, terms[1:2]])
        a = check(t, orc, rows, ids, with_zero, "any", k=k, what=("zero term any", k))
        b = check(t, orc, rows, ids, terms[:2], "any", k=k, what=("any", k))
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
        e = check(t, orc, rows, ids, with_zero, "all", k=k, what=("zero term all", k))
        assert e[4] == 200 and np.all(e[0] == NO_ID)
        # a zero negative term excludes nothing, whatever its threshold
        z = check(t, orc, rows, ids, terms[:2], "all", zero, [np.inf], k=k, what=("zero negative", k))
        assert z[3] == 0 and np.array_equal(z[0], want[0])
    t.close()


# ---- ties -----------------------------------------------------------------------------------------------------------------------

def test_exact_copies_are_ordered_by_id_across_a_tile_edge(orc, corpus):
    rows, terms = corpus
    rows = rows[:300].copy()
    rows[60:70] = rows[5]                # a block of copies over the edge at 64
    rows[120:136] = rows[200]            # ... and over the edge at 128
    rows[250] = rows[5]
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    near = (rows[[5, 200]] + 0.05).astype(np.float32)
    for mode in ("all", "any"):
        for k in (20, 64, 300):
            want = check(t, orc, rows, np.arange(300), near, mode, k=k, what=("ties", mode, k))
            if mode == "any" and k >= 29:   # both blocks lead the list (a term sits next to each); equal scores in id order
                assert sorted(want[0][:29].tolist()) == sorted([5] + list(range(60, 70)) + [250] + list(range(120, 136)) + [200])
    t.close()


# ---- deleted rows ---------------------------------------------------------------------------------------------------------------

def test_deleted_rows(orc, corpus):
    rows, terms = corpus
    rows = rows[:1000]
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    gone = sorted(set(range(60, 70)) | set(range(128, 192)) | {0, 511, 512, 999})   # straddles a bitmap word; a whole tile
    t.delete(gone)
    live = np.array([r for r in range(1000) if r not in set(gone)])
    try:
        for blocks in (0, 1):
            t.set_option("compound_blocks", blocks)
            for k in (10, 64, 100, 1000):
                check(t, orc, rows[live], live, terms[:3], "all", terms[3:4], [mid(orc, terms[3], rows)], k=k, what=("deleted", blocks, k), scanned=1000)
                check(t, orc, rows[live], live, terms[:2], "any", k=k, what=("deleted any", blocks, k), scanned=1000)
    finally:
        t.set_option("compound_blocks", 0)
    t.close()


# ---- among ----------------------------------------------------------------------------------------------------------------------

def test_among(orc, corpus):
    rows, terms = corpus
    rows = rows[:1000]
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    gone = [5, 64, 300, 301, 700]
    t.delete(gone)
    rng = np.random.default_rng(5)
    for n in (0, 1, 64, 65, 700):
        chosen = rng.choice(1000, n, replace=False)
        if n >= 64:
            chosen[:3] = gone[:3]                                  # deleted ids are allowed and left out
        among = np.concatenate([chosen, chosen[: n // 3]])          # duplicates
        rng.shuffle(among)
        keep = np.array(sorted(set(int(c) for c in chosen) - set(gone)), np.int64)
        for k in (10, 100):
            for mode in ("all", "any"):
                check(t, orc, rows[keep], keep, terms[:3], mode, terms[3:4], [mid(orc, terms[3], rows)], k=k, among=among,
                      what=("among", n, k, mode), scanned=keep.size)
    # an id outside the table: MI_ERR_INVALID, nothing written
    rc, idx, dist, td = call(t, terms[:2], "all", k=5, among=[1, 2, 1000])
    assert rc == MI_ERR_INVALID and np.all(idx == 7) and np.all(dist == -7.0) and np.all(td == -7.0)
    t.close()


# ---- the two identities -----------------------------------------------------------------------------------------------------------

def test_one_term_is_the_plain_search_and_a_repeated_term_changes_nothing(orc, corpus):
    rows, terms = corpus
    rows = rows[:1000].copy()
    rows[40] = 0.0                        # a NaN entry of the plain search
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    for k in (10, 64, 1000):
        p_idx, p_dist = t.knn(terms[0], k)
        ok = ~np.isnan(p_dist) & (p_idx != NO_ID)
        for mode in ("all", "any"):
            idx, dist = t.knn_compound(terms[:1], mode, k=k)
            n = int(ok.sum())
            assert np.array_equal(idx[:n], p_idx[ok]) and np.array_equal(bits(dist[:n]), bits(p_dist[ok]))
            assert np.all(idx[n:] == NO_ID) and np.all(np.isinf(dist[n:]))
            once = t.knn_compound(terms[:3], mode, k=k, term_dist=True)
            twice = t.knn_compound(terms[[0, 1, 2, 1, 0]], mode, k=k, term_dist=True)
            assert np.array_equal(once[0], twice[0]) and np.array_equal(bits(once[1]), bits(twice[1]))
            assert same_bits(once[2], twice[2][:, :3])
    t.close()


# ---- base, borrowed shard, sharded table ----------------------------------------------------------------------------------------

def test_base_and_borrowed_shard(orc, corpus):
    rows, terms = corpus
    rows = rows[:300]
    base = 10 ** 12
    t = EmbeddingTable(768, 0)
    t.set_base(base)
    t.insert(rows)
    want = check(t, orc, rows, base + np.arange(300), terms[:2], "all", terms[2:3], [mid(orc, terms[2], rows)], k=10, what="base")
    assert np.all(want[0] >= base)
    check(t, orc, rows[10:200], base + np.arange(10, 200), terms[:2], "any", k=100, among=base + np.arange(10, 200), what="base among", scanned=190)
    rc, idx, dist, td = call(t, terms[:2], "all", k=5, among=[3])     # an id below the base is not a row
    assert rc == MI_ERR_INVALID and np.all(idx == 7)
    t.close()
    sh = ShardedTable(768, (0, 0), 64)
    sh.insert(rows[:256])
    borrowed = EmbeddingTable.__new__(EmbeddingTable)
    borrowed._h, borrowed.dim, borrowed.device = ctypes.c_void_p(_lib.lib().mi_knn_sharded_shard(sh._h, 1)), 768, 0
    held = np.array([r for r in range(256) if (r // 64) % 2 == 1])    # shard 1 of 2 holds the odd blocks, under their global ids
    check(borrowed, orc, rows[held], held, terms[:3], "all", k=10, what="borrowed")
    check(borrowed, orc, rows[held[5:70]], held[5:70], terms[:3], "any", k=100, among=held[5:70], what="borrowed among", scanned=65)
    borrowed._h = ctypes.c_void_p()
    sh.close()


def test_sharded_equals_one_table(orc, corpus):
    rows, terms = corpus
    rows = rows[:1000]
    sh = ShardedTable(768, devices=(0, 0, 0), block_rows=64)
    sh.insert(rows)
    one = EmbeddingTable(768, 0)
    one.insert(rows)
    w = [mid(orc, terms[3], rows)]
    rng = np.random.default_rng(9)
    within = rng.choice(1000, 400, replace=False)

    def same(**kw):
        for mode in ("all", "any"):
            for k in (10, 100):
                a = sh.knn_compound(terms[:3], mode, terms[3:4], w, k=k, **kw)
                b = one.knn_compound(terms[:3], mode, terms[3:4], w, k=k, **kw)
                assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), (mode, k, kw)
                assert a[0][0] != NO_ID
    same()
    same(within=within)
    gone = [0, 63, 64, 65, 500, 999] + [int(i) for i in within[:40]]
    sh.delete(gone)
    one.delete(gone)
    same()
    same(within=within)
    live = np.array([r for r in range(1000) if r not in set(gone)])
    check(one, orc, rows[live], live, terms[:3], "all", terms[3:4], w, k=10, what="one table, deleted", scanned=1000)
    idx, dist = sh.knn_compound(terms[:3], "all", k=5, within=[])
    assert np.all(idx == NO_ID) and np.all(np.isinf(dist))
    with pytest.raises(_lib.MiError):
        sh.knn_compound(terms[:3], "all", k=5, within=[1000])
    one.close()
    sh.close()


# ---- the index ------------------------------------------------------------------------------------------------------------------

def test_image_index_web_search_compound(orc, corpus):
    rows, terms = corpus
    rows = rows[:504]
    paths = [f"/srv/media/{'trip' if i % 3 else 'home'}/{i:04d}.jpg" for i in range(504)]
    ix = ImageIndex(768, 0, "/srv/media/")
    ix.insert(paths, rows)
    gone = [paths[j] for j in range(210, 504, 11)]
    ix.remove(gone)
    live = np.array([j for j in range(504) if paths[j] not in set(gone)])
    w = [mid(orc, terms[3], rows)]
    for folders, keep in (((), live), (("media/trip",), np.array([j for j in live if j % 3]))):
        for mode in ("all", "any"):
            got = ix.web_search_compound(terms[:2], mode, terms[3:4], w, k=40, folders=folders, term_dist=True, web=True)
            idx, dist, td = ix.table.knn_compound(terms[:2], mode, terms[3:4], w, k=40, within=keep, term_dist=True)
            D_pos, D_neg = per_term(orc, terms[:2], rows[keep]), per_term(orc, terms[3:4], rows[keep])
            w_idx, w_dist, order, _, _ = expected(D_pos, D_neg, w, mode, 40, keep)
            assert np.array_equal(idx, w_idx) and np.array_equal(bits(dist), bits(w_dist))
            n = int((idx != NO_ID).sum())
            assert len(got) == n == 40
            assert [g[0] for g in got] == [int(i) for i in idx[:n]]
            assert np.array_equal(bits(np.array([g[2] for g in got], np.float32)), bits(dist[:n]))
            assert same_bits(np.array([g[3] for g in got], np.float32), td[:n])
            assert all(g[1] == "media/" + paths[g[0]][len("/srv/media/"):] for g in got)
            assert not {paths[g[0]] for g in got} & set(gone)
    assert ix.web_search_compound(terms[:2], "all", k=5, folders=("media/none",)) == []
    ix.close()


# ---- errors and the empty cases ---------------------------------------------------------------------------------------------------

def test_errors_write_nothing_and_empty_sets_pad(corpus, table1000):
    rows, terms = corpus
    t = table1000
    lib = _lib.lib()

    def untouched(got, code):
        rc, idx, dist, td = got
        assert rc == code, (rc, lib.mi_last_error())
        assert np.all(idx == 7) and np.all(dist == -7.0) and np.all(td == -7.0)

    untouched(call(t, terms[:1], "all", k=0), MI_ERR_INVALID)
    untouched(call(t, terms[:1], "all", k=4, n_pos=0), MI_ERR_INVALID)
    untouched(call(t, np.zeros((0, 768), np.float32), "all", k=4, n_pos=1), MI_ERR_INVALID)          # pos is NULL
    untouched(call(t, terms[:1], "all", k=4, mode_code=2), MI_ERR_INVALID)
    untouched(call(t, terms[:1], "all", k=4, n_neg=1), MI_ERR_INVALID)                               # negatives without neg / neg_within
    untouched(call(t, terms[:1], "all", terms[1:2], [np.nan], k=4), MI_ERR_INVALID)
    untouched(call(t, terms[:1], "all", terms[1:2], [-1e-9], k=4), MI_ERR_INVALID)
    untouched(call(t, terms[:1], "all", k=4, among=[1000]), MI_ERR_INVALID)
    v = terms[0]
    idx, dist = np.full(4, 7, np.uint64), np.full(4, -7.0, np.float32)
    assert lib.mi_knn_search_compound(t._h, v.ctypes.data, 1, 0, None, None, 0, 4, None, 0, None, dist.ctypes.data, None) == MI_ERR_INVALID
    assert lib.mi_knn_search_compound(t._h, v.ctypes.data, 1, 0, None, None, 0, 4, None, 0, idx.ctypes.data, None, None) == MI_ERR_INVALID
    assert lib.mi_knn_search_compound(t._h, v.ctypes.data, 1, 0, None, None, 0, 4, None, 3, idx.ctypes.data, dist.ctypes.data, None) == MI_ERR_INVALID
    assert np.all(idx == 7) and np.all(dist == -7.0)
    assert call(t, np.tile(terms, (2, 1))[:9], "all", k=4)[0] == MI_ERR_UNSUPPORTED                  # 9 terms
    assert call(t, terms[:5], "all", terms[:4], [0.1] * 4, k=4)[0] == MI_ERR_UNSUPPORTED            # 5 + 4
    assert call(t, terms[:1], "all", k=4097)[0] == MI_ERR_UNSUPPORTED
    odd = EmbeddingTable(192, 0)
    odd.insert(np.ones((3, 192), np.float32))
    assert call(odd, np.ones((1, 192), np.float32), "all", k=2)[0] == MI_ERR_UNSUPPORTED            # a dim outside the set
    odd.close()
    # an empty table, an empty candidate set: all padding, MI_OK
    e = EmbeddingTable(768, 0)
    for target, among in ((e, None), (t, [])):
        rc, idx, dist, td = call(target, terms[:2], "any", terms[2:3], [0.5], k=3, among=among)
        assert rc == 0 and np.all(idx == NO_ID) and np.all(np.isinf(dist)) and np.all(np.isinf(td)) and np.all(td > 0)
        assert target.knn_compound_stats() == {"scanned": 0, "excluded": 0, "nan": 0, "results": 0}
    e.close()
    # without term_dist the call writes idx / dist alone; the Python surface validates its own arguments
    rc, idx, dist, td = call(t, terms[:2], "all", k=4, want_td=False)
    assert rc == 0 and np.all(td == -7.0) and np.all(idx != 7)
    with pytest.raises(ValueError):
        t.knn_compound(terms[:2], "most")
    with pytest.raises(ValueError):
        t.knn_compound(terms[:2], "all", without=terms[2:4], without_within=[0.1, 0.2, 0.3])
