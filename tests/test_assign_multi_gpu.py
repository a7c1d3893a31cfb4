"""mi_knn_assign_multi on the GPU: up to m labels per row — for a live row the entries of a search over a table of the
vectors with q = the row and k = m, without those whose distance is NaN or > max_dist: the same ids and the same distance
bits, MI_KNN_NO_LABEL / +inf behind them.  Oracle: orc_cosine_dist(row, vectors) (oracle.c) followed by the search's order
(distance key ascending, then id, NaN last), as in tests/test_assign_gpu.py whose planted corpus is re-created here.
Labels are compared for equality and distances on their bits: there is no tolerance anywhere in this file."""
import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable, rows_of_labels
from oracle.binding import orc_cosine_dist

pytestmark = pytest.mark.gpu

DIM = 768
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
NO_LABEL = 0xFFFFFFFF
N_PLANTED, N_CLUSTERS = 3072, 16
INF = float("inf")


def planted_corpus(seed=11):
    """tests/test_assign_gpu.py's: 4 096 rows, 3 072 = vectors[i % 16] + sigma x noise (sigma 0.1 .. 1.5) under row scales
    0.1 .. 10, then 1 024 plain Gaussian rows; and 1 024 Gaussian vectors"""
    rng = np.random.default_rng(seed)
    vectors = rng.standard_normal((1024, DIM)).astype(np.float32)
    sigma = rng.uniform(0.1, 1.5, N_PLANTED)
    scale = rng.uniform(0.1, 10.0, N_PLANTED)
    own = np.arange(N_PLANTED) % N_CLUSTERS
    planted = (vectors[own] + sigma[:, None] * rng.standard_normal((N_PLANTED, DIM))) * scale[:, None]
    rows = np.concatenate([planted.astype(np.float32), rng.standard_normal((1024, DIM)).astype(np.float32)])
    return rows, vectors, own


def dist_keys(d):
    """the search's 32-bit distance key (knn_kernels.h dist_to_u32): ascending key = ascending distance, NaN last"""
    b = np.ascontiguousarray(d, np.float32).view(np.uint32)
    k = np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))
    return np.where(np.isnan(d), np.uint32(0xFFFFFFFF), k)


def oracle_matrix(orc, rows, vectors):
    return np.stack([orc_cosine_dist(orc, rows[r], vectors) for r in range(rows.shape[0])])


def oracle_multi(D, m, max_dist=INF, live=None):
    """the first m of every row of D under the search's order, then NaN and > max_dist removed (they are last: a suffix)"""
    n, C = D.shape
    key = (dist_keys(D).astype(np.uint64) << np.uint64(32)) | np.arange(C, dtype=np.uint64)[None, :]
    order = np.argsort(key, axis=1, kind="stable")[:, :m]
    d = np.take_along_axis(D, order, axis=1).astype(np.float32)
    ok = ~np.isnan(d) & (d <= np.float32(max_dist))
    if live is not None:
        ok &= live[:, None]
    lab = np.full((n, m), NO_LABEL, np.uint32)
    dd = np.full((n, m), np.inf, np.float32)
    lab[:, :order.shape[1]] = np.where(ok, order, NO_LABEL)
    dd[:, :order.shape[1]] = np.where(ok, d, np.float32(np.inf))
    return lab, dd


def same(got, want, what=""):
    gl, gd = got
    wl, wd = want
    assert gl.shape == wl.shape and gd.shape == wd.shape, what
    assert np.array_equal(gl, wl), (what, np.argwhere(gl != wl)[:8])
    assert not np.any(np.isnan(gd)), what
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what


@pytest.fixture(scope="module")
def corpus(built, orc):
    rows, vectors, own = planted_corpus()
    return rows, vectors, own, oracle_matrix(orc, rows, vectors)


@pytest.fixture(scope="module")
def table(corpus):
    t = EmbeddingTable(DIM, 0)
    t.insert(corpus[0])
    yield t
    t.close()


# 1: the planted corpus, no threshold; m > C pads
@pytest.mark.parametrize("m", [1, 4, 16])
@pytest.mark.parametrize("C", [1, 16, 256, 1000, 1024])
def test_planted_corpus_equals_the_oracle(corpus, table, C, m):
    rows, vectors, own, D = corpus
    want = oracle_multi(D[:, :C], m)
    got = table.assign_multi(vectors[:C], m)
    st = table.assign_multi_stats()
    print(f"C {C} m {m}: stats {st}")
    same(got, want, f"C {C} m {m}")
    if C >= N_CLUSTERS:   # the planted rows recover their vector first
        assert np.array_equal(got[0][:N_PLANTED, 0], own.astype(np.uint32))
    if m > C:
        assert np.all(got[0][:, C:] == NO_LABEL) and np.all(np.isposinf(got[1][:, C:]))
    assert st["hits"] == int(np.sum(want[0] != NO_LABEL)) and st["hits"] <= st["candidates"]


# 2: thresholds — rows with no hit, with fewer than m and with more than m within the distance; a pair exactly at max_dist
def test_thresholds_drop_what_is_beyond_them(corpus, table):
    rows, vectors, own, D = corpus
    m = 4
    kinds = set()
    at = float(np.sort(D[5])[2])   # an oracle distance as the threshold: that pair is <= max_dist and stays
    for max_dist in (0.6, 0.9, 0.95, at):
        within = np.sum(D <= np.float32(max_dist), axis=1)
        want = oracle_multi(D, m, max_dist)
        got = table.assign_multi(vectors, m, max_dist)
        print(f"max_dist {max_dist}: {int(np.sum(within == 0))} rows without a hit, {int(np.sum((within > 0) & (within < m)))} with "
              f"fewer than m, {int(np.sum(within > m))} with more; stats {table.assign_multi_stats()}")
        same(got, want, f"max_dist {max_dist}")
        hits = np.sum(got[0] != NO_LABEL, axis=1)
        assert np.array_equal(hits, np.minimum(within, m))
        assert np.all(got[1][got[0] != NO_LABEL] <= np.float32(max_dist))
        kinds |= {"none"} if np.any(within == 0) else set()
        kinds |= {"fewer"} if np.any((within > 0) & (within < m)) else set()
        kinds |= {"more"} if np.any(within > m) else set()
    assert kinds == {"none", "fewer", "more"}
    got = table.assign_multi(vectors, m, at)
    assert np.sum(got[0][5] != NO_LABEL) == 3 and got[1][5, 2] == np.float32(at)


# 3: stage 1 really filters
def test_stage1_filters(corpus, table):
    rows, vectors, own, D = corpus
    table.assign_multi(vectors, 4)
    st = table.assign_multi_stats()
    print(f"C 1024 m 4: {st}, {st['candidates'] / rows.shape[0]:.1f} candidates per row")
    # a stage 1 that passes everything must not hide behind a correct stage 2
    assert st["candidates"] <= rows.shape[0] * 1024 // 8, st
    assert st["hits"] == rows.shape[0] * 4 and st["launches"] >= 1 and st["tiles"] >= 32 * 8


# 4: m = 1 is mi_knn_assign where that reports a number; m = 8 is a real search over a table of the vectors
def test_equals_assign_and_a_search_over_the_vectors(corpus, table):
    rows, vectors, own, D = corpus
    lab1, d1 = table.assign(vectors)
    got = table.assign_multi(vectors, 1)
    num = ~np.isnan(d1)
    assert num.all()   # (this corpus has no NaN distance)
    assert np.array_equal(got[0][num, 0], lab1[num]) and np.array_equal(got[1][num, 0].view(np.uint32), d1[num].view(np.uint32))
    labels, dist = table.assign_multi(vectors, 8)
    tv = EmbeddingTable(DIM, 0)
    tv.insert(vectors)
    for r in np.random.default_rng(2).choice(rows.shape[0], 32, replace=False):
        idx, d = tv.knn(rows[r], 8)
        assert np.array_equal(idx.astype(np.uint32), labels[r]), r
        assert np.array_equal(d.view(np.uint32), dist[r].view(np.uint32)), r
    tv.close()


# 5: ordering corners (the rows and vectors of tests/test_assign_gpu.py::test_ordering_corners)
def test_ordering_corners(built, orc):
    rng = np.random.default_rng(4)
    rows = rng.standard_normal((300, DIM)).astype(np.float32)
    rows[7] = 0.0                        # a zero row: every distance NaN -> only padding
    rows[9, 5] = np.inf                  # a row with an inf element
    rows[11, 3] = 3.2e38                 # marked by the mirror (an element > 3e38)
    rows[13] *= np.float32(1e-17)        # marked: norm^2 below 1e-30
    rows[15] *= np.float32(1e14)         # marked: norm^2 above 1e30
    vec = rng.standard_normal((40, DIM)).astype(np.float32)
    vec[3] = vec[21]                     # identical vectors: both labels, the lower first
    vec[5] = vec[17] * np.float32(3.0)   # a scaled copy: tie or not, whatever the oracle says
    vec[8] = 0.0                         # a zero vector and a NaN vector never appear
    vec[10, 0] = np.nan
    vec[12, 1] = 3.3e38                  # marked vectors
    vec[14] *= np.float32(1e-17)
    vec[30:34] = rows[100:104] * np.float32(0.5)   # rows that meet their own direction
    D = oracle_matrix(orc, rows, vec)
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    for m in (1, 4, 16):
        want = oracle_multi(D, m)
        got = t.assign_multi(vec, m)
        same(got, want, f"corners m {m}")
        assert not np.any(np.isin(got[0], (8, 10)))
        assert np.all(got[0][7] == NO_LABEL) and np.all(np.isposinf(got[1][7]))
    lab, d = t.assign_multi(vec, 16)
    for r in range(300):   # the twins: never the higher label alone or first; on an ordinary row it follows the lower directly
        p3, p21 = np.flatnonzero(lab[r] == 3), np.flatnonzero(lab[r] == 21)
        assert not (p21.size and not p3.size) and not (p21.size and p21[0] < p3[0]), r
        if r >= 16 and p3.size and p3[0] + 1 < 16:
            assert lab[r, p3[0] + 1] == 21 and d[r, p3[0]].view(np.uint32) == d[r, p3[0] + 1].view(np.uint32), r
    assert np.any(lab == 3)
    # a NaN vector in front, alone: nothing but padding (mi_knn_assign says label 0, NaN here)
    lab, d = t.assign_multi(vec[10:11], 2)
    assert np.all(lab == NO_LABEL) and np.all(np.isposinf(d))
    t.close()


# 6: bounded memory — every pair a candidate, the buffer at its floor
def test_overflow_every_pair_a_candidate(built, orc):
    v = np.random.default_rng(7).standard_normal(DIM).astype(np.float32)
    t = EmbeddingTable(DIM, 0)
    t.insert(np.tile(v, (2000, 1)))
    t.set_option("join_cap", 1 << 14)
    lab, d = t.assign_multi(np.tile(v, (512, 1)), 4)
    st = t.assign_multi_stats()
    print("every pair a candidate:", st)
    want = orc_cosine_dist(orc, v, v[None, :])[0]
    assert np.array_equal(lab, np.tile(np.arange(4, dtype=np.uint32), (2000, 1)))
    assert np.all(d.view(np.uint32) == np.float32(want).view(np.uint32))
    assert st["candidates"] == 2000 * 512 and st["launches"] > 1 and st["hits"] == 2000 * 4
    t.close()


# 7: deleted rows are padded, before and after more appends; every mirror route gives the same bits
def test_deleted_rows_appends_and_mirror_routes(corpus):
    rows, vectors, own, D = corpus
    C, m, max_dist = 256, 4, 0.9
    dead = np.unique(np.random.default_rng(6).integers(0, 3000, 300))
    live = np.ones(rows.shape[0], bool)
    live[dead] = False
    results = []
    for prefilter in (0, 1, 2):
        t = EmbeddingTable(DIM, 0)
        t.insert(rows[:3000])
        if prefilter:
            t.set_option("prefilter", prefilter)
        t.delete(dead)
        got = t.assign_multi(vectors[:C], m, max_dist)
        same(got, oracle_multi(D[:3000, :C], m, max_dist, live[:3000]), f"deleted, prefilter {prefilter}")
        assert np.all(got[0][dead] == NO_LABEL) and np.all(np.isposinf(got[1][dead]))
        t.insert(rows[3000:])   # (with "prefilter" = 1 the table's mirror catches up)
        got = t.assign_multi(vectors[:C], m, max_dist)
        same(got, oracle_multi(D[:, :C], m, max_dist, live), f"deleted + appended, prefilter {prefilter}")
        assert t.assign_multi_stats()["hits"] == int(np.sum(got[0] != NO_LABEL))
        results.append(got)
        t.close()
    for got in results[1:]:
        assert np.array_equal(got[0], results[0][0]) and np.array_equal(got[1].view(np.uint32), results[0][1].view(np.uint32))


# 8: a ragged table, an empty one, the errors
def test_ragged_empty_and_errors(corpus, table):
    rows, vectors, own, D = corpus
    t = EmbeddingTable(DIM, 0)
    t.insert(rows[2900:3200])   # 300 rows: two full tiles and 44, planted and Gaussian
    for C, m in ((40, 16), (1000, 3)):
        same(t.assign_multi(vectors[:C], m), oracle_multi(D[2900:3200, :C], m), f"ragged C {C} m {m}")
    t.close()

    mi = _lib.lib()
    n = rows.shape[0]
    lab, d = np.full((n, 4), 7, np.uint32), np.full((n, 4), 7.0, np.float32)
    v = vectors.ctypes.data

    def err(rc, code):
        assert rc == code
        assert len(mi.mi_last_error()) > 0

    empty = EmbeddingTable(DIM, 0)   # an empty table succeeds and writes nothing
    assert mi.mi_knn_assign_multi(empty._h, v, 4, 4, INF, lab.ctypes.data, d.ctypes.data) == 0
    assert np.all(lab == 7) and np.all(d == 7.0)
    empty.close()
    err(mi.mi_knn_assign_multi(table._h, v, 0, 4, INF, lab.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_assign_multi(table._h, v, 4, 0, INF, lab.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_assign_multi(table._h, v, 4, 17, INF, lab.ctypes.data, d.ctypes.data), MI_ERR_UNSUPPORTED)
    big = np.zeros((65537, DIM), np.float32)
    err(mi.mi_knn_assign_multi(table._h, big.ctypes.data, 65537, 4, INF, lab.ctypes.data, d.ctypes.data), MI_ERR_UNSUPPORTED)
    err(mi.mi_knn_assign_multi(table._h, None, 4, 4, INF, lab.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_assign_multi(table._h, v, 4, 4, INF, None, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_assign_multi(None, v, 4, 4, INF, lab.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_assign_multi(table._h, v, 4, 4, float("nan"), lab.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_assign_multi(table._h, v, 4, 4, -0.5, lab.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_assign_multi_stats(table._h, None), MI_ERR_INVALID)
    odd = EmbeddingTable(192, 0)
    odd.insert(np.ones((4, 192), np.float32))
    err(mi.mi_knn_assign_multi(odd._h, v, 4, 4, INF, lab.ctypes.data, d.ctypes.data), MI_ERR_UNSUPPORTED)
    odd.close()
    assert np.all(lab == 7) and np.all(d == 7.0)   # no error wrote anything
    # dist may be NULL; the table still answers
    assert mi.mi_knn_assign_multi(table._h, v, 16, 4, INF, lab.ctypes.data, None) == 0
    assert np.array_equal(lab, oracle_multi(D[:, :16], 4)[0])


# 9: sharded; the index's tags
def test_sharded_equals_the_single_table(corpus, table):
    rows, vectors, own, D = corpus
    want = table.assign_multi(vectors[:256], 4, 0.9)
    st = ShardedTable(DIM, [0, 0], block_rows=64)
    st.insert(rows)
    got = st.assign_multi(vectors[:256], 4, 0.9)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    st.close()


def test_index_tags_with_a_removed_path(built):
    rng = np.random.default_rng(12)
    themes = rng.standard_normal((3, DIM)).astype(np.float32)
    names = ["dog", "receipt", "beach"]
    emb, paths, themes_of = [], [], {}
    for i in range(9):   # every image shows theme i % 3; every third one a second theme too
        mine = [i % 3] + ([(i + 1) % 3] if i % 3 == 0 else [])
        paths.append(f"/media/{'trip' if i % 2 else 'home'}/p{i}.jpg")
        themes_of[paths[-1]] = mine
        emb.append(themes[mine].sum(axis=0) + 0.2 * rng.standard_normal(DIM))
    paths.append("/media/home/noise.jpg")   # matches nothing
    themes_of[paths[-1]] = []
    emb.append(rng.standard_normal(DIM))
    ix = ImageIndex(DIM, 0, "/media")
    ix.insert(paths, np.asarray(emb, np.float32))
    gone = paths[5]
    ix.remove([gone])
    tags = ix.tags(themes, names=names, m=3, max_dist=0.6)
    assert gone not in tags and set(tags) == set(paths) - {gone}
    for p, hits in tags.items():
        assert sorted(n for n, _ in hits) == sorted(names[c] for c in themes_of[p]), p
        assert [d for _, d in hits] == sorted(d for _, d in hits) and all(0.0 <= d <= 0.6 for _, d in hits)
    assert tags["/media/home/noise.jpg"] == []
    assert [l for l, _ in ix.tags(themes, m=1)[paths[1]]] == [1]
    web = ix.tags(themes, web=True)
    assert all(p.startswith("media/") for p in web) and len(web) == len(tags)
    # "show me everything tagged beach"
    labels, _ = ix.table.assign_multi(themes, 3, 0.6)
    assert rows_of_labels(labels, 3)[2].tolist() == [r for r, p in enumerate(paths) if p != gone and 2 in themes_of[p]]
    ix.close()
