"""mi_knn_assign on the GPU: every row labelled by the nearest of C vectors — for a live row the first entry of a search
over a table of the vectors with q = the row: the same id and the same distance bits.  Oracle: orc_cosine_dist(row,
vectors) (oracle.c) followed by the search's order (distance key ascending, then id, NaN last).  Labels are compared for
equality and distances on their bits: there is no tolerance anywhere in this file."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ShardedTable
from oracle.binding import orc_cosine_dist
from test_join_bound import worst_pair

pytestmark = pytest.mark.gpu

DIM = 768
EPS2 = 2.0 ** -7 + 2.0 ** -16 + 4.1 * (DIM + 8) * 2.0 ** -24 + 2e-6
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
NO_LABEL = 0xFFFFFFFF
N_PLANTED, N_CLUSTERS = 3072, 16


def planted_corpus(seed=11):
    """4 096 rows: 3 072 = vectors[i % 16] + sigma x noise (sigma 0.1 .. 1.5) under row scales 0.1 .. 10, then 1 024 plain
    Gaussian rows; and 1 024 Gaussian vectors"""
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


def oracle_assign(D, live=None):
    lab = np.argmin(dist_keys(D), axis=1).astype(np.uint32)   # (the first minimum: the lower label)
    d = D[np.arange(D.shape[0]), lab].astype(np.float32)
    if live is not None:
        lab[~live] = NO_LABEL
        d[~live] = np.inf
    return lab, d


def same(got, want, what=""):
    gl, gd = got
    wl, wd = want
    assert np.array_equal(gl, wl), (what, np.flatnonzero(gl != wl)[:8])
    nan = np.isnan(wd)
    assert np.array_equal(np.isnan(gd), nan), what
    assert np.array_equal(gd.view(np.uint32)[~nan], wd.view(np.uint32)[~nan]), what


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


# 1 + 3: the planted corpus against 1, 16, 256, 1 024 and a ragged 1 000 vectors; stage 1 really filters
@pytest.mark.parametrize("C", [1, 16, 256, 1024, 1000])
def test_planted_corpus_equals_the_oracle_and_stage1_filters(corpus, table, C):
    rows, vectors, own, D = corpus
    want = oracle_assign(D[:, :C])
    got = table.assign(vectors[:C])
    st = table.assign_stats()
    print(f"C {C}: stats {st}")
    same(got, want, f"C {C}")
    if C >= N_CLUSTERS:   # the planted rows recover their vector
        assert np.array_equal(got[0][:N_PLANTED], own.astype(np.uint32))
    assert st["rows"] == rows.shape[0]
    assert st["rows"] <= st["candidates"]
    if C in (256, 1024):
        # a stage 1 that passes everything must not hide behind a correct stage 2 (the final-maximum band holds 1.2 % / 0.4 % here)
        assert st["candidates"] <= rows.shape[0] * C // 8, st


# 2: the result equals a real search over a table of the vectors
def test_assign_equals_a_search_over_the_vectors(corpus, table):
    rows, vectors, own, D = corpus
    labels, dist = table.assign(vectors)
    tv = EmbeddingTable(DIM, 0)
    tv.insert(vectors)
    for r in np.random.default_rng(2).choice(rows.shape[0], 32, replace=False):
        idx, d = tv.knn(rows[r], 1)
        assert int(idx[0]) == int(labels[r]), r
        assert d.view(np.uint32)[0] == dist.view(np.uint32)[r], r
    tv.close()


# 4: ordering corners
def test_ordering_corners(built, orc):
    rng = np.random.default_rng(4)
    rows = rng.standard_normal((300, DIM)).astype(np.float32)
    rows[7] = 0.0                        # a zero row: every distance NaN -> label 0
    rows[9, 5] = np.inf                  # a row with an inf element
    rows[11, 3] = 3.2e38                 # marked by the mirror (an element > 3e38)
    rows[13] *= np.float32(1e-17)        # marked: norm^2 below 1e-30
    rows[15] *= np.float32(1e14)         # marked: norm^2 above 1e30
    vec = rng.standard_normal((40, DIM)).astype(np.float32)
    vec[3] = vec[21]                     # identical vectors: the lower label wins on every row
    vec[5] = vec[17] * np.float32(3.0)   # a scaled copy: tie or not, whatever the oracle says
    vec[8] = 0.0                         # a zero vector and a NaN vector never win unless the oracle says so
    vec[10, 0] = np.nan
    vec[12, 1] = 3.3e38                  # marked vectors
    vec[14] *= np.float32(1e-17)
    vec[30:34] = rows[100:104] * np.float32(0.5)   # rows that meet their own direction
    D = oracle_matrix(orc, rows, vec)
    want = oracle_assign(D)
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    got = t.assign(vec)
    same(got, want, "corners")
    assert not np.any(got[0] == 21) and got[0][7] == 0 and np.isnan(got[1][7])
    assert not np.any(np.isin(got[0][~np.isnan(want[1])], (8, 10)))
    # a NaN vector in front, alone: label 0 and NaN for every row
    lab, d = t.assign(vec[10:11])
    assert np.all(lab == 0) and np.all(np.isnan(d))
    t.close()


def _bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


# 5: rows at the rounding's worst case, vectors placed so that the bf16 winner is not the fp32 winner
def test_worst_case_rounding_keeps_the_exact_winner(built, orc):
    rng = np.random.default_rng(5)
    n = 64
    rows, vec = np.empty((n, DIM), np.float32), np.empty((2 * n, DIM), np.float32)
    for i in range(n):
        x, y = worst_pair(rng, +1)
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        cos_xy = x64 @ y64 / np.sqrt((x64 @ x64) * (y64 @ y64))
        # z: bf16-exact, its exact cosine to x 1e-3 below y's — y loses 2^-7 to the rounding, z only 2^-8
        noise = rng.standard_normal(DIM)
        lo, hi = 0.0, 4.0
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            z = _bf16((x64 / np.linalg.norm(x64) * np.sqrt(DIM) + mid * noise).astype(np.float32)).astype(np.float64)
            c = x64 @ z / np.sqrt((x64 @ x64) * (z @ z))
            lo, hi = (mid, hi) if c > cos_xy - 1e-3 else (lo, mid)
        rows[i], vec[2 * i], vec[2 * i + 1] = x, y, z.astype(np.float32)
    D = oracle_matrix(orc, rows, vec)
    want = oracle_assign(D)
    xb, vb = _bf16(rows).astype(np.float64), _bf16(vec).astype(np.float64)
    coarse = (xb @ vb.T) / np.sqrt(np.sum(rows.astype(np.float64) ** 2, 1)[:, None] * np.sum(vec.astype(np.float64) ** 2, 1)[None, :])
    flipped = int(np.sum(np.argmax(coarse, axis=1) != want[0]))
    print(f"{flipped} of {n} rows whose bf16 winner is not the fp32 winner")
    assert flipped >= n // 2   # the premise of this test
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    same(t.assign(vec), want, "worst case")
    t.close()


# 6: deleted rows
def test_deleted_rows(corpus):
    rows, vectors, own, D = corpus
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    dead = np.unique(np.random.default_rng(6).integers(0, rows.shape[0], 300))
    t.delete(dead)
    live = np.ones(rows.shape[0], bool)
    live[dead] = False
    got = t.assign(vectors[:256])
    same(got, oracle_assign(D[:, :256], live), "deleted")
    assert np.all(got[0][dead] == NO_LABEL) and np.all(np.isposinf(got[1][dead]))
    st = t.assign_stats()
    assert st["rows"] == int(live.sum()) and st["rows"] <= st["candidates"]
    t.close()


# 7: bounded memory — every pair a candidate, the buffer at its floor
def test_bounded_memory_every_pair_a_candidate(built, orc):
    v = np.random.default_rng(7).standard_normal(DIM).astype(np.float32)
    t = EmbeddingTable(DIM, 0)
    t.insert(np.tile(v, (6000, 1)))
    t.set_option("join_cap", 1 << 14)
    lab, d = t.assign(np.tile(v, (4096, 1)))
    st = t.assign_stats()
    print("every pair a candidate:", st)
    want = orc_cosine_dist(orc, v, v[None, :])[0]
    assert np.all(lab == 0)
    assert np.all(d.view(np.uint32) == np.float32(want).view(np.uint32))
    assert st["candidates"] == 6000 * 4096 and st["launches"] > 1
    t.close()


# 8: scale — 300 000 synthetic rows, the table's own mirror and a mirror of the call's own
def test_scale_300k_rows_both_mirror_routes(built, orc):
    n, C = 300_000, 512
    vec = np.random.default_rng(8).standard_normal((C, DIM)).astype(np.float32)
    sample = np.random.default_rng(9).choice(n, 2000, replace=False)
    want = None
    for prefilter in (1, 2):
        t = EmbeddingTable(DIM, 0)
        t.insert_synthetic(5, 0, n)
        t.set_option("prefilter", prefilter)
        lab, d = t.assign(vec)
        print(f"prefilter {prefilter}:", t.assign_stats())
        if want is None:
            srows = np.concatenate([t.rows(int(r), 1) for r in sample])
            want = oracle_assign(oracle_matrix(orc, srows, vec))
        same((lab[sample], d[sample]), want, f"prefilter {prefilter}")
        lab2, d2 = t.assign(vec)   # (with 1: the table's mirror, now built)
        assert np.array_equal(lab, lab2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))
        t.close()


# 9: sharded
@pytest.mark.parametrize("shards", [1, 3, 8])
def test_sharded_equals_the_single_table(corpus, table, shards):
    rows, vectors, own, D = corpus
    want = table.assign(vectors[:256])
    st = ShardedTable(DIM, [0] * shards, block_rows=64)
    st.insert(rows)
    got = st.assign(vectors[:256])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    st.close()


# 10: errors
def test_errors_leave_the_table_usable(corpus, table):
    rows, vectors, own, D = corpus
    mi = _lib.lib()
    n = rows.shape[0]
    lab, d = np.empty(n, np.uint32), np.empty(n, np.float32)
    big = np.zeros((65537, DIM), np.float32)

    def err(rc, code):
        assert rc == code
        assert len(mi.mi_last_error()) > 0

    err(mi.mi_knn_assign(table._h, vectors.ctypes.data, 0, lab.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_assign(table._h, big.ctypes.data, 65537, lab.ctypes.data, d.ctypes.data), MI_ERR_UNSUPPORTED)
    err(mi.mi_knn_assign(table._h, None, 4, lab.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_assign(table._h, vectors.ctypes.data, 4, None, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_assign(None, vectors.ctypes.data, 4, lab.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_assign_stats(table._h, None), MI_ERR_INVALID)
    odd = EmbeddingTable(192, 0)
    odd.insert(np.ones((4, 192), np.float32))
    err(mi.mi_knn_assign(odd._h, vectors.ctypes.data, 4, lab.ctypes.data, d.ctypes.data), MI_ERR_UNSUPPORTED)
    odd.close()
    empty = EmbeddingTable(DIM, 0)   # an empty table succeeds and writes nothing
    assert mi.mi_knn_assign(empty._h, vectors.ctypes.data, 4, lab.ctypes.data, None) == 0
    empty.close()
    # dist may be NULL; the table still answers
    assert mi.mi_knn_assign(table._h, vectors.ctypes.data, 16, lab.ctypes.data, None) == 0
    assert np.array_equal(lab, oracle_assign(D[:, :16])[0])
