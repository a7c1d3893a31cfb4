"""The dims the tile-based calls dispatch on beside 768: near_pairs, near_pairs_with, dbscan, dbscan_levels, the sharded
dbscan, assign, assign_multi, knn_many and neighbors at dim 128, 256, 512 and 1024 (NCH = 2, 4, 8, 16 of the shared 128 x 128
tile and of the rescore kernels; the other GPU tests of these calls all run at 768).  NCH = 2 has two K steps, the shortest
case of the double buffer.

One table of 300 rows per dim — two full tiles and a ragged one of 44 — with four planted near-duplicate pairs (inside a
tile, across tiles, into the ragged tile) and one deleted row, which is half of a planted pair.  130 vectors and 129 queries:
a full tile and a ragged one of 2 and of 1.  Oracle: orc_cosine_dist (oracle.c) at the dim, through the oracle helpers of
the four calls' own test files.  Ids are compared for equality and distances on their bits: there is no tolerance here."""
import numpy as np
import pytest

from image_search_amd.search import EmbeddingTable, ShardedTable, drop_self
from oracle.binding import orc_cosine_dist

import test_assign_gpu as asg
import test_assign_multi_gpu as amu
import test_density_host as dens
import test_join_between_gpu as btw
import test_join_gpu as join
import test_search_many_gpu as smy

pytestmark = pytest.mark.gpu

DIMS = [128, 256, 512, 1024]
N_ROWS, N_VEC, N_Q = 300, 130, 129
MAX_DIST = 0.05
PLANTED = [(5, 17), (3, 140), (130, 299), (100, 260)]   # (a, b): row b is row a, rescaled, plus a little noise
DELETED = 260
NO_ID = smy.NO_ID


def make(dim):
    """rows [300, dim], vectors [130, dim], queries [129, dim]"""
    rng = np.random.default_rng(1000 + dim)
    rows = rng.standard_normal((N_ROWS, dim)) * rng.uniform(0.1, 10.0, (N_ROWS, 1))
    for a, b in PLANTED:
        # noise of relative norm 0.1: a cosine distance near 0.005, a tenth of MAX_DIST, where two Gaussian rows lie at
        # 1 +- 1 / sqrt(dim) (at least ten standard deviations from MAX_DIST)
        rows[b] = (rows[a] + 0.1 * np.linalg.norm(rows[a]) / np.sqrt(dim) * rng.standard_normal(dim)) * rng.uniform(0.5, 2.0)
    rows = rows.astype(np.float32)
    vectors = rng.standard_normal((N_VEC, dim)).astype(np.float32)
    vectors[:40] += 2.0 * rows[np.arange(40) * 7] / np.linalg.norm(rows[np.arange(40) * 7], axis=1, keepdims=True) * np.sqrt(dim)
    vectors[129] = 0.5 * rows[299]            # the ragged tile's last row and the ragged column tile's last vector
    queries = rng.standard_normal((N_Q, dim)).astype(np.float32)
    queries[:32] += rows[np.arange(32) * 9] / np.linalg.norm(rows[np.arange(32) * 9], axis=1, keepdims=True) * np.sqrt(dim)
    queries[128] = rows[DELETED] * 3.0        # the ragged query tile: its nearest row is deleted, the next its planted twin
    return rows, vectors.astype(np.float32), queries.astype(np.float32)


def matrix(orc, queries, rows):
    return np.stack([orc_cosine_dist(orc, queries[q], rows) for q in range(queries.shape[0])])


@pytest.fixture(scope="module", params=DIMS, ids=lambda d: f"dim{d}")
def case(request, built, orc):
    """the table (row DELETED deleted) and the oracle's three distance matrices, computed once per dim"""
    dim = request.param
    rows, vectors, queries = make(dim)
    ref = {"dim": dim, "rows": rows, "vectors": vectors, "queries": queries, "live": np.ones(N_ROWS, bool),
           "self": matrix(orc, rows, rows), "vec": matrix(orc, rows, vectors), "query": matrix(orc, queries, rows)}
    ref["live"][DELETED] = False
    for m in (ref["self"], ref["vec"], ref["query"]):
        m.setflags(write=False)
    t = EmbeddingTable(dim, 0)
    t.insert(rows)
    assert t.delete([DELETED]) == 1
    yield t, ref
    t.close()


def test_near_pairs(case):
    t, ref = case
    want = join.oracle_join(ref["self"], MAX_DIST, live=ref["live"])
    pairs = set(zip(want[0].tolist(), want[1].tolist()))
    assert pairs == {p for p in PLANTED if DELETED not in p}, pairs   # the distance keeps the planted pairs, and only them
    join.same(t.near_pairs(MAX_DIST), want, f"dim {ref['dim']}")
    st = t.near_pairs_stats()
    assert st["pairs"] == 3 and st["tiles"] == 6 and st["candidates"] >= 3, st


def test_assign(case):
    t, ref = case
    want = asg.oracle_assign(ref["vec"], ref["live"])
    assert want[0][299] == 129 and want[0][DELETED] == asg.NO_LABEL
    asg.same(t.assign(ref["vectors"]), want, f"dim {ref['dim']}")
    st = t.assign_stats()
    assert st["rows"] == N_ROWS - 1 and st["tiles"] == 3 * 2 and st["candidates"] >= N_ROWS - 1, st


def test_assign_multi(case):
    t, ref = case
    want = amu.oracle_multi(ref["vec"], 4, live=ref["live"])
    amu.same(t.assign_multi(ref["vectors"], 4), want, f"dim {ref['dim']}")
    st = t.assign_multi_stats()
    assert st["hits"] == 4 * (N_ROWS - 1) and st["tiles"] == 3 * 2, st
    # with a threshold: the join's distance test in stage 1, dist <= max_dist in stage 2
    cut = float(np.median(want[1][ref["live"], 1]))
    amu.same(t.assign_multi(ref["vectors"], 4, cut), amu.oracle_multi(ref["vec"], 4, cut, ref["live"]), f"dim {ref['dim']}, max_dist {cut}")


def test_search_many(case):
    t, ref = case
    want = smy.oracle_many(ref["query"], 4, ref["live"])
    assert want[0][128, 0] == 100                                   # the deleted row's twin, not the deleted row
    got = t.knn_many(ref["queries"], 4)
    smy.same(got, want, f"dim {ref['dim']}")
    st = t.search_many_stats()
    assert st["hits"] == 4 * N_Q and st["tiles"] == 2 * (2 * 3), st   # threshold pass + emit pass
    # the documented equality with a loop of single searches
    for q0 in range(0, N_Q, 16):
        smy.same((got[0][q0:q0 + 16], got[1][q0:q0 + 16]), smy.strip_nan(*t.knn(ref["queries"][q0:q0 + 16], 4)), f"dim {ref['dim']}, queries from {q0}")


def test_neighbors(case):
    t, ref = case
    ids = np.arange(N_ROWS, dtype=np.uint64)
    want = drop_self(*smy.oracle_many(ref["self"], 3 + 1, ref["live"]), ids)
    want[0][DELETED], want[1][DELETED] = NO_ID, np.inf
    assert want[0][299, 0] == 130 and want[0][100, 0] != DELETED
    smy.same(t.neighbors(3), want, f"dim {ref['dim']}")


# ---- the threshold-pair calls beside the join: every one runs pair_tile / pair_dist (pair_kernels.h) at its NCH ------------

def dbscan_want(ref, max_dist, min_pts):
    """the host restatement (tests/test_density_host.py) fed with the oracle's pairs"""
    return dens.expected_dbscan(N_ROWS, *join.oracle_join(ref["self"], max_dist, live=ref["live"]), min_pts, live=ref["live"])


def same_bytes(x, y):
    return all(x[k].tobytes() == y[k].tobytes() for k in ("labels", "cluster", "via", "via_dist", "counts")) and x["summary"] == y["summary"]


def test_dbscan(case):
    t, ref = case
    want = dbscan_want(ref, MAX_DIST, 2)
    assert want[4] == [3, 6, 0, N_ROWS - 1 - 6]                     # the three live planted pairs: two cores each
    assert np.array_equal(t.neighbor_counts(MAX_DIST), want[3])
    dens.check_same(t.dbscan(MAX_DIST, 2), want, f"dim {ref['dim']}")
    st = t.dbscan_stats()
    assert st["pairs"] == 3 and st["tiles_pass1"] == 6 and st["tiles_visited"] + st["tiles_skipped"] == 6, st


def test_dbscan_levels(case):
    t, ref = case
    levels = [MAX_DIST / 2, MAX_DIST]
    got = t.dbscan_levels(levels, 2)
    for l, d in enumerate(levels):
        one = {k: got[k][l] for k in ("labels", "cluster", "via", "via_dist", "counts")}
        one["summary"] = got["summary"][l]
        dens.check_same(one, dbscan_want(ref, d, 2), f"dim {ref['dim']}, level {l}")
        assert same_bytes(one, t.dbscan(d, 2)), (ref["dim"], l)


def test_near_pairs_with(case):
    _, ref = case
    half, base_b = 150, 5000
    live_b = ref["live"][half:]
    want = btw.oracle_between(ref["self"][:half, half:], MAX_DIST, 0, base_b, live_b=live_b)
    assert list(zip(want[0].tolist(), want[1].tolist())) == [(130, base_b + 299 - half)]   # (100, 260) is gone with row 260
    for options in ({}, {"join_stage": 1, "join_stage_rows": 128}):   # direct, then staged in chunks of one tile
        ta, tb = EmbeddingTable(ref["dim"], 0), EmbeddingTable(ref["dim"], 0)
        ta.insert(ref["rows"][:half])
        tb.set_base(base_b)
        tb.insert(ref["rows"][half:])
        assert tb.delete([base_b + DELETED - half]) == 1
        for k, v in options.items():
            ta.set_option(k, v)
        btw.same(ta.near_pairs_with(tb, MAX_DIST), want, f"dim {ref['dim']}, {options}")
        st = ta.near_pairs_with_stats()
        assert st["pairs"] == 1 and st["tiles"] == 2 * 2 and st["launches"] == (2 if options else 1), st
        ta.close(); tb.close()


def test_sharded_dbscan(case):
    t, ref = case
    s = ShardedTable(ref["dim"], [0, 0], 128)
    s.insert(ref["rows"])
    assert s.delete([DELETED]) == 1
    got = s.dbscan(MAX_DIST, 2)
    dens.check_same(got, dbscan_want(ref, MAX_DIST, 2), f"dim {ref['dim']}")
    assert same_bytes(got, t.dbscan(MAX_DIST, 2)), ref["dim"]
    assert s.dbscan_stats()["pairs"] == 3
    s.close()


@pytest.mark.parametrize("dim", DIMS, ids=lambda d: f"dim{d}")
def test_dbscan_border_rows(built, orc, dim):
    """A chain a - b - c behind the rows of `case`: dist(a, b) = dist(b, c) = 1 - cos(0.245) = 0.030 and dist(a, c) =
    1 - cos(0.49) = 0.118 > MAX_DIST, so at min_pts = 3 row b is a core (two neighbours) and a, c are its border rows: the
    border keys (atomicMin of make_key) at this NCH."""
    rows = make(dim)[0]
    rng = np.random.default_rng(2000 + dim)
    b = rng.standard_normal(dim)
    u = rng.standard_normal(dim)
    u -= (u @ b) / (b @ b) * b
    u *= np.linalg.norm(b) / np.linalg.norm(u)                     # orthogonal to b, of b's length
    ang = 0.245
    chain = np.stack([np.cos(ang) * b + np.sin(ang) * u, b, np.cos(ang) * b - np.sin(ang) * u]) * np.array([[0.5], [1.0], [3.0]])
    rows = np.concatenate([rows, chain.astype(np.float32)])
    n, (ra, rb, rc) = rows.shape[0], range(N_ROWS, N_ROWS + 3)
    live = np.ones(n, bool)
    live[DELETED] = False
    D = matrix(orc, rows, rows)
    pairs = join.oracle_join(D, MAX_DIST, live=live)
    want = dens.expected_dbscan(n, *pairs, 3, live=live)
    cluster, via, via_dist, deg, summary = want
    assert deg[ra] == 1 and deg[rb] == 2 and deg[rc] == 1 and deg.max() == 2 and (deg == 2).sum() == 1   # b: the only core
    assert cluster[ra] == cluster[rb] == cluster[rc] == rb and via[ra] == rb and via[rc] == rb
    assert via_dist[ra] == D[ra, rb] and via_dist[rc] == D[rb, rc] and summary == [1, 1, 2, n - 1 - 3]
    t = EmbeddingTable(dim, 0)
    t.insert(rows)
    assert t.delete([DELETED]) == 1
    dens.check_same(t.dbscan(MAX_DIST, 3), want, f"dim {dim}")
    t.close()
