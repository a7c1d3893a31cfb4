"""The threshold self-join on the GPU (mi_knn_near_pairs): every pair of live rows a < b within a cosine distance, the
same ids and the same distance bits as the oracle's single pass with q = row a (oracle.c: orc_cosine_dist), thresholded
on that fp32 value."""
import ctypes
import os

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd._lib import MiError
from image_search_amd.search import EmbeddingTable, ImageIndex, pairs_to_groups
from oracle.binding import orc_cosine_dist

pytestmark = pytest.mark.gpu

DIM = 768
EPS2 = 2.0 ** -7 + 2.0 ** -16 + 4.1 * (DIM + 8) * 2.0 ** -24 + 2e-6
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5


def planted_corpus(n=4096, seed=7):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, DIM)).astype(np.float32)
    src = rng.integers(0, 2048, 320)
    scale = rng.uniform(0.1, 10.0, 320)
    sigma = np.concatenate([np.zeros(20), np.linspace(0.02, 0.32, 300)])
    noise = rng.standard_normal((320, DIM))
    rows[3000:3320] = ((rows[src] + sigma[:, None] * noise) * scale[:, None]).astype(np.float32)
    return rows


def distance_matrix(orc, rows):
    """D[a, b] = what the single pass with q = row a reports for row b"""
    return np.stack([orc_cosine_dist(orc, rows[a], rows) for a in range(rows.shape[0])])


def oracle_join(D, max_dist, live=None, first_new=0):
    n = D.shape[0]
    ok = np.triu(np.ones((n, n), bool), 1) & (D <= np.float32(max_dist))   # (a NaN compares false: never a pair)
    if live is not None:
        ok &= live[:, None] & live[None, :]
    ok[:, :first_new] = False
    a, b = np.nonzero(ok)   # row-major: ascending by (a, b)
    return a.astype(np.uint64), b.astype(np.uint64), D[a, b]


def same(got, want, what=""):
    ga, gb, gd = got
    wa, wb, wd = want
    assert ga.size == wa.size, (what, ga.size, wa.size)
    assert np.array_equal(ga, wa) and np.array_equal(gb, wb), what
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), what


@pytest.fixture(scope="module")
def corpus(built, orc):
    rows = planted_corpus()
    return rows, distance_matrix(orc, rows)


@pytest.fixture(scope="module")
def table(corpus):
    t = EmbeddingTable(DIM, 0)
    t.insert(corpus[0])
    yield t
    t.close()


# 1 + 3: the planted corpus at three thresholds; stage 1 really filters
def test_planted_corpus_equals_the_oracle_and_stage1_filters(corpus, table):
    rows, D = corpus
    n_band = {}
    for max_dist in (0.0, 0.02, 0.05):
        want = oracle_join(D, max_dist)
        got = table.near_pairs(max_dist)
        print(f"max_dist {max_dist}: {want[0].size} pairs, stats {table.near_pairs_stats()}")
        same(got, want, max_dist)
        st = table.near_pairs_stats()
        assert st["pairs"] == got[0].size
        # a candidate has coarse <= max_dist + eps2 and |coarse - exact| <= eps2: a consequence of the bound, not a tuned number
        in_band = oracle_join(D, max_dist + 2 * EPS2)[0].size
        assert got[0].size <= st["candidates"] <= in_band, (max_dist, st, in_band)
        n_band[max_dist] = (got[0].size, st["candidates"], in_band)
    # the planted structure is there: stage 2 both accepts and rejects inside the band, random rows enter at 0.05
    assert n_band[0.02][0] >= 150 and n_band[0.02][2] > n_band[0.02][0] and n_band[0.05][0] > n_band[0.02][0]
    assert n_band[0.02][2] < 4096 * 4095 // 2 // 1000


# 2: the same bits as the search
def test_pairs_carry_the_bits_of_the_search(corpus, table):
    rows, D = corpus
    a, b, d = table.near_pairs(0.05)
    pick = np.random.default_rng(1).choice(a.size, 32, replace=False)
    for j in pick:
        idx, dist = table.knn(rows[int(a[j])], 64)
        at = np.nonzero(idx == b[j])[0]
        assert at.size == 1, (int(a[j]), int(b[j]))
        assert dist[at[0]].view(np.uint32) == d[j].view(np.uint32)


# 4: shapes
def test_tiny_tables(built, orc):
    t = EmbeddingTable(DIM, 0)
    assert t.near_pairs(0.1)[0].size == 0
    row = np.random.default_rng(2).standard_normal((1, DIM)).astype(np.float32)
    t.insert(row)
    assert t.near_pairs(0.1)[0].size == 0
    t.insert(row)
    a, b, d = t.near_pairs(0.001)
    want = orc_cosine_dist(orc, row[0], row)
    assert a.tolist() == [0] and b.tolist() == [1] and d.view(np.uint32)[0] == want.view(np.uint32)[0]
    t.close()


def test_ragged_last_tile_and_growth(built, orc):
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((4096 + 37, DIM)).astype(np.float32)
    rows[4096 + 5] = rows[4000] * np.float32(3.0)                        # a in the last full tile, b in the ragged one
    rows[4096 + 30] = rows[4096 + 9] + np.float32(0.01) * rng.standard_normal(DIM).astype(np.float32)   # both in the ragged one
    rows[4096 + 36] = rows[17]                                           # the very last row
    t = EmbeddingTable(DIM, 0)
    t.insert(rows[:4096])
    assert t.near_pairs(0.03)[0].size == 0
    t.insert(rows[4096:])                                                # grown after a first join: the second sees the new rows
    D = distance_matrix(orc, rows)
    want = oracle_join(D, 0.03)
    assert {(4000, 4101), (4105, 4126), (17, 4132)} <= set(zip(want[0].tolist(), want[1].tolist()))
    same(t.near_pairs(0.03), want, "ragged")
    t.close()


# 5: first_new
def test_first_new(corpus, table):
    rows, D = corpus
    full = table.near_pairs(0.05)
    for first_new in (1000 + 77, 3000, 4095):
        keep = full[1] >= first_new
        want = (full[0][keep], full[1][keep], full[2][keep])
        same(want, oracle_join(D, 0.05, first_new=first_new), "the filtered full result is the oracle's")
        same(table.near_pairs(0.05, first_new=first_new), want, first_new)
    assert table.near_pairs(0.05, first_new=4096)[0].size == 0   # the table's end: no pairs
    with pytest.raises(MiError) as e:
        table.near_pairs(0.05, first_new=4097)
    assert e.value.code == MI_ERR_INVALID


# 6: deleted rows
def test_deleted_rows_are_left_out(corpus, orc):
    rows, D = corpus
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    full = t.near_pairs(0.05)
    rng = np.random.default_rng(4)
    planted = rng.choice(np.arange(3000, 3320), 50, replace=False)
    sources = np.unique(full[0][np.isin(full[1], np.arange(3000, 3320)) & (full[0] < 2048)])
    sources = rng.choice(sources, 50, replace=False)
    gone = np.concatenate([planted, sources]).astype(np.uint64)
    assert t.delete(gone) == 100
    live = np.ones(rows.shape[0], bool)
    live[gone.astype(np.int64)] = False
    got = t.near_pairs(0.05)
    same(got, oracle_join(D, 0.05, live=live), "deleted")
    keep = ~np.isin(full[0], gone) & ~np.isin(full[1], gone)
    same(got, (full[0][keep], full[1][keep], full[2][keep]), "the full result minus the deleted ids")
    assert got[0].size < full[0].size
    t.close()


# 7: special rows
def test_special_rows(built, orc):
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((300, DIM)).astype(np.float32)
    rows[10] = 0.0; rows[200] = 0.0                              # a zero row and its copy: NaN, never a pair
    rows[20, 5] = np.float32(3.2e38); rows[210] = rows[20]       # marked: an element bf16 would round to inf
    rows[30, 7] = np.inf                                         # marked: an inf
    direction = rng.standard_normal(DIM).astype(np.float32)
    rows[40] = direction * np.float32(1e-17)                     # squared norms 7.7e-32 and 7.7e34: both marked,
    rows[220] = direction * np.float32(1e16)                     # both finite in fp32: a pair the join must find
    rows[250] = rows[100] * np.float32(2.0)                      # and an ordinary pair beside them
    D = distance_matrix(orc, rows)
    assert D[40, 220] <= np.float32(0.01), D[40, 220]            # the oracle does report them as a pair
    assert not (D[10, 200] <= np.float32(2.0))
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    for max_dist in (0.01, 1.5):
        want = oracle_join(D, max_dist)
        got = t.near_pairs(max_dist)
        same(got, want, max_dist)
        pairs = set(zip(got[0].tolist(), got[1].tolist()))
        assert (40, 220) in pairs and (100, 250) in pairs and (10, 200) not in pairs
    t.close()


# 8: the cap
def test_cap_stops_the_call_and_leaves_the_handle_usable(corpus, table):
    rows, D = corpus
    before = table.knn(rows[5], 10)
    a = np.empty(1000, np.uint64); b = np.empty(1000, np.uint64); d = np.empty(1000, np.float32)
    n = ctypes.c_uint64()
    rc = _lib.lib().mi_knn_near_pairs(table._h, 2.0, 0, a.ctypes.data, b.ctypes.data, d.ctypes.data, 1000, ctypes.byref(n))
    assert rc == MI_ERR_UNSUPPORTED and n.value == 1001
    assert b"cap" in _lib.lib().mi_last_error()
    after = table.knn(rows[5], 10)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    rc = _lib.lib().mi_knn_near_pairs(table._h, 0.0, 3500, None, None, None, 0, ctypes.byref(n))   # no pairs among the random tail
    assert rc == 0 and n.value == 0


# 9: the overflow path
def test_everything_is_a_duplicate(built, orc):
    n = 6000
    row = np.random.default_rng(6).standard_normal(DIM).astype(np.float32)
    t = EmbeddingTable(DIM, 0)
    t.insert(np.tile(row, (n, 1)))
    t.set_option("join_cap", 1 << 16)   # one tile row holds 128 x 6000 candidates: column ranges are needed
    a, b, d = t.near_pairs(0.001, cap=1 << 25)
    st = t.near_pairs_stats()
    print("all duplicates:", st)
    assert a.size == n * (n - 1) // 2 == st["pairs"] == st["candidates"]
    ia, ib = np.triu_indices(n, 1)   # ascending by (a, b)
    assert np.array_equal(a, ia.astype(np.uint64)) and np.array_equal(b, ib.astype(np.uint64))
    want = orc_cosine_dist(orc, row, row[None])   # every pair is (row, row)
    assert np.all(d.view(np.uint32) == want.view(np.uint32)[0])
    n_tile_rows = (n + 127) // 128
    assert st["strips"] > n_tile_rows   # more launches than tile rows: tile rows were cut into column ranges
    t.close()


# 10: scale
def test_three_hundred_thousand_rows(built, orc):
    n, n_planted = 300_000, 200
    t = EmbeddingTable(DIM, 0)
    t.insert_synthetic(11, 0, n)
    rng = np.random.default_rng(11)
    src = np.sort(rng.choice(n, n_planted, replace=False))
    base = np.stack([t.rows(int(r), 1)[0] for r in src])
    sigma = np.linspace(0.0, 0.4, n_planted)
    planted = ((base + sigma[:, None] * np.abs(base).mean() * rng.standard_normal((n_planted, DIM)))
               * rng.uniform(0.1, 10.0, (n_planted, 1))).astype(np.float32)
    t.insert(planted)
    # unplanted pairs of i.i.d. rows lie at distance >= 0.7: the expected result is the oracle's pairs of the planted rows
    # against all rows
    pa, pb, pd = [], [], []
    unit = planted / np.linalg.norm(planted, axis=1, keepdims=True)
    for first in range(0, n + n_planted, 50_000):
        blk = t.rows(first, min(50_000, n + n_planted - first))
        # where to look: a plain fp32 product, a margin of 0.01 around the threshold (its own error is below 1e-5)
        approx = 1.0 - (blk / np.linalg.norm(blk, axis=1, keepdims=True)) @ unit.T
        for r, j in zip(*np.nonzero(approx <= 0.06)):
            a, b = first + int(r), n + int(j)
            if a >= b:
                continue
            d = orc_cosine_dist(orc, blk[r], planted[j][None])[0]   # the smaller id is the query
            if d <= np.float32(0.05):
                pa.append(a); pb.append(b); pd.append(d)
    order = np.lexsort((pb, pa))
    want = (np.array(pa, np.uint64)[order], np.array(pb, np.uint64)[order], np.array(pd, np.float32)[order])
    assert 50 <= want[0].size < 2 * n_planted
    got = t.near_pairs(0.05)
    print("300 k rows:", t.near_pairs_stats())
    same(got, want, "own mirror")
    for prefilter in (1, 2):
        t.set_option("prefilter", prefilter)
        same(t.near_pairs(0.05), want, f"prefilter {prefilter}")
        same(t.near_pairs(0.05), want, f"prefilter {prefilter}, again")   # (with 1: the table's mirror, now built)
    t.close()


# 11: the index
def test_index_duplicates(built, tmp_path):
    rng = np.random.default_rng(12)
    media = str(tmp_path / "media") + "/"   # (rows store media_dir + <rel>)
    names = [f"{media}{folder}/{i}.jpg" for folder in ("a", "b", "c") for i in range(40)]
    emb = rng.standard_normal((120, DIM)).astype(np.float32)
    unit = emb / np.linalg.norm(emb, axis=1, keepdims=True)
    emb[45] = emb[3] * np.float32(2.0)            # a/3 ~ b/5
    emb[100] = emb[3]                             # a/3 ~ c/20
    # a transitive group: 50 ~ 60 and 60 ~ 70 at distance 0.0075, 50 and 70 at 0.03 (angles t, 2 t with cos 2t = 0.97)
    u = unit[50]
    v = unit[51] - np.dot(unit[51], u) * u
    v /= np.linalg.norm(v)
    t2 = np.arccos(0.97)
    emb[60] = (np.cos(t2 / 2) * u + np.sin(t2 / 2) * v).astype(np.float32)
    emb[70] = (np.cos(t2) * u + np.sin(t2) * v).astype(np.float32)
    ix = ImageIndex(DIM, 0, media)
    ix.insert(names, emb)
    a, b, d = ix.table.near_pairs(0.02)
    assert (50, 70) not in set(zip(a.tolist(), b.tolist())) and abs(1.0 - float(np.dot(emb[50] / np.linalg.norm(emb[50]), emb[70])) - 0.03) < 1e-3
    want = [[names[3], names[45], names[100]], [names[50], names[60], names[70]]]
    assert ix.duplicates(0.02) == want
    assert [[int(i) for i in g] for g in pairs_to_groups(a, b)] == [[3, 45, 100], [50, 60, 70]]
    assert ix.duplicates(0.02, web=True)[0] == ["media/a/3.jpg", "media/b/5.jpg", "media/c/20.jpg"]
    assert ix.duplicates(0.02, first_new=100) == [[names[3], names[45], names[100]]]   # (3, 100) and (45, 100)
    ix.save(str(tmp_path / "saved"))
    ix.remove([names[60], names[45]])
    assert ix.duplicates(0.02) == [[names[3], names[100]]]   # one group shrinks, the chain falls apart
    ix.remove([names[100]])
    assert ix.duplicates(0.02) == []
    back = ImageIndex.load(str(tmp_path / "saved"))
    assert back.duplicates(0.02) == want
    back.close()
    ix.close()


# 12: concurrency and order
def test_join_behind_an_append_on_another_stream(built, orc):
    import torch
    rng = np.random.default_rng(13)
    rows = rng.standard_normal((20_500, DIM)).astype(np.float32)
    rows[20_100] = rows[77] * np.float32(0.5)
    rows[20_499] = rows[20_001]
    t = EmbeddingTable(DIM, 0)
    t.insert(rows[:20_000])
    q = rows[123]
    before = t.knn(q, 10)
    assert t.near_pairs(0.01)[0].size == 0
    d_new = torch.from_numpy(rows[20_000:].copy()).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t.insert_device(d_new.data_ptr(), 500, s.cuda_stream)   # enqueued on s, not waited for
    a, b, d = t.near_pairs(0.01)
    s.synchronize()
    assert list(zip(a.tolist(), b.tolist())) == [(77, 20_100), (20_001, 20_499)]
    assert d[0].view(np.uint32) == orc_cosine_dist(orc, rows[77], rows[20_100][None]).view(np.uint32)[0]
    after = t.knn(q, 10)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    t.close()
