"""Filtered search (mi_knn_search_filtered, mi_knn_sharded_search_filtered, mi_index_search_within) on a real MI355X.
The oracle is orc_knn over the filter's live rows, `rows[sub]` with sub = the filter's rows ascending, each result
ordinal mapped back to its id (sub[ordinal]: ids are monotone in the ordinal, so ties keep their order).
Bar: bit-exact ids and distance bits."""
import numpy as np
import pytest

from image_search_amd import synth
from image_search_amd._lib import MiError
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable
from oracle.binding import orc_knn

pytestmark = pytest.mark.gpu
NO_ID = 0xFFFFFFFFFFFFFFFF
N = 20_000
KS = [1, 10, 64, 65, 1000, 4096]


def _oracle(orc, q, rows, sub, k, base=0):
    """the answer of a table that holds only rows[sub] under their own ids (sub ascending, unique)"""
    sub = np.asarray(sub, np.int64)
    ids = np.full(k, NO_ID, np.uint64)
    if sub.size == 0:
        return ids, np.full(k, np.inf, np.float32)
    oi, od = orc_knn(orc, q, rows[sub], k)
    m = oi != NO_ID
    ids[m] = sub[oi[m].astype(np.int64)].astype(np.uint64) + np.uint64(base)
    return ids, od


def _same(got, want, what=""):
    gi, gd = got
    oi, od = want
    assert np.array_equal(gi, oi), (what, np.nonzero(gi != oi)[0][:5], gi[:4], oi[:4])
    assert np.array_equal(gd.view(np.uint32), od.view(np.uint32)), what


@pytest.fixture(scope="module")
def table_rows():
    """20 k rows with exact ties (duplicate rows), a NaN row and a zero row"""
    rows = synth.corpus_rows(81, 0, N).copy()
    rows[[100, 5000, 19_999]] = rows[77]                  # duplicates of row 77: equal distances, ties by id
    rows[[3, 4]] = rows[12_345]
    rows[250, 17] = np.nan                                # NaN distance: ranks last
    rows[251] = 0.0                                       # zero row: 0 / 0, NaN
    qs = np.concatenate([rows[[77, 12_345]], synth.corpus_rows(1081, 0, 14)])
    return rows, qs


def _filters(rng):
    scattered = np.sort(rng.choice(N, 3000, replace=False))
    mixed = np.concatenate([rng.choice(N, 500), [77, 100, 5000, 19_999, 3, 4, 12_345, 250, 251]])
    return {
        "empty": np.zeros(0, np.int64),
        "one": np.array([5000]),
        "0.1pct": rng.choice(N, N // 1000, replace=False),
        "10pct": rng.choice(N, N // 10, replace=False),
        "run": np.arange(6000, 8100),
        "scattered": scattered,
        "unsorted_dups": rng.permutation(np.concatenate([mixed, mixed[:200]])),   # duplicates, any order, ties + NaN inside
        "all": np.arange(N),
    }


def test_filters_against_the_oracle(built, orc, table_rows):
    rows, qs = table_rows
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    for name, f in _filters(np.random.default_rng(8)).items():
        sub = np.unique(f)
        for k in KS:
            want = [_oracle(orc, q, rows, sub, k) for q in qs]
            _same(t.knn(qs[0], k, within=f), want[0], (name, k))
            gi, gd = t.knn(qs, k, within=f)                 # nq = 16: groups of 8 for k <= 64, one by one above
            for u in range(16):
                _same((gi[u], gd[u]), want[u], (name, k, u))
    t.close()


def test_lds_lists(built, orc, table_rows, monkeypatch):
    """64 < k <= 1024 through the per-wave LDS lists (a handle made with MI_KNN_SELECT=0 takes them for every n)"""
    rows, qs = table_rows
    monkeypatch.setenv("MI_KNN_SELECT", "0")
    t = EmbeddingTable(768, 0)
    monkeypatch.delenv("MI_KNN_SELECT")
    t.insert(rows)
    for name, f in _filters(np.random.default_rng(9)).items():
        sub = np.unique(f)
        for k in (65, 256, 257, 1000, 1024, 1500):
            for u in (0, 1, 5):
                _same(t.knn(qs[u], k, within=f), _oracle(orc, qs[u], rows, sub, k), (name, k, u))
    t.close()


def test_many_tiles_per_wave(built, monkeypatch):
    """2.2 M filtered rows: every wave of the gathered scan walks 8 to 17 tiles (the next tile's entries loaded a tile ahead,
    the LDS lists merging while they are offered keys).  The reference is the unfiltered search of a second table that
    holds the same rows with every row outside the filter deleted (tests/test_delete_gpu.py checks it against the oracle)."""
    n = 2_500_000
    rng = np.random.default_rng(14)
    keep = rng.permutation(n)[:2_200_000]
    drop = np.setdiff1d(np.arange(n), keep).astype(np.uint64)
    qs = synth.corpus_rows(1088, 0, 2)
    ref = EmbeddingTable(768, 0)
    ref.insert_synthetic(88, 0, n)
    ref.delete(drop)
    monkeypatch.setenv("MI_KNN_SELECT", "0")               # 64 < k <= 1024 through the LDS lists
    lists = EmbeddingTable(768, 0)
    monkeypatch.delenv("MI_KNN_SELECT")
    lists.insert_synthetic(88, 0, n)
    plain = EmbeddingTable(768, 0)                          # the default rule: radix select above k = 64
    plain.insert_synthetic(88, 0, n)
    for k in (10, 64, 65, 300, 1000, 2000):
        want = ref.knn(qs, k)
        for t in (lists, plain):
            _same(t.knn(qs, k, within=keep), want, k)
    for t in (ref, lists, plain):
        t.close()


def test_small_filters_with_deleted_ids(built, orc, table_rows):
    """fewer ids than rows / 1024 take the sorted list (sort, unique, minus the deleted rows); from rows / 1024 on the bitmap"""
    rows, qs = table_rows
    base = 7
    t = EmbeddingTable(768, 0, base=base)
    t.insert(rows)
    dead = np.array([40, 41, 77, 19_999])
    t.delete(dead + base)
    for f in (np.array([77, 40, 41, 19_999, 5, 5, 9_000, 77, 3, 12_345, 100, 251, 250, 41]),   # 14 ids < 20 000 / 1024
              np.array([77, 40, 41, 19_999, 5, 9_000, 3, 12_345, 100, 251, 250, 4, 6, 8, 10, 12, 14, 16, 18, 20]),   # 20 ids
              np.array([40, 41])):                                                       # nothing but deleted rows
        sub = np.setdiff1d(np.unique(f), dead)
        for k in (1, 5, 64, 65, 1000):
            for u in (0, 1, 3):
                _same(t.knn(qs[u], k, within=f + base), _oracle(orc, qs[u], rows, sub, k, base), (f.size, k, u))
    t.close()


def test_full_filter_equals_the_unfiltered_search(built):
    n = 300_000                                           # above the two-stage search's minimum (2^18 rows)
    qs = synth.corpus_rows(1082, 0, 3)
    every = np.arange(n)
    for prefilter in (0, 1, 2):
        t = EmbeddingTable(768, 0)
        t.insert_synthetic(82, 0, n)
        t.set_option("prefilter", prefilter)
        t.set_option("prefilter_adaptive", 0)
        for k in (10, 1000):
            _same(t.knn(qs, k, within=every), t.knn(qs, k), (prefilter, k))
        t.close()


def test_deleted_rows_base_and_errors(built, orc, table_rows):
    rows, qs = table_rows
    base = 1_000_000
    t = EmbeddingTable(768, 0, base=base)
    t.insert(rows)
    f = np.arange(1000, 4000)
    dead = np.concatenate([np.arange(1000, 1100), orc_knn(orc, qs[2], rows[1000:4000], 50)[0].astype(np.int64) + 1000])
    t.delete(dead + base)
    sub = np.setdiff1d(f, dead)
    for k in (10, 64, 1000):
        _same(t.knn(qs[2], k, within=f + base), _oracle(orc, qs[2], rows, sub, k, base), k)
    # every id is checked before anything runs: one that is no row of the table fails the call
    for bad in ([base - 1], [base + N], [base, base + N + 5]):
        with pytest.raises(MiError) as e:
            t.knn(qs[2], 10, within=bad)
        assert e.value.code == -1, bad
    _same(t.knn(qs[2], 10, within=f + base), _oracle(orc, qs[2], rows, sub, 10, base), "after the error")
    with pytest.raises(MiError) as e:
        t.knn(qs[2], 4097, within=f + base)
    assert e.value.code == -5
    _same(t.knn(qs[2], 4096, within=f + base), _oracle(orc, qs[2], rows, sub, 4096, base), 4096)
    t.close()


def test_groups_equal_single_calls(built, table_rows):
    rows, qs = table_rows
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    rng = np.random.default_rng(10)
    for f in (rng.choice(N, 700, replace=False), np.arange(N), np.array([9, 8, 7])):
        for k in (1, 10, 64):
            one = [t.knn(q, k, within=f) for q in qs]
            for nq in (2, 3, 4, 5, 8, 16):
                gi, gd = t.knn(qs[:nq], k, within=f)
                for u in range(nq):
                    _same((gi[u], gd[u]), one[u], (len(f), k, nq, u))
    t.close()


def test_writes_on_other_streams_are_seen(built, orc):
    """a delete and an append enqueued before a filtered search (on another stream) are both honoured"""
    import torch
    n = 20_000
    rows = synth.corpus_rows(83, 0, n + 500)
    t = EmbeddingTable(768, 0)
    t.insert(rows[:n])
    q = rows[n + 10]
    d_q = torch.from_numpy(q[None].copy()).cuda()
    d_new = torch.from_numpy(rows[n:].copy()).cuda()
    s = torch.cuda.Stream()
    a_i = torch.zeros((1, 5), dtype=torch.int64, device="cuda"); a_d = torch.zeros((1, 5), dtype=torch.float32, device="cuda")
    with torch.cuda.stream(s):
        t.knn_device(d_q.data_ptr(), 1, 5, a_i.data_ptr(), a_d.data_ptr(), s.cuda_stream)
        t.insert_device(d_new.data_ptr(), 500, s.cuda_stream)   # enqueued on s, not waited for
        t.delete([n + 11])
        got = t.knn(q, 20, within=np.arange(n - 2000, n + 500))
    s.synchronize()
    sub = np.setdiff1d(np.arange(n - 2000, n + 500), [n + 11])
    _same(got, _oracle(orc, q, rows, sub, 20), "ordered")
    assert int(got[0][0]) == n + 10
    t.close()


def _oracle_sub(orc, q, sub_rows, sub, k):
    """_oracle with only the filter's rows at hand (sub ascending, sub_rows = rows[sub])"""
    oi, od = orc_knn(orc, q, sub_rows, k)
    ids = np.full(k, NO_ID, np.uint64)
    m = oi != NO_ID
    ids[m] = sub[oi[m].astype(np.int64)].astype(np.uint64)
    return ids, od


@pytest.mark.parametrize("n,frac,seed", [(1_000_000, 1000, 84), (10_000_000, 10_000, 85)])
def test_synthetic_tables_at_scale(built, orc, n, frac, seed):
    """1 M rows with a 0.1 % filter and 10 M rows with a 0.01 % filter (same seed on both sides)"""
    t = EmbeddingTable(768, 0)
    t.insert_synthetic(seed, 0, n)
    rng = np.random.default_rng(seed)
    sub = np.sort(rng.choice(n, n // frac, replace=False))
    sub_rows = np.stack([synth.corpus_rows(seed, int(r), 1)[0] for r in sub])
    qs = synth.corpus_rows(1000 + seed, 0, 2)
    for k in (10, 1000):
        for q in qs:
            _same(t.knn(q, k, within=rng.permutation(sub)), _oracle_sub(orc, q, sub_rows, sub, k), (n, k))
    t.close()


def test_sharded_filtered_equals_one_table(built, orc, table_rows, monkeypatch):
    rows, qs = table_rows
    one = EmbeddingTable(768, 0)
    one.insert(rows)
    rng = np.random.default_rng(13)
    dead = rng.choice(N, 300, replace=False)
    one.delete(dead)
    filters = [np.zeros(0, np.int64), np.array([19_999]), rng.choice(N, 900), np.arange(2000, 9000), np.arange(N)]
    want = {(j, k): one.knn(qs[:3], k, within=f) for j, f in enumerate(filters) for k in (10, 1000)}
    for j, f in enumerate(filters):
        sub = np.setdiff1d(np.unique(f), dead)
        _same((want[j, 10][0][0], want[j, 10][1][0]), _oracle(orc, qs[0], rows, sub, 10), j)
    tables = [ShardedTable(768, [0] * n_sh, block) for n_sh, block in ((1, 0), (2, 512), (3, 256), (8, 1024))]
    monkeypatch.setenv("MI_KNN_SHARDED_TRANSPORT", "rccl")
    tables.append(ShardedTable(768, [0], 0))
    monkeypatch.delenv("MI_KNN_SHARDED_TRANSPORT")
    assert tables[-1].info()["transport"] == "rccl all-gather"
    for sh in tables:
        sh.insert(rows)
        sh.delete(dead)
        for j, f in enumerate(filters):
            for k in (10, 1000):
                _same(sh.knn(qs[:3], k, within=f), want[j, k], (sh.info()["shards"], j, k))
        with pytest.raises(MiError) as e:
            sh.knn(qs[0], 10, within=[N])
        assert e.value.code == -1
        sh.close()
    one.close()


def test_index_search_within_folders(built, orc, tmp_path):
    dim = 768
    folders = ["2024/trip", "2024/trip/day2", "2024/tripb", "2024", "2023", "other"]
    paths, rows = [], []
    for j, fo in enumerate(folders):
        for i in range(60):
            paths.append(f"/m/{fo}/img{i}.jpg")
    rows = synth.corpus_rows(86, 0, len(paths))
    ix = ImageIndex(dim, 0, "/m/")
    ix.insert(paths, rows)
    ix.remove(["/m/2024/trip/img5.jpg"])
    q = synth.corpus_rows(1086, 0, 1)[0]

    def expect(prefixes, k, refs=()):
        from image_search_amd.search import refine_query
        sub = [i for i, p in enumerate(paths) if any(p.startswith(pr) for pr in prefixes) and p != "/m/2024/trip/img5.jpg"]
        marked = [rows[i] for i, p in enumerate(paths) if "media/" + p[3:] in refs]
        qq = refine_query(q, marked) if marked else q
        i, d = _oracle(orc, qq, rows, np.array(sub, np.int64), k)
        return [(int(a), float(b)) for a, b in zip(i, d) if a != NO_ID]

    def got(res):
        return [(r[0], r[2]) for r in res]

    for fs, prefixes in ((["media/2024/trip"], ["/m/2024/trip/"]),                      # nested, not the sibling 2024b
                         (["media/2024/trip/"], ["/m/2024/trip/"]),
                         (["media/2024"], ["/m/2024/"]),
                         (["media/2024/tripb", "media/2023"], ["/m/2024/tripb/", "/m/2023/"]),
                         (["media/2024/trip/day2", "media/2024/trip"], ["/m/2024/trip/"]),  # overlapping folders: rows once
                         (["media/nothing", "elsewhere/2024"], [])):
        for k in (5, 1000):
            assert got(ix.web_search_text(q, (), k, folders=fs)) == expect(prefixes, k), (fs, k)
    refs = ["media/other/img3.jpg", "media/2023/img1.jpg"]            # marked images outside the folder still refine
    assert got(ix.web_search_text(q, refs, 10, folders=["media/2024/trip"])) == expect(["/m/2024/trip/"], 10, refs)
    assert ix.web_search_text(q, refs, 50, folders=["media/"]) == ix.web_search_text(q, refs, 50)
    assert ix.web_search_text(q, (), 3, folders=[]) == []
    ix.save(str(tmp_path / "ix"))
    ix2 = ImageIndex.load(str(tmp_path / "ix"), 0, dim)
    assert got(ix2.web_search_text(q, (), 100, folders=["media/2024/trip"])) == expect(["/m/2024/trip/"], 100)
    new = synth.corpus_rows(87, 0, 1)
    ix2.insert(["/m/2024/trip/new.jpg"], new)                    # an insert joins its folder
    assert ix2.web_search_text(new[0], (), 1, folders=["media/2024/trip"])[0][0] == len(paths)
    ix2.remove(["/m/2024/trip/new.jpg"])                          # a remove leaves it
    assert len(paths) not in [r[0] for r in ix2.web_search_text(new[0], (), 200, folders=["media/2024/trip"])]
    ix.close(); ix2.close()
