"""mi_knn_search_where and its kin on the GPU.  The row lists (mi_knn_rows_where) are compared with the numpy restatement
(tests/test_where_host.py: where_rows) for equality; the search with mi_knn_search_filtered over those ids — ids, distance BITS,
padding — and once with the CPU oracle's distances directly.  Integers and bits only: no tolerance anywhere."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable, refine_query
from oracle.binding import orc_cosine_dist
from test_page_host import NO_ID, bits, expected_page
from test_where_host import BIT63, I64_MAX, I64_MIN, NO_GROUP, as_kwargs, where_rows

pytestmark = pytest.mark.gpu

HALF = {"all_of": 1}                    # one random bit: about half the rows
PERCENT = {"all_of": 0x7F}              # seven random bits: about 0.8 %
NOTHING_RUN = {"stamp_lo": 5000}        # no row has it, but only the kernels can tell
NOTHING_SEEN = {"stamp_lo": 1, "stamp_hi": 0}   # lo > hi: refused without a launch


def columns(n, seed):
    rng = np.random.default_rng(seed)
    tags = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)   # all 64 bits random
    stamps = rng.integers(-1000, 1001, n, dtype=np.int64)
    return tags, stamps


def table(n, seed=3, dim=64, tags=None, stamps=None):
    t = EmbeddingTable(dim, 0)
    t.insert(np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32))
    if tags is not None or stamps is not None:
        t.set_attrs(np.arange(n), tags, stamps)
    return t


def check_rows(t, tags, stamps, groups, dead, where, what=""):
    """rows_where and count_where against the restatement; returns the rows"""
    want = where_rows(tags, stamps, groups, dead, dict(where, n=len(t)))
    got = t.rows_where(**as_kwargs(where))
    assert got.dtype == np.uint64 and np.array_equal(got, want), (what, where, got[:8], want[:8], got.size, want.size)
    assert t.count_where(**as_kwargs(where)) == want.size, (what, where)
    return want


# ---- 1. chunk and tile edges ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_chunk_and_tile_edges(built, n):
    tags, stamps = columns(n, n)
    t = table(n, tags=tags, stamps=stamps)
    for chunk in (64, 256, 0):
        t.set_option("where_chunk", chunk)
        check_rows(t, tags, stamps, None, (), HALF, (n, chunk))
        check_rows(t, tags, stamps, None, (), {"stamp_lo": -100, "stamp_hi": 400, "none_of": 2}, (n, chunk))
        check_rows(t, tags, stamps, None, (), {}, (n, chunk))
    for bad in (-64, 1, 100, 65600):
        with pytest.raises(_lib.MiError):
            t.set_option("where_chunk", bad)
    t.close()


# ---- 2. more chunks than the offsets kernel has threads --------------------------------------------------------------------------------

def test_more_chunks_than_the_offsets_kernel_has_threads(built):
    n = 70000                                                 # 1 094 chunks of 64 rows: the scan's second round, with its carry
    tags, stamps = columns(n, 17)
    t = table(n, tags=tags, stamps=stamps)
    lists = {}
    for chunk in (64, 0):
        t.set_option("where_chunk", chunk)
        for name, where in (("1 %", PERCENT), ("50 %", HALF), ("all", {}), ("none, counted", NOTHING_RUN), ("none, seen", NOTHING_SEEN)):
            rows = check_rows(t, tags, stamps, None, (), where, (name, chunk))
            lists.setdefault(name, rows)
            assert np.array_equal(rows, lists[name])          # the same list for any grid
    assert 300 < lists["1 %"].size < 900 and 33000 < lists["50 %"].size < 37000
    assert lists["all"].size == n and lists["none, counted"].size == 0 and lists["none, seen"].size == 0
    # cap below the count: the first ids, the whole count
    w = _lib.KnnWhere(1, 0, 0, I64_MIN, I64_MAX, 0, 0)
    ids, cnt = np.full(12, 7, np.uint64), ctypes.c_uint64()
    assert _lib.lib().mi_knn_rows_where(t._h, w, ids.ctypes.data, 10, ctypes.byref(cnt)) == 0
    assert cnt.value == lists["50 %"].size and np.array_equal(ids[:10], lists["50 %"][:10]) and np.all(ids[10:] == 7)
    t.close()


# ---- 3. signed compare ------------------------------------------------------------------------------------------------------------

def test_signed_stamps_their_extremes_and_tag_bit_63(built):
    n = 300
    rng = np.random.default_rng(5)
    stamps = rng.integers(-50, 51, n, dtype=np.int64)
    stamps[[0, 64, 130]] = I64_MIN
    stamps[[1, 63, 131]] = I64_MIN + 1
    stamps[[2, 65, 299]] = I64_MAX
    stamps[[3, 127, 298]] = I64_MAX - 1
    tags = rng.integers(0, 4, n, dtype=np.uint64)
    tags[::3] |= np.uint64(BIT63)
    t = table(n, tags=tags, stamps=stamps)
    t.set_option("where_chunk", 64)
    for where in ({"stamp_lo": I64_MIN, "stamp_hi": I64_MIN}, {"stamp_lo": I64_MIN + 1}, {"stamp_hi": I64_MIN + 1}, {"stamp_hi": -1},
                  {"stamp_lo": 0}, {"stamp_lo": -1, "stamp_hi": 0}, {"stamp_lo": I64_MAX}, {"stamp_lo": I64_MAX - 1}, {"stamp_hi": I64_MAX - 1},
                  {"stamp_lo": I64_MIN, "stamp_hi": I64_MAX}, {"stamp_lo": I64_MAX, "stamp_hi": I64_MIN}, {"all_of": BIT63},
                  {"any_of": BIT63}, {"none_of": BIT63}, {"all_of": BIT63 | 1, "none_of": 2, "stamp_hi": -1}):
        rows = check_rows(t, tags, stamps, None, (), where)
        if where == {"stamp_hi": -1}:
            assert 0 in rows and 2 not in rows                # INT64_MIN is below -1, INT64_MAX is not: a signed compare
    t.close()


# ---- 4. deleted rows ----------------------------------------------------------------------------------------------------------------

def test_deleted_rows_are_left_out(built):
    n = 1000
    tags, stamps = columns(n, 23)
    t = table(n, tags=tags, stamps=stamps)
    t.set_option("where_chunk", 64)
    for where in (HALF, {}):
        check_rows(t, tags, stamps, None, (), where, "before")
    dead = list(range(128, 192)) + [0, 63, 64, 500, 999]      # a whole chunk, and rows at chunk edges
    t.delete(dead)
    for chunk in (64, 0):
        t.set_option("where_chunk", chunk)
        for where in (HALF, {}, {"stamp_lo": 0}):
            rows = check_rows(t, tags, stamps, None, dead, where, ("after", chunk))
            assert not np.isin(rows, dead).any()
    t.set_attrs([130, 500], [1, 1], [0, 0])                   # a deleted row may be set and read, and stays out
    tags[[130, 500]], stamps[[130, 500]] = 1, 0
    assert t.get_attrs([130, 500])[0].tolist() == [1, 1]
    check_rows(t, tags, stamps, None, dead, HALF, "set while deleted")
    t.close()


# ---- 5. the group flag -------------------------------------------------------------------------------------------------------------

def test_the_group_flag(built):
    n = 700
    tags, stamps = columns(n, 29)
    t = table(n, tags=tags, stamps=stamps)
    t.set_option("where_chunk", 64)
    for g in (0, 1, NO_GROUP):                                # no column: nothing under the flag, whatever the value
        assert check_rows(t, tags, stamps, None, (), {"group": g}).size == 0
    groups = (np.arange(n) % 5).astype(np.uint32)
    groups[::7] = NO_GROUP
    groups[64:128] = 9
    t.set_groups(groups)
    for where in ({"group": 1}, {"group": 9}, {"group": NO_GROUP}, {"group": 77}, {"group": 3, "all_of": 1}, {"group": NO_GROUP, "stamp_lo": 0}, HALF):
        check_rows(t, tags, stamps, groups, (), where)
    assert check_rows(t, tags, stamps, groups, (), {"group": 9}).tolist() == list(range(64, 128))
    t.delete([70, 0])
    check_rows(t, tags, stamps, groups, (70, 0), {"group": 9})
    check_rows(t, tags, stamps, groups, (70, 0), {"group": NO_GROUP})
    t.close()


# ---- 6. the search contract, to the bit ------------------------------------------------------------------------------------------------

N6 = 20000


@pytest.fixture(scope="module")
def corpus(built):
    rng = np.random.default_rng(2031)
    rows = rng.standard_normal((N6, 768)).astype(np.float32)
    qs = (rows[[70, 900, 4000, 12000, 19999, 5, 6, 7]] + 0.7 * rng.standard_normal((8, 768))).astype(np.float32)
    tags, _ = columns(N6, 41)
    stamps = rng.permutation(N6).astype(np.int64)             # every stamp once: a range of m stamps keeps exactly m rows
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    t.set_attrs(np.arange(N6), tags, stamps)
    yield t, rows, qs, tags, stamps
    t.close()


PREDICATES = {"0 rows": {"stamp_lo": N6 + 5}, "1 row": {"stamp_lo": 5, "stamp_hi": 5}, "7 rows": {"stamp_lo": 100, "stamp_hi": 106},
              "1 %": PERCENT, "100 %": {}}


@pytest.mark.parametrize("name", list(PREDICATES))
def test_search_where_equals_search_filtered_to_the_bit(corpus, name):
    t, rows, qs, tags, stamps = corpus
    where = PREDICATES[name]
    ids = check_rows(t, tags, stamps, None, (), where, name)
    assert ids.size == {"0 rows": 0, "1 row": 1, "7 rows": 7, "100 %": N6}.get(name, ids.size) and (name != "1 %" or 80 < ids.size < 300)
    for nq in (1, 2, 3, 4, 8):
        for k in (1, 10, 64, 100, 1024, 4096):
            q = qs[:nq]
            f_idx, f_dist = t.knn(q, k, within=ids)
            w_idx, w_dist, matched = t.knn_where(q, k, **as_kwargs(where))
            assert matched == ids.size, (name, nq, k)
            assert w_idx.shape == (nq, k) and np.array_equal(w_idx, f_idx), (name, nq, k)
            assert np.array_equal(w_dist.view(np.uint32), f_dist.view(np.uint32)), (name, nq, k)
            hits = min(k, ids.size)
            assert np.all(w_idx[:, hits:] == NO_ID) and np.all(w_dist[:, hits:].view(np.uint32) == 0x7F800000), (name, nq, k)
            assert np.all(w_idx[:, :hits] != NO_ID)


def test_search_where_against_the_oracle(orc, corpus):
    """not through the filtered call: the oracle's distances of the restatement's rows, ordered by (distance word, id)"""
    t, rows, qs, tags, stamps = corpus
    ids = where_rows(tags, stamps, None, (), PERCENT)
    for k in (10, 100):
        d = orc_cosine_dist(orc, qs[0], rows[ids.astype(np.int64)])
        e_idx, e_dist, _ = expected_page(d, ids, k)
        w_idx, w_dist, matched = t.knn_where(qs[0], k, **as_kwargs(PERCENT))
        assert matched == ids.size and np.array_equal(w_idx, e_idx) and np.array_equal(bits(w_dist), bits(e_dist)), k


def test_search_where_limits(corpus):
    t, rows, qs, tags, stamps = corpus
    with pytest.raises(_lib.MiError) as e:
        t.knn_where(qs[0], 4097)
    assert e.value.code == -5                                  # MI_ERR_UNSUPPORTED
    with pytest.raises(_lib.MiError) as e:
        t.knn_where(qs[0], 0)
    assert e.value.code == -1
    w = _lib.KnnWhere(0, 0, 0, I64_MIN, I64_MAX, 0, 2)          # an unknown flag
    idx, dist, n = np.full(4, 7, np.uint64), np.full(4, -7.0, np.float32), ctypes.c_uint64(7)
    lib = _lib.lib()
    assert lib.mi_knn_search_where(t._h, qs.ctypes.data, 1, 4, w, idx.ctypes.data, dist.ctypes.data, ctypes.byref(n)) == -1
    assert lib.mi_knn_count_where(t._h, w, ctypes.byref(n)) == -1 and lib.mi_knn_rows_where(t._h, w, idx.ctypes.data, 4, ctypes.byref(n)) == -1
    assert np.all(idx == 7) and np.all(dist == -7.0) and n.value == 7


# ---- 7. lifetime ---------------------------------------------------------------------------------------------------------------------

def test_lifetime_of_the_columns(built):
    n0, n1 = 100, 5100
    t = table(n0)
    t.set_option("where_chunk", 64)
    # no columns: every row holds the defaults
    assert np.array_equal(t.rows_where(), np.arange(n0)) and t.rows_where(all_of=1).size == 0 and t.count_where(stamp=(0, 0)) == n0
    assert t.count_where(stamp=(1, None)) == 0 and all(not c.any() for c in t.get_attrs())
    tags, stamps = columns(n0, 7)
    t.set_attrs(np.arange(n0), tags, stamps)
    assert all(np.array_equal(a, b) for a, b in zip(t.get_attrs(), (tags, stamps)))
    t.insert(np.random.default_rng(8).standard_normal((n1 - n0, 64)).astype(np.float32))   # past the capacity: grow() carries the columns
    tags = np.concatenate([tags, np.zeros(n1 - n0, np.uint64)])
    stamps = np.concatenate([stamps, np.zeros(n1 - n0, np.int64)])
    assert all(np.array_equal(a, b) for a, b in zip(t.get_attrs(), (tags, stamps)))
    for where in (HALF, {"stamp_lo": 0, "stamp_hi": 0}, {"none_of": 1}, {}):
        check_rows(t, tags, stamps, None, (), where, "grown")
    # one column NULL keeps the other; a duplicate id takes its last value
    t.set_attrs([5, 4000, 5], tags=[3, 3, 9])
    tags[[5, 4000]] = 9, 3
    t.set_attrs([6, 4001], stamps=[-77, 77])
    stamps[[6, 4001]] = -77, 77
    assert all(np.array_equal(a, b) for a, b in zip(t.get_attrs(), (tags, stamps)))
    for where in (HALF, {"stamp_lo": 77, "stamp_hi": 77}, {"stamp_hi": -77, "stamp_lo": -77}, {"all_of": 9}):
        check_rows(t, tags, stamps, None, (), where, "one column")
    # a bad id writes nothing, on the host or on the device
    flipped = int(~tags[7])                                   # every bit row 7 does not hold: row 7 would match it only if written
    with pytest.raises(_lib.MiError) as e:
        t.set_attrs([7, n1], tags=[flipped, 1], stamps=[123456, 1])
    assert e.value.code == -1
    with pytest.raises(_lib.MiError):
        t.get_attrs([n1])
    assert all(np.array_equal(a, b) for a, b in zip(t.get_attrs(), (tags, stamps)))
    assert 7 not in check_rows(t, tags, stamps, None, (), {"all_of": flipped & -flipped}, "bad id") and t.count_where(stamp=(123456, 123456)) == 0
    t.close()


# ---- 8. sharded ------------------------------------------------------------------------------------------------------------------------

def test_sharded_equals_the_single_table(built):
    n = 1000
    rows = np.random.default_rng(51).standard_normal((n, 64)).astype(np.float32)
    qs = rows[[3, 700]] + np.float32(0.5)
    tags, stamps = columns(n, 53)
    one = EmbeddingTable(64, 0)
    one.insert(rows)
    sh = ShardedTable(64, devices=(0, 0), block_rows=64)
    sh.insert(rows)
    for t in (one, sh):
        t.set_attrs(np.arange(n), tags, stamps)
        t.delete([0, 63, 64, 500])
    dead = (0, 63, 64, 500)
    assert all(np.array_equal(a, b) for a, b in zip(sh.get_attrs(), (tags, stamps)))
    assert sh.get_attrs([999, 64])[1].tolist() == [stamps[999], stamps[64]]
    with pytest.raises(_lib.MiError):
        sh.set_attrs([n], tags=[1])

    def same(a, where, what):
        want = where_rows(tags, stamps, None, dead, where)
        assert a.count_where(**as_kwargs(where)) == one.count_where(**as_kwargs(where)) == want.size, (what, where)
        assert np.array_equal(a.rows_where(**as_kwargs(where)), want), (what, where)
        for q, k in ((qs[0], 10), (qs, 100), (qs[1], 1000)):
            s_idx, s_dist, s_m = a.knn_where(q, k, **as_kwargs(where))
            o_idx, o_dist, o_m = one.knn_where(q, k, **as_kwargs(where))
            assert s_m == o_m == want.size and np.array_equal(s_idx, o_idx), (what, where, k)
            assert np.array_equal(s_dist.view(np.uint32), o_dist.view(np.uint32)), (what, where, k)

    for where in (HALF, PERCENT, {}, NOTHING_RUN, {"stamp_lo": -10, "stamp_hi": 300, "none_of": 4}):
        same(sh, where, "two shards")
    three = ShardedTable(64, devices=(0, 0, 0), block_rows=128)   # after a rebalance the columns follow the ids
    three.rebalance_from(sh)
    assert all(np.array_equal(a, b) for a, b in zip(three.get_attrs(), (tags, stamps)))
    for where in (HALF, {"stamp_lo": 0}):
        same(three, where, "rebalanced")
    three.close()
    sh.close()
    one.close()


# ---- 9. the index ------------------------------------------------------------------------------------------------------------------------

def test_image_index_set_attrs_and_web_search_where(built):
    rng = np.random.default_rng(61)
    n = 60
    rows = rng.standard_normal((n, 768)).astype(np.float32)
    q = (rows[9] + 0.6 * rng.standard_normal(768)).astype(np.float32)
    dirs = ["", "trip/", "trip/day1/", "home/"]
    which = rng.integers(0, 4, n)
    which[:4] = [2, 0, 3, 1]
    paths = [f"/srv/media/{dirs[w]}{i:03d}.jpg" for i, w in enumerate(which)]
    ix = ImageIndex(768, 0, "/srv/media/")
    ix.insert(paths, rows)
    refs = ["media/" + paths[j][len("/srv/media/"):] for j in (3, 12)]
    tags = rng.integers(0, 8, n, dtype=np.uint64)
    stamps = rng.integers(2015, 2025, n, dtype=np.int64)
    ix.set_attrs(paths, tags, stamps)
    assert all(np.array_equal(a, b) for a, b in zip(ix.table.get_attrs(), (tags, stamps)))
    with pytest.raises(_lib.MiError) as e:                      # an unknown path: nothing written
        ix.set_attrs([paths[0], "/srv/media/nope.jpg"], [7, 7], [1, 1])
    assert e.value.code == -1 and ix.table.get_attrs([0])[0][0] == tags[0]
    # "in this folder" is the directory's group: what mi_index_search_within finds for a folder without subfolders
    for folder in ("media/trip/day1", "media/home/", "media/trip/day1/"):
        hits, matched = ix.web_search_where(q, refs, k=n, folder=folder)
        within = ix.web_search_text(q, refs, k=n, folders=[folder])
        assert hits == within and matched == len(within) == int((which == dirs.index(folder.rstrip("/")[len("media/"):] + "/")).sum())
    hits, matched = ix.web_search_where(q, refs, k=n, folder="media/")             # the files directly in the media directory
    assert matched == len(hits) == int((which == 0).sum()) and all(h[1].count("/") == 1 for h in hits)
    with pytest.raises(_lib.MiError):
        ix.group_of("media/none")
    # tags and stamps on top, against the table's filtered search over the restatement's rows
    ix.remove([paths[20]])
    groups = np.array([ix.group_of("media/" + dirs[w]) for w in which], np.uint32)
    where = {"all_of": 1, "none_of": 4, "stamp_lo": 2017, "stamp_hi": 2022, "group": ix.group_of("media/trip")}
    ids = where_rows(tags, stamps, groups, (20,), where)
    query = refine_query(q, [rows[3], rows[12]])
    f_idx, f_dist = ix.table.knn(query, 20, within=ids)
    hits, matched = ix.web_search_where(q, refs, k=20, all_of=1, none_of=4, stamp=(2017, 2022), folder="media/trip")
    assert matched == ids.size and [h[0] for h in hits] == f_idx[:ids.size].tolist()
    assert np.array_equal(bits(np.array([h[2] for h in hits], np.float32)), bits(f_dist[:ids.size]))
    hits, matched = ix.web_search_where(q, (), k=5, any_of=6)                          # no folder: no group column needed
    assert matched == where_rows(tags, stamps, None, (20,), {"any_of": 6}).size and len(hits) == min(5, matched)
    ix.close()
