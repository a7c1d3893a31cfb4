"""mi_knn_search_ordered and mi_knn_stamp_histogram on the GPU: ids, distance BITS, stamps and counts for equality with the
numpy restatement (tests/test_ordered_host.py: expected_ordered / expected_hist), which is fed by the CPU oracle alone — d =
orc_cosine_dist(q, rows), what the single pass reports — and by the predicate's restatement (tests/test_where_host.py:
where_rows).  Integers and bits only: no tolerance anywhere."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import MI_KNN_ORDER_AFTER, MI_KNN_ORDER_DESC, EmbeddingTable, ImageIndex, ShardedTable, make_where, refine_query
from oracle.binding import orc_cosine_dist
from test_ordered_host import I64_MAX, I64_MIN, expected_hist, expected_ordered
from test_page_host import INF, NO_ID, bits
from test_where_host import as_kwargs, where_rows

pytestmark = pytest.mark.gpu

MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
NAMES = ("within", "before", "beyond", "nan")


def call(t, q, k, max_dist=INF, where=None, flags=0, after=(0, 0), fn=None, want_stamps=True):
    """the C call with every output -> (rc, idx, dist, stamps, counts); the arrays keep a sentinel where nothing was written"""
    q = np.ascontiguousarray(q, np.float32).reshape(-1)
    n = max(k, 1)
    idx, dist, stamps, counts = np.full(n, 7, np.uint64), np.full(n, -7.0, np.float32), np.full(n, 7, np.int64), np.full(4, 7, np.uint64)
    w = None if where is None else make_where(**as_kwargs(where))
    fn = fn or _lib.lib().mi_knn_search_ordered
    rc = fn(t._h, q.ctypes.data, k, float(max_dist), None if w is None else ctypes.byref(w), flags, int(after[0]), int(after[1]),
            idx.ctypes.data, dist.ctypes.data, stamps.ctypes.data if want_stamps else None, counts.ctypes.data)
    return rc, idx, dist, stamps, counts


def check(t, d, ids, stamps, keep, q, k, max_dist=INF, descending=False, after=None, where=None, what=""):
    """knn_ordered against the restatement over the candidates `keep`; returns (idx, stamps, counts)"""
    w_idx, w_dist, w_st, w_counts = expected_ordered(bits(d), ids, stamps, keep, max_dist, descending, after, k)
    idx, dist, st, counts = t.knn_ordered(q, k, max_dist, descending, after, **(as_kwargs(where) if where is not None else {}))
    assert np.array_equal(idx, w_idx), (what, idx[:8], w_idx[:8])
    assert np.array_equal(bits(dist), bits(w_dist)), what
    assert np.array_equal(st, w_st), (what, st[:8], w_st[:8])
    assert counts == w_counts and sum(counts[c] for c in ("within", "beyond", "nan")) == len(keep), (what, counts, w_counts)
    return idx, st, counts


@pytest.fixture(scope="module")
def corpus(built, orc):
    rng = np.random.default_rng(2031)
    rows = rng.standard_normal((5000, 768)).astype(np.float32)
    q = (rows[70] + 0.7 * rng.standard_normal(768)).astype(np.float32)
    d = orc_cosine_dist(orc, q, rows)
    distinct = rng.integers(I64_MIN, I64_MAX, 5000, dtype=np.int64, endpoint=True)        # every stamp distinct (random 64-bit)
    assert np.unique(distinct).size == 5000
    eight = rng.choice(np.array([I64_MIN, -(1 << 40), -1, 0, 1, 1 << 20, 1 << 41, I64_MAX], np.int64), 5000)
    return rows, q, d, distinct, eight


@pytest.fixture(scope="module")
def table5000(corpus):
    t = EmbeddingTable(768, 0)
    t.insert(corpus[0])
    yield t
    t.close()


ALL = np.arange(5000)


# ---- tile and tail edges ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_tile_and_tail_edges(corpus, N):
    rows, q, d, distinct, eight = corpus
    t = EmbeddingTable(768, 0)
    t.insert(rows[:N])
    ids, keep = np.arange(N), np.arange(N)
    bound = np.sort(d[:N])[N // 2]                      # an exact distance: the bound is inclusive
    for stamps in (distinct[:N], eight[:N]):
        t.set_attrs(ids, None, stamps)
        for desc in (False, True):
            for k in (1, 10, 64, 65):
                check(t, d[:N], ids, stamps, keep, q, k, descending=desc, what=(N, k, desc))
            idx, st, c = check(t, d[:N], ids, stamps, keep, q, 10, max_dist=bound, descending=desc, what=(N, "bound"))
            assert c["within"] == N // 2 + 1
            if idx[9] != NO_ID:
                check(t, d[:N], ids, stamps, keep, q, 10, max_dist=bound, descending=desc, after=(st[9], idx[9]), what=(N, "page 2"))
    t.close()


def test_dim_128(built, orc):
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((333, 128)).astype(np.float32)
    q = rng.standard_normal(128).astype(np.float32)
    d = orc_cosine_dist(orc, q, rows)
    stamps = rng.integers(-50, 50, 333, dtype=np.int64)
    t = EmbeddingTable(128, 0)
    t.insert(rows)
    t.set_attrs(np.arange(333), None, stamps)
    for desc in (False, True):
        check(t, d, np.arange(333), stamps, np.arange(333), q, 100, max_dist=np.median(d), descending=desc, what=("dim 128", desc))
    t.close()


# ---- both selection regimes and the limit ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["distinct", "eight"])
def test_distinct_stamps_and_heavy_ties(corpus, table5000, kind):
    """distinct: the pick is decided in the stamp digits; eight values: the k-th stamp is shared by hundreds of rows and the
    position digits decide"""
    rows, q, d, distinct, eight = corpus
    stamps = distinct if kind == "distinct" else eight
    table5000.set_attrs(ALL, None, stamps)
    bound = np.sort(d)[3999]
    for desc in (False, True):
        for k in (10, 100, 4096):
            check(table5000, d, ALL, stamps, ALL, q, k, descending=desc, what=(kind, k, desc))
            idx, st, c = check(table5000, d, ALL, stamps, ALL, q, k, max_dist=bound, descending=desc, what=(kind, k, desc, "bound"))
            assert c["within"] == 4000
        idx, st, c = check(table5000, d, ALL, stamps, ALL, q, 100, descending=desc, what="page 1")
        idx, st, c = check(table5000, d, ALL, stamps, ALL, q, 100, descending=desc, after=(st[99], idx[99]), what="page 2")
        assert c["before"] == 100


def test_a_table_without_attribute_columns_is_ordered_by_id(corpus):
    """the null column: every stamp is 0, so the position digits decide everything; a column of zeros gives the same result"""
    rows, q, d, distinct, eight = corpus
    n = 3000
    t = EmbeddingTable(768, 0)
    t.insert(rows[:n])
    ids, zeros = np.arange(n), np.zeros(n, np.int64)
    bound = np.sort(d[:n])[1999]
    got = []
    for step in ("no column", "zeros"):
        for desc in (False, True):
            a = check(t, d[:n], ids, zeros, ids, q, 100, max_dist=bound, descending=desc, what=(step, desc))
            b = check(t, d[:n], ids, zeros, ids, q, 100, max_dist=bound, descending=desc, after=(0, a[0][99]), what=(step, desc, "page 2"))
            c = check(t, d[:n], ids, zeros, ids, q, 4096, descending=desc, what=(step, desc, 4096))
            assert np.array_equal(c[0][:n], ids) and np.all(np.diff(a[0].astype(np.int64)) > 0)
            got.append((a[0].tolist(), b[0].tolist()))
        hist = t.stamp_histogram(q, [0, 1], max_dist=bound)
        assert hist.tolist() == [0, 2000, 0]
        t.set_attrs(ids, None, zeros)
    assert got[0] == got[1] == got[2] == got[3]
    t.close()


def test_sign_and_extremes(corpus):
    rows, q, d, distinct, eight = corpus
    n = 200
    stamps = np.random.default_rng(3).integers(-3, 4, n, dtype=np.int64)
    stamps[[0, 64, 130]] = I64_MIN
    stamps[[1, 63, 131]] = -1
    stamps[[5, 66]] = 0
    stamps[[2, 65, 199]] = I64_MAX
    stamps[[3, 127]] = 1
    t = EmbeddingTable(768, 0)
    t.insert(rows[:n])
    t.set_attrs(np.arange(n), None, stamps)
    for desc in (False, True):
        idx, st, c = check(t, d[:n], np.arange(n), stamps, np.arange(n), q, n, descending=desc, what=("extremes", desc))
        assert st[0] == (I64_MAX if desc else I64_MIN) and st[-1] == (I64_MIN if desc else I64_MAX)
        check(t, d[:n], np.arange(n), stamps, np.arange(n), q, 10, descending=desc, after=(I64_MIN, 64), what=("after min", desc))
        check(t, d[:n], np.arange(n), stamps, np.arange(n), q, 10, descending=desc, after=(I64_MAX, 65), what=("after max", desc))
        check(t, d[:n], np.arange(n), stamps, np.arange(n), q, 10, descending=desc, after=(-1, 63), what=("after -1", desc))
    t.close()


# ---- the timeline, cursors, changes between pages --------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["distinct", "eight"])
def test_timeline_equals_the_sorted_whole(corpus, table5000, kind):
    rows, q, d, distinct, eight = corpus
    stamps = distinct if kind == "distinct" else eight
    table5000.set_attrs(ALL, None, stamps)
    bound = np.sort(d)[1499]
    for desc in (False, True):
        full = expected_ordered(bits(d), ALL, stamps, ALL, bound, desc, None, 5000)
        got_i, got_d, got_s, pages = [], [], [], 0
        for idx, dist, st, counts in table5000.timeline(q, 100, max_dist=bound, descending=desc):
            assert counts["within"] == 1500 and counts["before"] == len(got_i)
            got_i += idx.tolist()
            got_d += bits(dist).tolist()
            got_s += st.tolist()
            pages += 1
        assert pages == 15 and got_i == full[0][:1500].tolist() and got_d == bits(full[1][:1500]).tolist()
        assert got_s == full[2][:1500].tolist()


def test_a_cursor_inside_a_group_of_equal_stamps_cuts_at_the_id(corpus, table5000):
    rows, q, d, distinct, eight = corpus
    table5000.set_attrs(ALL, None, eight)
    group = np.flatnonzero(eight == 1)
    assert group.size > 300
    for desc in (False, True):
        for cut in (group[0], group[group.size // 2], group[-1], group[5] + 1):        # the last: an id that holds another stamp
            idx, st, c = check(table5000, d, ALL, eight, ALL, q, 50, descending=desc, after=(1, int(cut)), what=("cut", desc, int(cut)))
            ones = idx[st == 1]
            assert np.all(ones > cut) and (ones.size == 0 or ones[0] == group[group > cut][0])


def test_changes_between_pages_skip_and_repeat_no_survivor(corpus):
    rows, q, d, distinct, eight = corpus
    n = 2000
    rng = np.random.default_rng(11)
    stamps = rng.integers(0, 40, n, dtype=np.int64)
    t = EmbeddingTable(768, 0)
    t.insert(rows[:n])
    t.set_attrs(np.arange(n), None, stamps)
    p1, st1, _ = check(t, d[:n], np.arange(n), stamps, np.arange(n), q, 300, what="page 1")
    cursor = (int(st1[-1]), int(p1[-1]))
    # between the pages: rows of page 1 and rows behind it are deleted — the cursor's own row too — and rows are appended with
    # stamps on both sides of the cursor
    dead = sorted({int(p1[-1]), int(p1[3]), 1999, 1500} | set(np.flatnonzero(stamps == cursor[0])[-2:].tolist()))
    t.delete(dead)
    t.insert(rows[n:n + 100])
    new = rng.integers(0, 40, 100, dtype=np.int64)
    new[:3] = cursor[0]                                           # in the cursor's group, at larger ids: behind it
    t.set_attrs(np.arange(n, n + 100), None, new)
    stamps2, ids2 = np.concatenate([stamps, new]), np.arange(n + 100)
    live = np.setdiff1d(ids2, dead)
    rest = []
    after = cursor
    while True:
        idx, st, c = check(t, d[:n + 100], ids2, stamps2, live, q, 300, after=after, what=("page", len(rest)))
        hits = idx[idx != NO_ID]
        rest += hits.tolist()
        if hits.size < 300:
            break
        after = (int(st[hits.size - 1]), int(hits[-1]))
    okey = [(int(stamps2[i]), i) for i in rest]
    assert okey == sorted(okey) and len(set(rest)) == len(rest) and not set(rest) & set(p1.tolist())
    # every survivor is in page 1 or behind the cursor
    behind = {int(i) for i in live if (int(stamps2[i]), int(i)) > cursor}
    assert set(rest) == behind
    assert behind | (set(p1.tolist()) - set(dead)) >= {int(i) for i in live if i < n}
    t.close()


def test_a_deleted_cursor_row_is_accepted(corpus):
    rows, q, d, distinct, eight = corpus
    n = 500
    t = EmbeddingTable(768, 0)
    t.insert(rows[:n])
    t.set_attrs(np.arange(n), None, eight[:n])
    t.delete([100])
    live = np.setdiff1d(np.arange(n), [100])
    for desc in (False, True):
        check(t, d[:n], np.arange(n), eight[:n], live, q, 50, descending=desc, after=(int(eight[100]), 100), what=("deleted cursor", desc))
    t.close()


# ---- predicates and deletions -----------------------------------------------------------------------------------------------------

def test_predicates_and_deletions(corpus, orc):
    rows, q, d, distinct, eight = corpus
    n = 3000
    rng = np.random.default_rng(13)
    tags = rng.integers(0, 16, n, dtype=np.uint64)
    stamps = rng.integers(-500, 500, n, dtype=np.int64)
    groups = rng.integers(0, 5, n).astype(np.uint32)
    t = EmbeddingTable(768, 0)
    t.insert(rows[:n])
    t.set_attrs(np.arange(n), tags, stamps)
    t.set_groups(groups)
    dead = list(range(128, 192)) + [0, 63, 64, 500, 2999]
    t.delete(dead)
    bound = np.sort(d[:n])[1999]
    for where in (None, {"all_of": 1}, {"any_of": 6, "none_of": 8}, {"stamp_lo": -100, "stamp_hi": 250}, {"group": 3},
                  {"all_of": 2, "stamp_lo": 0, "group": 1}, {"stamp_lo": 5000}, {"stamp_lo": 1, "stamp_hi": 0}):
        keep = where_rows(tags, stamps, groups, dead, dict(where or {}, n=n)).astype(np.int64)
        if where is not None:
            assert np.array_equal(t.rows_where(**as_kwargs(where)), keep.astype(np.uint64))
        for desc in (False, True):
            idx, st, c = check(t, d[:n], np.arange(n), stamps, keep, q, 100, max_dist=bound, descending=desc, where=where, what=(where, desc))
            if idx[99] != NO_ID:
                check(t, d[:n], np.arange(n), stamps, keep, q, 100, max_dist=bound, descending=desc, where=where,
                      after=(int(st[99]), int(idx[99])), what=(where, desc, "page 2"))
        # the same window as the paged search counts over the same rows
        page = t.knn_page(q, 1, None, bound, within=keep.astype(np.uint64) if where is not None else None)[2]
        assert c["within"] == page["window"] and c["beyond"] == page["beyond"] and c["nan"] == page["nan"]
        edges = [-400, -100, 0, 1, 250]
        hist = t.stamp_histogram(q, edges, max_dist=bound, **(as_kwargs(where) if where is not None else {}))
        assert np.array_equal(hist, expected_hist(bits(d[:n]), stamps, keep, bound, edges)) and int(hist.sum()) == c["within"]
    t.close()


def test_nan_rows_count_apart(built, orc):
    rng = np.random.default_rng(17)
    rows = rng.standard_normal((100, 768)).astype(np.float32)
    rows[[7, 64]] = 0.0                                          # a zero row: 0 / 0
    q = rng.standard_normal(768).astype(np.float32)
    d = orc_cosine_dist(orc, q, rows)
    assert np.isnan(d[[7, 64]]).all()
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    stamps = np.arange(100, dtype=np.int64)[::-1].copy()
    t.set_attrs(np.arange(100), None, stamps)
    idx, st, c = check(t, d, np.arange(100), stamps, np.arange(100), q, 100, what="nan")
    assert c["nan"] == 2 and c["within"] == 98 and 7 not in idx.tolist()
    t.close()


def test_ids_above_32_bits(corpus):
    rows, q, d, distinct, eight = corpus
    base = 1 << 33
    t = EmbeddingTable(768, 0)
    t.set_base(base)
    t.insert(rows[:300])
    ids = base + np.arange(300, dtype=np.uint64)
    t.set_attrs(ids, None, eight[:300])
    idx, st, c = check(t, d[:300], ids, eight[:300], np.arange(300), q, 100, what="base")
    assert idx.min() >= base
    check(t, d[:300], ids, eight[:300], np.arange(300), q, 100, after=(int(st[99]), int(idx[99])), what="base, page 2")
    rc, idx, dist, st, counts = call(t, q, 5, flags=MI_KNN_ORDER_AFTER, after=(0, 3))          # an id below the base is not a row
    assert rc == MI_ERR_INVALID and np.all(idx == 7) and np.all(counts == 7)
    t.close()


# ---- grid independence --------------------------------------------------------------------------------------------------------------

def test_the_same_bits_for_every_grid(corpus, table5000):
    rows, q, d, distinct, eight = corpus
    tags = np.random.default_rng(19).integers(0, 4, 5000, dtype=np.uint64)
    table5000.set_attrs(ALL, tags, eight)
    bound = np.sort(d)[2999]
    where = {"any_of": 1}
    keep = where_rows(tags, eight, None, (), dict(where, n=5000)).astype(np.int64)
    edges = [I64_MIN, -1, 0, 1, 2, 1 << 41]
    want_hist = expected_hist(bits(d), eight, keep, bound, edges)
    try:
        for blocks in (1, 3, 1000, 0):
            for chunk in (64, 4096):
                table5000.set_option("page_blocks", blocks)
                table5000.set_option("where_chunk", chunk)
                for k, desc in ((100, True), (4096, False)):
                    idx, st, c = check(table5000, d, ALL, eight, keep, q, k, max_dist=bound, descending=desc, where=where,
                                       what=(blocks, chunk, k))
                    check(table5000, d, ALL, eight, keep, q, k, max_dist=bound, descending=desc, where=where,
                          after=(int(st[49]), int(idx[49])), what=(blocks, chunk, k, "cursor"))
                    check(table5000, d, ALL, eight, ALL, q, k, max_dist=bound, descending=desc, what=(blocks, chunk, k, "no predicate"))
                hist = table5000.stamp_histogram(q, edges, max_dist=bound, **as_kwargs(where))
                assert np.array_equal(hist, want_hist), (blocks, chunk)
    finally:
        table5000.set_option("page_blocks", 0)
        table5000.set_option("where_chunk", 0)
        table5000.set_attrs(ALL, np.zeros(5000, np.uint64), None)


# ---- the histogram --------------------------------------------------------------------------------------------------------------------

def test_histogram_edges(corpus, table5000):
    rows, q, d, distinct, eight = corpus
    stamps = np.random.default_rng(23).integers(-3000, 3000, 5000, dtype=np.int64)
    table5000.set_attrs(ALL, None, stamps)
    bound = np.sort(d)[2499]
    within = table5000.knn_ordered(q, 1, bound)[3]["within"]
    assert within == 2500
    cases = {"on stamps": np.unique(stamps[:40]), "one edge": [0], "below all": [-9000, -8000], "above all": [4000, 5000, I64_MAX],
             "the extremes": [I64_MIN, I64_MAX], "4096 edges": np.arange(-2048, 2048), "4096 sparse": np.arange(4096) * 3 - 6000}
    for name, edges in cases.items():
        hist = table5000.stamp_histogram(q, edges, max_dist=bound)
        assert hist.dtype == np.uint64 and hist.size == len(edges) + 1
        assert np.array_equal(hist, expected_hist(bits(d), stamps, ALL, bound, edges)), name
        assert int(hist.sum()) == within, name
    assert table5000.stamp_histogram(q, [-9000, -8000], max_dist=bound).tolist() == [0, 0, 2500]
    assert table5000.stamp_histogram(q, [4000], max_dist=bound).tolist() == [2500, 0]


# ---- sharded ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shards", [1, 3, 8])
def test_sharded_equals_the_single_table(corpus, shards):
    rows, q, d, distinct, eight = corpus
    n = 1500
    rng = np.random.default_rng(29)
    tags = rng.integers(0, 4, n, dtype=np.uint64)
    stamps = eight[:n]
    one = EmbeddingTable(768, 0)
    one.insert(rows[:n])
    sh = ShardedTable(768, devices=(0,) * shards, block_rows=64)
    sh.insert(rows[:n])
    dead = [0, 63, 64, 700, 1499]
    for t in (one, sh):
        t.set_attrs(np.arange(n), tags, stamps)
        t.delete(dead)
    bound = np.sort(d[:n])[999]
    edges = [I64_MIN, -1, 0, 1, 2, 1 << 41]
    for where in (None, {"any_of": 1}):
        kw = as_kwargs(where) if where is not None else {}
        keep = where_rows(tags, stamps, None, dead, dict(where or {}, n=n)).astype(np.int64)
        for desc in (False, True):
            after = None
            for page in range(3):
                a = one.knn_ordered(q, 100, bound, desc, after, **kw)
                b = check(sh, d[:n], np.arange(n), stamps, keep, q, 100, max_dist=bound, descending=desc, after=after, where=where,
                          what=(shards, where, desc, page))
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[1]) and a[3] == b[2]
                after = (int(a[2][99]), int(a[0][99]))            # its row lives on one shard; the others translate it
            # a cursor at a deleted row, and one at the last row of a block
            for cut in (700, 63, 64):
                check(sh, d[:n], np.arange(n), stamps, keep, q, 100, max_dist=bound, descending=desc, after=(int(stamps[cut]), cut),
                      where=where, what=(shards, "cut", cut))
        assert np.array_equal(sh.stamp_histogram(q, edges, bound, **kw), one.stamp_histogram(q, edges, bound, **kw))
        assert np.array_equal(sh.stamp_histogram(q, edges, bound, **kw), expected_hist(bits(d[:n]), stamps, keep, bound, edges))
    rc = call(sh, q, 5, flags=MI_KNN_ORDER_AFTER, after=(0, n), fn=_lib.lib().mi_knn_sharded_search_ordered)[0]
    assert rc == MI_ERR_INVALID
    sh.close()
    one.close()


# ---- the index ------------------------------------------------------------------------------------------------------------------------

def test_image_index_web_search_ordered(built, orc):
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
    stamps = rng.integers(2015, 2025, n, dtype=np.int64)
    ix.set_attrs(paths, None, stamps)
    gone = int(np.flatnonzero(which == 1)[2])
    ix.remove([paths[gone]])
    query = refine_query(q, [rows[3], rows[12]])
    d = orc_cosine_dist(orc, query, rows)
    groups = np.array([ix.group_of("media/" + dirs[w]) for w in which], np.uint32)
    where = {"stamp_lo": 2017, "stamp_hi": 2022, "group": ix.group_of("media/trip")}
    keep = where_rows(None, stamps, groups, (gone,), dict(where, n=n)).astype(np.int64)
    bound = np.sort(d[keep])[keep.size - 2]
    w_idx, w_dist, w_st, w_counts = expected_ordered(bits(d), np.arange(n), stamps, keep, bound, True, None, 5)
    hits, counts, nxt = ix.web_search_ordered(q, refs, k=5, max_dist=bound, stamp=(2017, 2022), folder="media/trip")
    assert [h[0] for h in hits] == w_idx[:len(hits)].tolist() and len(hits) == int((w_idx != NO_ID).sum()) == 5
    assert [h[1] for h in hits] == ["media/" + paths[i][len("/srv/media/"):] for i in w_idx[:5]]
    assert np.array_equal(bits(np.array([h[2] for h in hits], np.float32)), bits(w_dist[:5])) and [h[3] for h in hits] == w_st[:5].tolist()
    assert counts == w_counts and nxt == (int(w_st[4]), int(w_idx[4]))
    hits2, counts2, nxt2 = ix.web_search_ordered(q, refs, k=5, max_dist=bound, after=nxt, stamp=(2017, 2022), folder="media/trip")
    w2 = expected_ordered(bits(d), np.arange(n), stamps, keep, bound, True, nxt, 5)
    assert [h[0] for h in hits2] == w2[0][w2[0] != NO_ID].tolist() and counts2 == w2[3]
    # the removed path never appears, with or without a predicate
    everything, c_all, _ = ix.web_search_ordered(q, refs, k=n, descending=False)
    assert len(everything) == n - 1 and gone not in [h[0] for h in everything] and c_all["within"] == n - 1
    assert [h[3] for h in everything] == sorted(h[3] for h in everything)
    edges = list(range(2016, 2025))
    hist = ix.web_timeline_histogram(q, edges, refs, max_dist=bound, stamp=(2017, 2022), folder="media/trip")
    assert np.array_equal(hist, expected_hist(bits(d), stamps, keep, bound, edges)) and int(hist.sum()) == w_counts["within"]
    ix.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------

def test_errors_write_nothing_and_an_empty_table_pads(corpus, table5000):
    rows, q, d, distinct, eight = corpus
    lib = _lib.lib()
    for what, kw, code in (("k = 0", dict(k=0), MI_ERR_INVALID), ("k = 4097", dict(k=4097), MI_ERR_UNSUPPORTED),
                           ("NaN bound", dict(k=5, max_dist=np.nan), MI_ERR_INVALID), ("an unknown flag", dict(k=5, flags=4), MI_ERR_INVALID),
                           ("after_id outside", dict(k=5, flags=MI_KNN_ORDER_AFTER, after=(0, 5000)), MI_ERR_INVALID),
                           ("after_id = NO_ID", dict(k=5, flags=MI_KNN_ORDER_AFTER | MI_KNN_ORDER_DESC, after=(0, int(NO_ID))), MI_ERR_INVALID)):
        rc, idx, dist, st, counts = call(table5000, q, **kw)
        assert rc == code, (what, rc, lib.mi_last_error())
        assert np.all(idx == 7) and np.all(dist == -7.0) and np.all(st == 7) and np.all(counts == 7), what
    rc, idx, dist, st, counts = call(table5000, q, 5, flags=0, after=(0, 5000))      # without the flag the cursor is not looked at
    assert rc == 0
    rc, idx, dist, st, counts = call(table5000, q, 5, want_stamps=False)               # stamps may be NULL
    assert rc == 0 and np.all(st == 7) and np.all(idx != NO_ID)
    hist = np.full(4, 7, np.uint64)
    for edges in ([3, 2, 1], [1, 1, 2]):
        e = np.array(edges, np.int64)
        assert lib.mi_knn_stamp_histogram(table5000._h, q.ctypes.data, 1.0, None, e.ctypes.data, 3, hist.ctypes.data) == MI_ERR_INVALID
    assert np.all(hist == 7)
    with pytest.raises(_lib.MiError):
        table5000.stamp_histogram(q, np.arange(4097))
    empty = EmbeddingTable(768, 0)
    rc, idx, dist, st, counts = call(empty, q, 5)
    assert rc == 0 and np.all(idx == NO_ID) and np.all(np.isinf(dist)) and np.all(st == 0) and np.all(counts == 0)
    assert empty.stamp_histogram(q, [0]).tolist() == [0, 0]
    empty.close()
    rc, idx, dist, st, counts = call(table5000, q, 5, where={"stamp_lo": 1, "stamp_hi": 0})   # a predicate that keeps nothing
    assert rc == 0 and np.all(idx == NO_ID) and np.all(counts == 0)
