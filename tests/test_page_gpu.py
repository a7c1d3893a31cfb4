"""mi_knn_search_page on the GPU: ids, distance BITS and counts for equality with the numpy restatement
(tests/test_page_host.py: expected_page), which is fed by the CPU oracle alone — d = orc_cosine_dist(q, rows), what the single
pass reports.  No tolerance anywhere."""
import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable
from oracle.binding import orc_cosine_dist
from test_page_host import INF, NO_ID, bits, expected_page, total

pytestmark = pytest.mark.gpu

MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
NAMES = ("before", "window", "beyond", "nan")


def call(t, q, k, after=None, max_dist=INF, among=None, fn=None):
    """the C call with every output -> (rc, idx, dist, counts); the arrays keep a sentinel where nothing was written"""
    q = np.ascontiguousarray(q, np.float32).reshape(-1)
    idx, dist, counts = np.full(max(k, 1), 7, np.uint64), np.full(max(k, 1), -7.0, np.float32), np.full(4, 7, np.uint64)
    ids, n_ids = None, 0
    if among is not None:
        a = np.ascontiguousarray(among, np.uint64)
        n_ids = a.size
        ids = (a if a.size else np.zeros(1, np.uint64)).ctypes.data
    a_dist, a_id = (0.0, int(NO_ID)) if after is None else (float(after[0]), int(after[1]))
    fn = fn or _lib.lib().mi_knn_search_page
    rc = fn(t._h, q.ctypes.data, k, a_dist, a_id, float(max_dist), ids, n_ids, idx.ctypes.data, dist.ctypes.data, counts.ctypes.data)
    return rc, idx, dist, counts


def check(t, d, ids, q, k, after=None, max_dist=INF, among=None, what="", fn=None):
    """one call against the restatement over the candidates (distances d, held under ids); returns (idx, dist, counts, next)"""
    w_idx, w_dist, w_counts = expected_page(d, ids, k, after, max_dist)
    rc, idx, dist, counts = call(t, q, k, after, max_dist, among, fn)
    assert rc == 0, (what, _lib.lib().mi_last_error())
    assert np.array_equal(idx[:k], w_idx), (what, idx[:8], w_idx[:8])
    assert np.array_equal(bits(dist[:k]), bits(w_dist)), what
    got = dict(zip(NAMES, (int(c) for c in counts)))
    assert got == w_counts and total(got) == len(np.asarray(ids).reshape(-1)), (what, got, w_counts)
    nxt = (dist[k - 1], int(idx[k - 1])) if idx[k - 1] != NO_ID else None
    return idx[:k], dist[:k], got, nxt


def walk(t, d, ids, q, k, max_dist=INF, among=None, what="", fn=None):
    """every page, each against the restatement with the previous page's last hit as the cursor; returns the concatenation"""
    got, after = [], None
    while True:
        idx, dist, counts, after = check(t, d, ids, q, k, after, max_dist, among, (what, "after", after), fn)
        assert counts["before"] == len(got)
        got += [int(i) for i in idx if i != NO_ID]
        if after is None:
            return got


@pytest.fixture(scope="module")
def corpus(built, orc):
    rng = np.random.default_rng(2027)
    rows = rng.standard_normal((5000, 768)).astype(np.float32)
    q = (rows[70] + 0.7 * rng.standard_normal(768)).astype(np.float32)
    return rows, q, orc_cosine_dist(orc, q, rows)


@pytest.fixture(scope="module")
def table5000(corpus):
    t = EmbeddingTable(768, 0)
    t.insert(corpus[0])
    yield t
    t.close()


# ---- tile edges, both selection paths, a cursor at every page boundary ----------------------------------------------------

@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_tile_edges(corpus, N):
    rows, q, d = corpus
    t = EmbeddingTable(768, 0)
    t.insert(rows[:N])
    ids = np.arange(N)
    full = expected_page(d[:N], ids, N)[0].tolist()
    for k in (1, 10, 64, 65, 100):
        assert walk(t, d[:N], ids, q, k, what=(N, k)) == full
    t.close()


# ---- the paging identity under every grid ------------------------------------------------------------------------------------

@pytest.mark.parametrize("blocks", [0, 1, 3, 1000])
def test_pages_concatenate_to_the_full_list(corpus, table5000, blocks):
    rows, q, d = corpus
    ids = np.arange(5000)
    full, full_dist, _ = expected_page(d, ids, 5000)
    lib = _lib.lib()
    try:
        table5000.set_option("page_blocks", blocks)
        for size in (7, 64, 100):
            got_i, got_d, after = [], [], None
            while True:
                rc, idx, dist, counts = call(table5000, q, size, after)
                assert rc == 0, lib.mi_last_error()
                assert int(counts[0]) == len(got_i) and int(counts.sum()) == 5000 and int(counts[1]) == 5000 - len(got_i)
                n = int((idx != NO_ID).sum())
                got_i += idx[:n].tolist()
                got_d += bits(dist[:n]).tolist()
                assert np.all(idx[n:] == NO_ID) and np.all(np.isinf(dist[n:]))
                if n < size:
                    break
                after = (dist[size - 1], idx[size - 1])
            assert got_i == full.tolist() and got_d == bits(full_dist).tolist(), (blocks, size)
    finally:
        table5000.set_option("page_blocks", 0)
    with pytest.raises(_lib.MiError):
        table5000.set_option("page_blocks", -1)


def test_the_generator_and_identity_a(corpus, table5000):
    """(a): no cursor, no bound = mi_knn_search without its NaN entries; pages() walks the whole list"""
    rows, q, d = corpus
    for k in (10, 64, 1000):
        p_idx, p_dist = table5000.knn(q, k)
        idx, dist, counts, nxt = table5000.knn_page(q, k)
        assert np.array_equal(idx, p_idx) and np.array_equal(bits(dist), bits(p_dist))
        assert nxt is not None and nxt[1] == int(idx[-1]) and bits(nxt[0]) == bits(dist[-1])
    bound = np.sort(d)[2499]
    got = np.concatenate([p[0] for p in table5000.pages(q, 1000, max_dist=float(bound))])
    want = expected_page(d, np.arange(5000), 5000, max_dist=bound)[0]
    assert 2500 <= got.size < 2510 and np.array_equal(got, want[want != NO_ID])


# ---- ties --------------------------------------------------------------------------------------------------------------------

def test_a_cursor_inside_a_group_of_exact_copies(orc, corpus):
    rows, q, _ = corpus
    rows = rows[:1000].copy()
    group = [10, 63, 64, 700]
    rows[group] = rows[10]
    q = (rows[10] + 0.05).astype(np.float32)                 # the group leads the list
    d = orc_cosine_dist(orc, q, rows)
    assert len(set(bits(d[group]).tolist())) == 1
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    ids = np.arange(1000)
    for k in (2, 3, 100):
        idx, dist, counts, nxt = check(t, d, ids, q, k, what=("ties", k))
        assert idx[:min(k, 4)].tolist() == group[:min(k, 4)]
        for cut in range(4):                                 # the rest of the group opens the next page in id order
            idx, dist, counts, _ = check(t, d, ids, q, k, after=(d[10], group[cut]), what=("ties", k, cut))
            rest = group[cut + 1:]
            assert idx[:min(k, len(rest))].tolist() == rest[:k] and counts["before"] == cut + 1
    assert walk(t, d, ids, q, 3, what="ties walk")[:4] == group
    t.close()


# ---- NaN ----------------------------------------------------------------------------------------------------------------------

def test_a_zero_row_is_counted_and_never_returned(orc, corpus):
    rows, q, _ = corpus
    rows = rows[:200].copy()
    rows[17] = 0.0                                           # x.x = 0: its distance is NaN
    d = orc_cosine_dist(orc, q, rows)
    assert np.isnan(d[17])
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    for k in (10, 64, 200):
        got = walk(t, d, np.arange(200), q, k, what=("nan", k))
        assert 17 not in got and len(got) == 199
        assert check(t, d, np.arange(200), q, k, what=("nan", k))[2]["nan"] == 1
        assert check(t, d, np.arange(200), q, k, max_dist=np.sort(d)[50], what=("nan bound", k))[2]["nan"] == 1
    t.close()


# ---- the bound ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [10, 100])
def test_the_bound_is_inclusive_on_the_key_order(corpus, table5000, k):
    rows, q, d = corpus
    ids = np.arange(5000)
    order = expected_page(d, ids, 5000)[0]
    for rank in (0, 5, k - 1, 777):
        r = int(order[rank])
        at = d[r]
        idx, dist, counts, _ = check(table5000, d, ids, q, k, max_dist=at, what=("at", rank))
        n_within = int((d <= at).sum())                       # (distances of random rows may coincide: counted, not assumed)
        assert counts["window"] + counts["before"] == n_within >= rank + 1
        assert (r in idx.tolist()) == (rank < k)
        below = np.nextafter(at, np.float32(-1))
        idx, dist, counts, _ = check(table5000, d, ids, q, k, max_dist=below, what=("below", rank))
        assert r not in idx.tolist() and counts["window"] == int((d < at).sum()) <= rank
        # with a cursor: the window shrinks by what lies before it, the sum stays
        if rank >= 3:
            cur = (d[order[2]], int(order[2]))
            idx, dist, counts, _ = check(table5000, d, ids, q, k, after=cur, max_dist=at, what=("at, cursor", rank))
            assert counts["before"] == 3 and counts["window"] + counts["before"] == n_within
    # a cursor past the bound: nothing, and everything is before or beyond
    cur = (d[order[100]], int(order[100]))
    idx, dist, counts, nxt = check(table5000, d, ids, q, k, after=cur, max_dist=d[order[50]], what="cursor past the bound")
    assert nxt is None and np.all(idx == NO_ID) and counts == {"before": 101, "window": 0, "beyond": 4899, "nan": 0}


# ---- rows deleted and appended between two pages --------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [10, 100])
def test_changes_between_pages(orc, corpus, k):
    rows, q, d = corpus
    n0 = 1000
    t = EmbeddingTable(768, 0)
    t.insert(rows[:n0])
    ids = np.arange(n0)
    idx1, dist1, _, cur = check(t, d[:n0], ids, q, k, what="page 1")
    order = expected_page(d[:n0], ids, n0)[0]
    # delete the cursor's own row, two rows already delivered and three of the next page
    gone = [cur[1], int(order[0]), int(order[k // 2]), int(order[k]), int(order[k + 3]), int(order[2 * k - 1])]
    t.delete(gone)
    live = np.array([r for r in range(n0) if r not in set(gone)])
    idx2, dist2, counts2, cur2 = check(t, d[live], live, q, k, after=cur, what="page 2 after deletes")
    assert not set(idx2.tolist()) & set(gone) and not set(idx2.tolist()) & set(idx1.tolist())
    assert idx2.tolist() == [int(r) for r in order[k:] if int(r) not in set(gone)][:k] and counts2["before"] == k - 3
    # append rows that sort before the cursor (copies of delivered rows, and of the cursor's row: an equal distance, a higher
    # id, so it sorts AFTER the cursor) and after it
    new = np.concatenate([rows[[int(order[1]), int(order[3])]], rows[[cur2[1]]], rows[[int(order[3 * k]), int(order[n0 - 1])]],
                          rows[n0:n0 + 40]])
    t.insert(new)
    d_new = orc_cosine_dist(orc, q, new)
    assert bits(d_new[2]) == bits(cur2[0])
    all_d, all_ids = np.concatenate([d[:n0], d_new]), np.arange(n0 + len(new))
    live = np.array([r for r in all_ids if r not in set(gone)])
    idx3, dist3, counts3, _ = check(t, all_d[live], live, q, k, after=cur2, what="page 3 after appends")
    assert int(idx3[0]) == n0 + 2                            # the copy of the cursor's row opens the page
    assert n0 not in idx3.tolist() and n0 + 1 not in idx3.tolist() and counts3["before"] >= 2 * k - 3 + 2
    assert not set(idx3.tolist()) & (set(idx1.tolist()) | set(idx2.tolist()))
    walk(t, all_d[live], live, q, k if k > 10 else 37, what="the table as it is now")
    t.close()


# ---- among -----------------------------------------------------------------------------------------------------------------------

def test_among(corpus):
    rows, q, d = corpus
    t = EmbeddingTable(768, 0)
    t.insert(rows[:1000])
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
            got = walk(t, d[keep], keep, q, k, among=among, what=("among", n, k))
            assert sorted(got) == keep.tolist()
            if n >= 64:
                check(t, d[keep], keep, q, k, after=(d[keep[7]], int(keep[7])), max_dist=np.sort(d[keep])[40], among=among, what=("among window", n, k))
    # a deleted row as the cursor, outside `among`
    check(t, d[keep], keep, q, 10, after=(d[300], 300), among=among, what="deleted cursor")
    # an id outside the table: MI_ERR_INVALID, nothing written
    rc, idx, dist, counts = call(t, q, 5, among=[1, 2, 1000])
    assert rc == MI_ERR_INVALID and np.all(idx == 7) and np.all(dist == -7.0) and np.all(counts == 7)
    t.close()


# ---- ids above 32 bits, another dim ---------------------------------------------------------------------------------------------

def test_ids_above_32_bits(corpus):
    rows, q, d = corpus
    base = 1 << 33
    t = EmbeddingTable(768, 0)
    t.set_base(base)
    t.insert(rows[:300])
    ids = base + np.arange(300, dtype=np.uint64)
    for k in (7, 100):
        got = walk(t, d[:300], ids, q, k, what=("base", k))
        assert min(got) >= base and len(got) == 300
    sub = ids[10:200]
    walk(t, d[10:200], sub, q, 64, among=sub, what="base among")
    rc, idx, dist, counts = call(t, q, 5, after=(0.5, 3))          # an id below the base is not a row
    assert rc == MI_ERR_INVALID and np.all(idx == 7)
    t.close()


def test_dim_128(orc, built):
    rng = np.random.default_rng(128)
    rows = rng.standard_normal((300, 128)).astype(np.float32)
    rows[[40, 41, 250]] = rows[7]
    q = (rows[7] + 0.3 * rng.standard_normal(128)).astype(np.float32)
    d = orc_cosine_dist(orc, q, rows)
    t = EmbeddingTable(128, 0)
    t.insert(rows)
    for k in (3, 64, 100):
        assert len(walk(t, d, np.arange(300), q, k, what=(128, k))) == 300
    check(t, d, np.arange(300), q, 10, after=(d[40], 40), max_dist=np.sort(d)[100], what=(128, "window"))
    t.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------

def test_errors_write_nothing_and_empty_sets_pad(corpus, table5000):
    rows, q, d = corpus
    t = table5000
    lib = _lib.lib()

    def untouched(got, code):
        rc, idx, dist, counts = got
        assert rc == code, (rc, lib.mi_last_error())
        assert np.all(idx == 7) and np.all(dist == -7.0) and np.all(counts == 7)

    untouched(call(t, q, 4, after=(0.5, 5000)), MI_ERR_INVALID)              # after_id is not a row
    untouched(call(t, q, 4, after=(np.nan, 5)), MI_ERR_INVALID)
    untouched(call(t, q, 4, max_dist=np.nan), MI_ERR_INVALID)
    untouched(call(t, q, 0), MI_ERR_INVALID)
    untouched(call(t, q, 4097), MI_ERR_UNSUPPORTED)
    untouched(call(t, q, 4, among=[5000]), MI_ERR_INVALID)
    idx, dist = np.full(4, 7, np.uint64), np.full(4, -7.0, np.float32)
    no = int(NO_ID)
    assert lib.mi_knn_search_page(t._h, None, 4, 0.0, no, np.inf, None, 0, idx.ctypes.data, dist.ctypes.data, None) == MI_ERR_INVALID
    assert lib.mi_knn_search_page(t._h, q.ctypes.data, 4, 0.0, no, np.inf, None, 0, None, dist.ctypes.data, None) == MI_ERR_INVALID
    assert lib.mi_knn_search_page(t._h, q.ctypes.data, 4, 0.0, no, np.inf, None, 3, idx.ctypes.data, dist.ctypes.data, None) == MI_ERR_INVALID
    assert np.all(idx == 7) and np.all(dist == -7.0)
    # counts may be NULL; a NaN after_dist is ignored without a cursor
    assert lib.mi_knn_search_page(t._h, q.ctypes.data, 4, np.nan, no, np.inf, None, 0, idx.ctypes.data, dist.ctypes.data, None) == 0
    assert np.array_equal(idx, expected_page(d, np.arange(5000), 4)[0])
    odd = EmbeddingTable(192, 0)
    odd.insert(np.ones((3, 192), np.float32))
    assert call(odd, np.ones(192, np.float32), 2)[0] == MI_ERR_UNSUPPORTED    # a dim outside the set
    odd.close()
    # an empty table, an empty candidate set: all padding, every count 0, MI_OK
    e = EmbeddingTable(768, 0)
    for target, among in ((e, None), (t, [])):
        rc, idx, dist, counts = call(target, q, 3, among=among)
        assert rc == 0 and np.all(idx == NO_ID) and np.all(np.isinf(dist)) and np.all(counts == 0)
    e.close()


# ---- the sharded table -----------------------------------------------------------------------------------------------------------

def test_sharded_equals_one_table(orc, corpus):
    rows, q, _ = corpus
    rows = rows[:600].copy()
    group = [3, 70, 130, 200, 260, 595]                       # blocks of 64 rows, two shards: rows 3, 130, 260 live in shard 0, 70, 200, 595 in shard 1
    rows[group] = rows[3]
    q = (rows[3] + 0.05).astype(np.float32)
    d = orc_cosine_dist(orc, q, rows)
    sh = ShardedTable(768, devices=(0, 0), block_rows=64)
    sh.insert(rows)
    one = EmbeddingTable(768, 0)
    one.insert(rows)
    assert [(g // 64) % 2 for g in group] == [0, 1, 0, 1, 0, 1]
    ids = np.arange(600)
    fn = _lib.lib().mi_knn_sharded_search_page
    for k in (4, 100):
        for cut in range(len(group)):                         # the cursor cuts the group between the shards
            a = check(sh, d, ids, q, k, after=(d[3], group[cut]), what=("sharded cut", k, cut), fn=fn)
            b = check(one, d, ids, q, k, after=(d[3], group[cut]), what=("one cut", k, cut))
            assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
            assert a[0][:len(group) - cut - 1].tolist() == group[cut + 1:][:k]
    for k in (7, 100):
        assert walk(sh, d, ids, q, k, what=("sharded walk", k), fn=fn) == walk(one, d, ids, q, k, what=("one walk", k))
    gone = [0, 63, 64, 70, 500, 599]
    sh.delete(gone)
    one.delete(gone)
    live = np.array([r for r in range(600) if r not in set(gone)])
    rng = np.random.default_rng(9)
    within = rng.choice(600, 250, replace=False)
    keep = np.array(sorted(set(int(i) for i in within) - set(gone)))
    for k in (7, 100):
        walk(sh, d[live], live, q, k, max_dist=np.sort(d)[400], what=("sharded deleted", k), fn=fn)
        check(sh, d[live], live, q, k, after=(d[70], 70), what=("sharded, a deleted cursor", k), fn=fn)
        walk(sh, d[keep], keep, q, k, among=within, what=("sharded among", k), fn=fn)
    idx, dist, counts, nxt = sh.knn_page(q, 5, within=[])
    assert np.all(idx == NO_ID) and np.all(np.isinf(dist)) and nxt is None and total(counts) == 0
    p_one, p_sh = one.knn_page(q, 50, max_dist=float(np.sort(d)[300])), sh.knn_page(q, 50, max_dist=float(np.sort(d)[300]))
    assert np.array_equal(p_one[0], p_sh[0]) and p_one[2] == p_sh[2] and p_one[3][1] == p_sh[3][1]
    with pytest.raises(_lib.MiError):
        sh.knn_page(q, 5, after=(0.5, 600))
    with pytest.raises(_lib.MiError):
        sh.knn_page(q, 5, within=[600])
    one.close()
    sh.close()


# ---- the index --------------------------------------------------------------------------------------------------------------------

def test_image_index_web_search_page(orc, corpus):
    rows, q, _ = corpus
    rows = rows[:504].copy()
    rows[33] = 0.0                                            # a NaN entry of web_search_text
    paths = [f"/srv/media/{'trip' if i % 3 else 'home'}/{i:04d}.jpg" for i in range(504)]
    ix = ImageIndex(768, 0, "/srv/media/")
    ix.insert(paths, rows)
    refs = ["media/" + paths[j][len("/srv/media/"):] for j in (12, 400)]      # client names, as the web client marks them
    from image_search_amd.search import refine_query
    query = refine_query(q, [rows[12], rows[400]])
    d = orc_cosine_dist(orc, query, rows)
    # page 1 = web_search_text without its NaN entries
    plain = [h for h in ix.web_search_text(q, refs, k=504) if not np.isnan(h[2])]
    hits, counts, nxt = ix.web_search_page(q, refs, k=40)
    assert hits == plain[:40] and counts == {"before": 0, "window": 503, "beyond": 0, "nan": 1} and nxt[1] == hits[-1][0]
    assert [h[0] for h in hits] == expected_page(d, np.arange(504), 40)[0].tolist()
    # a removed path never appears on a later page, the cursor's own included
    gone = [hits[-1][1].replace("media/", "/srv/media/", 1), plain[45][1].replace("media/", "/srv/media/", 1), plain[3][1].replace("media/", "/srv/media/", 1)]
    ix.remove(gone)
    gone_ids = {hits[-1][0], plain[45][0], plain[3][0]}
    live = np.array([j for j in range(504) if j not in gone_ids])
    seen, after = [h[0] for h in hits], nxt
    while after is not None:
        page, counts, after = ix.web_search_page(q, refs, k=40, after=after)
        assert counts["before"] == len(seen) - 2 and total(counts) == 501
        seen += [h[0] for h in page]
        assert all(h[1] == "media/" + paths[h[0]][len("/srv/media/"):] for h in page)
    assert seen == [int(i) for i in expected_page(d, np.arange(504), 504)[0][:503] if int(i) not in (gone_ids - {hits[-1][0], plain[3][0]})]
    # folders restrict the candidates
    keep = np.array([j for j in live if j % 3])
    page, counts, after = ix.web_search_page(q, refs, k=30, folders=("media/trip",), max_dist=float(np.sort(d[keep])[99]))
    w_idx, w_dist, w_counts = expected_page(d[keep], keep, 30, max_dist=np.sort(d[keep])[99])
    assert [h[0] for h in page] == w_idx.tolist() and counts == w_counts and counts["window"] >= 100
    assert np.array_equal(bits(np.array([h[2] for h in page], np.float32)), bits(w_dist))
    assert ix.web_search_page(q, refs, k=5, folders=("media/none",)) == ([], {"before": 0, "window": 0, "beyond": 0, "nan": 0}, None)
    ix.close()
