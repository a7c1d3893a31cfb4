"""mi_knn_search_grouped on the GPU: ids, distance BITS, groups, members, facets and totals for equality with the numpy
restatement (tests/test_grouped_host.py: expected_grouped), which is fed by the CPU oracle alone — d = orc_cosine_dist(q, rows),
what the single pass reports.  No tolerance anywhere."""
import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable, refine_query
from oracle.binding import orc_cosine_dist
from test_grouped_host import NG, NO_GROUP, expected_grouped
from test_page_host import INF, NO_ID, bits, expected_page

pytestmark = pytest.mark.gpu

MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
NAMES = ("groups", "window", "beyond", "nan")
N = 5000


def call(t, q, k, max_dist=INF, among=None, cap_facets=None, fn=None):
    """the C call with every output -> (rc, idx, dist, group, members, facets, totals); the arrays keep a sentinel where nothing
    was written.  cap_facets: None = as many as the table has groups"""
    q = np.ascontiguousarray(q, np.float32).reshape(-1)
    kk = max(k, 1)
    idx, dist = np.full(kk, 7, np.uint64), np.full(kk, -7.0, np.float32)
    group, members, totals = np.full(kk, 7, np.uint32), np.full(kk, 7, np.uint64), np.full(4, 7, np.uint64)
    cap = t.groups_info()["n_groups"] if cap_facets is None else cap_facets
    facets = np.full(cap + 2, 7, np.uint64)                   # two entries past the cap: left alone
    ids, n_ids = None, 0
    if among is not None:
        a = np.ascontiguousarray(among, np.uint64)
        n_ids = a.size
        ids = (a if a.size else np.zeros(1, np.uint64)).ctypes.data
    fn = fn or (_lib.lib().mi_knn_sharded_search_grouped if isinstance(t, ShardedTable) else _lib.lib().mi_knn_search_grouped)
    rc = fn(t._h, q.ctypes.data, k, float(max_dist), ids, n_ids, idx.ctypes.data, dist.ctypes.data, group.ctypes.data,
            members.ctypes.data, facets.ctypes.data, cap, totals.ctypes.data)
    return rc, idx, dist, group, members, facets, totals


def check(t, d, ids, groups, q, k, max_dist=INF, among=None, what=""):
    """one call against the restatement over the candidates (distances d, held under ids, in groups); returns the device's
    (idx, dist, group, members, facets, totals dict)"""
    n_groups = t.groups_info()["n_groups"]
    w = expected_grouped(d, ids, groups, k, max_dist, n_groups)
    rc, idx, dist, group, members, facets, totals = call(t, q, k, max_dist, among)
    assert rc == 0, (what, _lib.lib().mi_last_error())
    assert np.array_equal(idx[:k], w[0]), (what, idx[:8], w[0][:8])
    assert np.array_equal(bits(dist[:k]), bits(w[1])), what
    assert np.array_equal(group[:k], w[2]), (what, group[:8], w[2][:8])
    assert np.array_equal(members[:k], w[3]), (what, members[:8], w[3][:8])
    assert np.array_equal(facets[:n_groups], w[4]) and np.all(facets[n_groups:] == 7), what
    got = dict(zip(NAMES, (int(c) for c in totals)))
    assert got == w[5] and got["window"] + got["beyond"] + got["nan"] == len(np.asarray(ids).reshape(-1)), (what, got, w[5])
    # (c): the facets and the matched singletons add up to the window
    assert int(w[4].sum()) + (got["groups"] - int((w[4] > 0).sum())) == got["window"], what
    return idx[:k], dist[:k], group[:k], members[:k], facets[:n_groups], got


def layout(name, n=N):
    r = np.arange(n)
    rng = np.random.default_rng(31)
    if name == "none":
        return np.full(n, NO_GROUP, np.uint32)
    if name == "one":
        return np.zeros(n, np.uint32)
    if name == "mod7":
        return (r % 7).astype(np.uint32)
    if name == "div64":
        return (r // 64).astype(np.uint32)
    if name == "div65":
        return (r // 65).astype(np.uint32)
    if name == "random300":
        g = rng.integers(0, 300, n).astype(np.uint32)
        g[:300] = np.arange(300)                              # every id occurs: n_groups is exactly 300
        g[rng.random(n) < 0.1] = NO_GROUP
        g[299] = 299
        return g
    if name == "heavy":
        g = rng.integers(1, 16, n).astype(np.uint32)
        g[rng.random(n) < 0.82] = 0
        return g
    raise KeyError(name)


LAYOUTS = ["none", "one", "mod7", "div64", "div65", "random300", "heavy"]


@pytest.fixture(scope="module")
def corpus(built, orc):
    rng = np.random.default_rng(2027)
    rows = rng.standard_normal((N, 768)).astype(np.float32)
    q = (rows[70] + 0.7 * rng.standard_normal(768)).astype(np.float32)
    return rows, q, orc_cosine_dist(orc, q, rows)


@pytest.fixture(scope="module")
def table5000(corpus):
    t = EmbeddingTable(768, 0)
    t.insert(corpus[0])
    yield t
    t.close()


# ---- tile edges -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_tile_edges(corpus, n):
    rows, q, d = corpus
    t = EmbeddingTable(768, 0)
    t.insert(rows[:n])
    ids = np.arange(n)
    for k in (1, 10, 64, 65, 100):                            # a table that never had a group: all singletons = the page call
        idx, dist, group, members, facets, got = check(t, d[:n], ids, np.full(n, NO_GROUP), q, k, what=("unset", n, k))
        p = expected_page(d[:n], ids, k)
        assert np.array_equal(idx, p[0]) and np.array_equal(bits(dist), bits(p[1]))
    groups = layout("mod7", n)
    groups[::5] = NO_GROUP
    t.set_groups(groups)
    assert np.array_equal(t.groups(), groups)
    for lds in (0, 4096):
        t.set_option("group_lds_max", lds)
        for k in (1, 10, 64, 65, 100):
            check(t, d[:n], ids, groups, q, k, what=(n, k, lds))
    t.close()


# ---- every layout under both reduce forms and every grid ------------------------------------------------------------------------

@pytest.mark.parametrize("name", LAYOUTS)
def test_layouts_forms_and_grids(corpus, table5000, name):
    rows, q, d = corpus
    t, ids, groups = table5000, np.arange(N), layout(name)
    t.set_groups(groups)
    bound = np.sort(d)[N // 2]
    try:
        first = None
        for lds in (0, 4096):
            for blocks in (0, 1, 3, 1000):
                t.set_option("group_lds_max", lds)
                t.set_option("group_blocks", blocks)
                got = [check(t, d, ids, groups, q, k, md, what=(name, lds, blocks, k)) for k, md in ((10, INF), (100, bound))]
                flat = [np.asarray(a).tolist() if not isinstance(a, dict) else a for g in got for a in g]
                first = first or flat
                assert flat == first, (name, lds, blocks)      # identical across forms and grids, bit for bit
    finally:
        t.set_option("group_lds_max", 4096)
        t.set_option("group_blocks", 0)
    if name == "none":                                        # (a): the page call, members = 1
        idx, dist, group, members, facets, got = check(t, d, ids, groups, q, 100, bound, what="a")
        p_idx, p_dist, p_counts = expected_page(d, ids, 100, None, bound)
        assert np.array_equal(idx, p_idx) and np.array_equal(bits(dist), bits(p_dist)) and np.all(members == 1) and np.all(group == NO_GROUP)
        t_idx, t_dist, t_counts, _ = t.knn_page(q, 100, max_dist=float(bound))
        assert np.array_equal(idx, t_idx) and np.array_equal(bits(dist), bits(t_dist)) and got["window"] == t_counts["window"]
    if name == "one":                                         # (b): one hit, the top-1, members = the window count
        idx, dist, group, members, facets, got = check(t, d, ids, groups, q, 10, bound, what="b")
        top = t.knn(q, 1)
        assert idx[0] == top[0][0] and bits(dist[0]) == bits(top[1][0]) and np.all(idx[1:] == NO_ID)
        assert members[0] == got["window"] == int((d <= bound).sum()) and got["groups"] == 1


def test_the_threshold_between_the_two_forms(corpus):
    rows, q, d = corpus
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    groups = layout("random300")
    t.set_groups(groups)
    assert t.groups_info() == {"n_groups": 300, "rows": int((groups != NO_GROUP).sum())}
    got = []
    for lds in (300, 299, 4096, 0):                           # n_groups exactly at the threshold, then threshold + 1
        t.set_option("group_lds_max", lds)
        got.append([np.asarray(a).tolist() for a in check(t, d, np.arange(N), groups, q, 100, what=("threshold", lds))[:5]])
    assert got[0] == got[1] == got[2] == got[3]
    for bad in (-1, 4097):
        with pytest.raises(_lib.MiError):
            t.set_option("group_lds_max", bad)
    with pytest.raises(_lib.MiError):
        t.set_option("group_blocks", -1)
    t.close()


# ---- the bound, NaN ---------------------------------------------------------------------------------------------------------------

def test_max_dist_and_nan_rows(orc, corpus):
    rows, q, _ = corpus
    rows = rows[:1000].copy()
    rows[17] = 0.0                                            # x.x = 0: its distance is NaN
    rows[500, 3] = np.nan
    d = orc_cosine_dist(orc, q, rows)
    assert np.isnan(d[17]) and np.isnan(d[500])
    groups = layout("mod7", 1000)
    groups[100:140] = NO_GROUP
    groups[17] = NO_GROUP                                     # a NaN singleton; row 500 is a NaN member of group 3
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    t.set_groups(groups)
    ids = np.arange(1000)
    finite = np.sort(d[~np.isnan(d)])
    for lds in (0, 4096):
        t.set_option("group_lds_max", lds)
        for k in (10, 100):
            got = check(t, d, ids, groups, q, k, what=("nan", k, lds))[5]
            assert got["nan"] == 2
            check(t, d, ids, groups, q, k, finite[499], what=("median", k, lds))
            r = int(np.flatnonzero(d == finite[37])[0])
            at = check(t, d, ids, groups, q, k, d[r], what=("at a row", k, lds))[5]      # inclusive: the row itself is in
            below = check(t, d, ids, groups, q, k, np.nextafter(d[r], np.float32(-1)), what=("below a row", k, lds))[5]
            assert at["window"] == below["window"] + int((d == d[r]).sum())
            idx, dist, group, members, facets, got = check(t, d, ids, groups, q, k, np.nextafter(finite[0], np.float32(-1)),
                                                           what=("below the minimum", k, lds))
            assert np.all(idx == NO_ID) and np.all(members == 0) and got == {"groups": 0, "window": 0, "beyond": 998, "nan": 2}
    t.close()


# ---- among ------------------------------------------------------------------------------------------------------------------------

def test_among(corpus):
    rows, q, d = corpus
    t = EmbeddingTable(768, 0)
    t.insert(rows[:1000])
    groups = layout("div65", 1000)
    groups[900:] = NO_GROUP
    t.set_groups(groups)
    t.delete([5, 64, 300])
    rng = np.random.default_rng(5)
    half = np.array([r for r in range(1000) if r % 65 < 32])   # cuts every group in half
    shuffled = rng.choice(1000, 400, replace=False)
    shuffled = np.concatenate([shuffled, shuffled[:130], [5, 64]])   # duplicates and deleted ids: allowed, left out
    rng.shuffle(shuffled)
    for among in (half, shuffled):
        keep = np.array(sorted(set(int(a) for a in among) - {5, 64, 300}))
        for lds in (0, 4096):
            t.set_option("group_lds_max", lds)
            for k in (10, 100):
                check(t, d[keep], keep, groups[keep], q, k, among=among, what=("among", k, lds))
                check(t, d[keep], keep, groups[keep], q, k, np.sort(d[keep])[60], among=among, what=("among bound", k, lds))
    rc, idx, dist, group, members, facets, totals = call(t, q, 3, among=[])
    assert rc == 0 and np.all(idx == NO_ID) and np.all(np.isinf(dist)) and np.all(group == NO_GROUP) and np.all(members == 0)
    assert np.all(totals == 0) and np.all(facets[:-2] == 0) and np.all(facets[-2:] == 7)
    rc, idx, dist, group, members, facets, totals = call(t, q, 5, among=[1, 2, 1000])     # an id that is no row
    assert rc == MI_ERR_INVALID and np.all(idx == 7) and np.all(dist == -7.0) and np.all(group == 7) and np.all(members == 7)
    assert np.all(facets == 7) and np.all(totals == 7)
    t.close()


# ---- deletes, appends -------------------------------------------------------------------------------------------------------------

def test_deletes_and_appends(orc, corpus):
    rows, q, d = corpus
    n0 = 1000
    t = EmbeddingTable(768, 0)
    t.insert(rows[:n0])
    groups = layout("mod7", n0)
    t.set_groups(groups)
    ids = np.arange(n0)
    idx, dist, group, members, facets, got = check(t, d[:n0], ids, groups, q, 7, what="before")
    rep, g = int(idx[2]), int(group[2])
    t.delete([rep])                                           # the representative goes: the group's next row takes over
    live = ids[ids != rep]
    idx2, dist2, group2, members2, facets2, _ = check(t, d[live], live, groups[live], q, 7, what="representative deleted")
    j = group2.tolist().index(g)
    assert idx2[j] != rep and members2[j] == members[2] - 1 and facets2[g] == facets[g] - 1
    t.delete(ids[groups == 5])                                # a whole group goes: no hit, an empty facet
    live = live[groups[live] != 5]
    idx3, dist3, group3, members3, facets3, got3 = check(t, d[live], live, groups[live], q, 7, what="group deleted")
    assert 5 not in group3.tolist() and facets3[5] == 0 and got3["groups"] == 6 and np.sum(idx3 != NO_ID) == 6
    # appended rows are singletons, and the column survives a grow that reallocates
    new = rows[n0:n0 + 3000]
    t.insert(new)
    all_groups = np.concatenate([groups, np.full(3000, NO_GROUP, np.uint32)])
    assert np.array_equal(t.groups(), all_groups) and t.groups_info() == {"n_groups": 7, "rows": n0}
    live = np.concatenate([live, np.arange(n0, n0 + 3000)])
    for lds in (0, 4096):
        t.set_option("group_lds_max", lds)
        check(t, d[live], live, all_groups[live], q, 100, what=("appended", lds))
    t.set_groups([3, NG], ids=[n0 + 1, 4])                    # by id; a row leaves its group
    all_groups[n0 + 1], all_groups[4] = 3, NO_GROUP
    assert t.groups([4, n0 + 1, 0]).tolist() == [NG, 3, 0] and t.groups_info()["rows"] == n0
    check(t, d[live], live, all_groups[live], q, 100, what="set by id")
    with pytest.raises(_lib.MiError):
        t.set_groups([1 << 24], ids=[0])                      # a group id out of range
    with pytest.raises(_lib.MiError):
        t.set_groups([1, 2], ids=[0, n0 + 3000])              # an id that is no row: nothing written
    assert t.groups([0])[0] == 0
    t.close()


# ---- limits -----------------------------------------------------------------------------------------------------------------------

def test_limits_and_errors_write_nothing(corpus, table5000):
    rows, q, d = corpus
    t = table5000
    t.set_groups(layout("mod7"))
    lib = _lib.lib()

    def untouched(got, code):
        rc, idx, dist, group, members, facets, totals = got
        assert rc == code, (rc, lib.mi_last_error())
        assert np.all(idx == 7) and np.all(dist == -7.0) and np.all(group == 7) and np.all(members == 7) and np.all(facets == 7) and np.all(totals == 7)

    assert call(t, q, 4096)[0] == 0
    untouched(call(t, q, 4097), MI_ERR_UNSUPPORTED)
    untouched(call(t, q, 0), MI_ERR_INVALID)
    untouched(call(t, q, 4, max_dist=np.nan), MI_ERR_INVALID)
    untouched(call(t, q, 4, among=[N]), MI_ERR_INVALID)
    n_groups = t.groups_info()["n_groups"]
    untouched(call(t, q, 4, cap_facets=n_groups - 1), MI_ERR_INVALID)
    # group, members, facets and totals may be NULL
    idx, dist = np.full(4, 7, np.uint64), np.full(4, -7.0, np.float32)
    assert lib.mi_knn_search_grouped(t._h, q.ctypes.data, 4, np.inf, None, 0, idx.ctypes.data, dist.ctypes.data, None, None, None, 0, None) == 0
    assert np.array_equal(idx, expected_grouped(d, np.arange(N), layout("mod7"), 4)[0])
    assert lib.mi_knn_search_grouped(t._h, None, 4, np.inf, None, 0, idx.ctypes.data, dist.ctypes.data, None, None, None, 0, None) == MI_ERR_INVALID
    odd = EmbeddingTable(192, 0)
    odd.insert(np.ones((3, 192), np.float32))
    assert call(odd, np.ones(192, np.float32), 2)[0] == MI_ERR_UNSUPPORTED    # a dim outside the set
    odd.close()
    e = EmbeddingTable(768, 0)                                # an empty table: all padding, zero counts
    rc, idx, dist, group, members, facets, totals = call(e, q, 3)
    assert rc == 0 and np.all(idx == NO_ID) and np.all(np.isinf(dist)) and np.all(group == NO_GROUP) and np.all(members == 0) and np.all(totals == 0)
    e.close()


# ---- identity (d) -----------------------------------------------------------------------------------------------------------------

def test_every_hit_is_the_filtered_top_1_of_its_group(corpus, table5000):
    rows, q, d = corpus
    t, groups = table5000, layout("random300")
    t.set_groups(groups)
    idx, dist, group, members, totals = t.knn_grouped(q, 200)
    rng = np.random.default_rng(3)
    for j in rng.choice(200, 10, replace=False):
        among = np.flatnonzero(groups == group[j]) if group[j] != NO_GROUP else [int(idx[j])]
        f_idx, f_dist = t.knn(q, 1, within=among)
        assert f_idx[0] == idx[j] and bits(f_dist[0]) == bits(dist[j])
    hits, dist2, group2, members2, totals2, facets = t.knn_grouped(q, 200, facets=True)
    assert np.array_equal(hits, idx) and totals2 == totals and facets.size == 300
    assert int(facets.sum()) + int((groups == NO_GROUP).sum()) == totals["window"] == N


# ---- the sharded table ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_shards", [1, 2, 3])
def test_sharded_equals_the_restatement(corpus, n_shards):
    rows, q, d = corpus
    n = 1000
    sh = ShardedTable(768, devices=(0,) * n_shards, block_rows=64)
    sh.insert(rows[:n])
    ids = np.arange(n)
    groups = layout("mod7", n)                                # every group has rows in every shard
    groups[::9] = NO_GROUP
    groups[700:764] = 11                                      # a group inside one block: one shard alone knows it
    sh.set_groups(groups)
    assert np.array_equal(sh.groups(), groups) and sh.groups_info() == {"n_groups": 12, "rows": int((groups != NO_GROUP).sum())}
    assert sh.groups([763, 0, 9]).tolist() == [11, NG, NG]
    for k in (5, 100):
        check(sh, d[:n], ids, groups, q, k, what=("sharded", n_shards, k))
        check(sh, d[:n], ids, groups, q, k, np.sort(d[:n])[300], what=("sharded bound", n_shards, k))
    sh.delete([0, 63, 64, 70, 500])
    live = np.array([r for r in range(n) if r not in (0, 63, 64, 70, 500)])
    check(sh, d[live], live, groups[live], q, 20, what=("sharded deleted", n_shards))
    among = np.random.default_rng(9).choice(n, 300, replace=False)
    keep = np.array(sorted(set(int(a) for a in among) - {0, 63, 64, 70, 500}))
    check(sh, d[keep], keep, groups[keep], q, 20, among=among, what=("sharded among", n_shards))
    # members and totals without the facets; the Python surface
    idx, dist, group, members, totals = sh.knn_grouped(q, 20, within=among)
    w = expected_grouped(d[keep], keep, groups[keep], 20, n_groups=12)
    assert np.array_equal(idx, w[0]) and np.array_equal(members, w[3]) and totals == w[5]
    rc = call(sh, q, 5, among=[n])[0]
    assert rc == MI_ERR_INVALID
    with pytest.raises(_lib.MiError):
        sh.set_groups([1], ids=[n])
    # rebalance into two shards keeps the column
    two = ShardedTable(768, devices=(0, 0), block_rows=128)
    two.rebalance_from(sh)
    assert np.array_equal(two.groups(), groups)
    check(two, d[live], live, groups[live], q, 20, what=("rebalanced", n_shards))
    two.close()
    sh.close()


# ---- the index --------------------------------------------------------------------------------------------------------------------

def test_image_index_web_search_grouped(orc, corpus, tmp_path):
    rows, q, _ = corpus
    rows = rows[:40].copy()
    dirs = ["", "trip/", "trip/day1/", "trip/day10/", "home/", "home/cat/"]
    which = np.random.default_rng(4).integers(0, 6, 40)
    which[:6] = [2, 0, 4, 1, 5, 3]                             # first seen in this order: ids 0..5 = day1, media, home, trip, cat, day10
    order = [2, 0, 4, 1, 5, 3]
    gid = np.array([order.index(w) for w in which], np.uint32)
    paths = [f"/srv/media/{dirs[w]}{i:03d}.jpg" for i, w in enumerate(which)]
    ix = ImageIndex(768, 0, "/srv/media/")
    ix.insert(paths[:25], rows[:25])
    refs = ["media/" + paths[j][len("/srv/media/"):] for j in (3, 12)]
    query = refine_query(q, [rows[3], rows[12]])
    d = orc_cosine_dist(orc, query, rows)

    def against(hits, totals, facets, live, k, among_dir=None, groups=gid, name=None):
        name = name or (lambda g: "media/" + dirs[order[g]])
        keep = np.array([r for r in live if among_dir is None or paths[r].startswith(among_dir)])
        w = expected_grouped(d[keep], keep, groups[keep], k, n_groups=int(groups.max()) + 1)
        n = int((w[0] != NO_ID).sum())
        assert [h[0] for h in hits] == w[0][:n].tolist() and [h[4] for h in hits] == w[3][:n].tolist()
        assert np.array_equal(bits(np.array([h[2] for h in hits], np.float32)), bits(w[1][:n]))
        assert [h[3] for h in hits] == [name(int(g)) for g in w[2][:n]]
        assert [h[1] for h in hits] == ["media/" + paths[h[0]][len("/srv/media/"):] for h in hits]
        assert totals == w[5] and facets == {name(g): int(c) for g, c in enumerate(w[4]) if c}

    hits, totals, facets = ix.web_search_grouped(q, refs, k=10, facets=True)
    against(hits, totals, facets, range(25), 10)
    ix.insert(paths[25:], rows[25:])                          # only the new rows are uploaded
    hits, totals, facets = ix.web_search_grouped(q, refs, k=10, facets=True)
    against(hits, totals, facets, range(40), 10)
    assert ix.group_count() == 6
    for g in range(6):
        assert ix.group_name(g) == "media/" + dirs[order[g]] and ix.group_name(g, web=False) == "/srv/media/" + dirs[order[g]]
    with pytest.raises(_lib.MiError):
        ix.group_name(6)
    best = next(h for h in hits if h[0] not in (3, 12))       # a directory's best file goes (not one of the marked images)
    ix.remove([paths[best[0]]])
    live = [r for r in range(40) if r != best[0]]
    hits, totals, facets = ix.web_search_grouped(q, refs, k=10, facets=True)
    against(hits, totals, facets, live, 10)
    assert best[0] not in [h[0] for h in hits] and facets.get(best[3], 0) == best[4] - 1
    hits, totals, facets = ix.web_search_grouped(q, (), k=10, folders=("media/trip",), facets=True)   # folders restrict the candidates
    d = orc_cosine_dist(orc, q, rows)
    against(hits, totals, facets, live, 10, among_dir="/srv/media/trip/")
    assert all(h[3].startswith("media/trip/") for h in hits) and "media/trip/day10/" in facets
    assert ix.web_search_grouped(q, (), k=5, folders=("media/none",)) == ([], {"groups": 0, "window": 0, "beyond": 0, "nan": 0})
    # by = an integer array, then the folders again
    labels = (np.arange(40) % 3).astype(np.uint32)
    labels[7] = NO_GROUP
    hits, totals, facets = ix.web_search_grouped(q, (), k=10, by=labels, facets=True)
    against(hits, totals, facets, live, 10, groups=labels, name=lambda g: None if g == NG else g)
    hits, totals, facets = ix.web_search_grouped(q, (), k=10, by="folder", facets=True)
    against(hits, totals, facets, live, 10)
    # save and load: the column is not saved, the index uploads everything again
    ix.save(str(tmp_path / "ix"))
    ix.close()
    ix2 = ImageIndex.load(str(tmp_path / "ix"))
    assert ix2.table.groups_info() == {"n_groups": 0, "rows": 0}
    hits, totals, facets = ix2.web_search_grouped(q, (), k=10, facets=True)
    against(hits, totals, facets, live, 10)
    ix2.close()
