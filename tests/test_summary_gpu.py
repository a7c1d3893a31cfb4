"""mi_knn_summarize on the GPU: per group its centroid, cover, odd one out, measured count and spread.

Centroids: against fp64 means of x / |x| under the bound tests/test_kmeans_gpu.py uses for one k-means update, and against
k-means' own centroids bit for bit.  dist: its bits against orc_cosine_dist(row, the returned centroid of the row's group)
(oracle.c).  Everything else: equality with the numpy restatement (tests/test_summary_host.py) fed the device's own dist."""
import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, typical_order
from oracle.binding import orc_cosine_dist
from test_assign_gpu import DIM, N_CLUSTERS, N_PLANTED, planted_corpus
from test_summary_host import MI_ERR_INVALID, MI_ERR_UNSUPPORTED, NO_LABEL, check_same, expected_summary

pytestmark = pytest.mark.gpu

NO_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZES = [0, 1, 2, 15, 16, 17, 511, 512, 513, 1025]   # then one group with the rest but 100, and 100 rows unlabelled
ARRAYS = ("centroids", "count", "cover", "cover_dist", "odd", "odd_dist", "measured", "spread", "dist")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_result(a, b):
    return all(same_bits(a[k], b[k]) if a[k].dtype == np.float32 else np.array_equal(a[k], b[k]) for k in ARRAYS) and a["totals"] == b["totals"]


def check_centroids(rows, member, labels, cent, groups):
    """fp64 means of x / |x| under 4 (n_c + 8) 2^-24 mean|unit| — the bound of test_one_update_against_fp64_means; an empty
    group's centroid is all +0"""
    worst = 0.0
    for c in groups:
        m = member & (labels == c)
        n_c = int(m.sum())
        if n_c == 0:
            assert not np.any(bits(cent[c])), c
            continue
        x = rows[m].astype(np.float64)
        unit = x / np.linalg.norm(x, axis=1, keepdims=True)
        want = unit.mean(axis=0)
        bound = 4.0 * (n_c + 8) * 2.0 ** -24 * np.abs(unit).mean(axis=0)
        err = np.abs(cent[c].astype(np.float64) - want)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (c, n_c, float(np.max(err / bound)))
    return worst


def check_dist(orc, rows, labels, C, live, usable, res, sample=None):
    """dist [rows]: a member's bits = the oracle's for (row, the returned centroid of its group); NaN for an unusable live row
    with a label < C; +inf elsewhere"""
    n = rows.shape[0]
    inside = live & (labels < C)
    member = inside & usable
    got = res["dist"]
    assert np.all(np.isposinf(got[~inside])) and np.all(np.isnan(got[inside & ~usable]))
    todo = np.flatnonzero(member) if sample is None else sample[member[sample]]
    want = np.array([orc_cosine_dist(orc, rows[r], res["centroids"][labels[r]][None, :])[0] for r in todo], np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got[todo]), nan)
    assert np.array_equal(bits(got[todo])[~nan], bits(want)[~nan]), np.flatnonzero(bits(got[todo]) != bits(want))[:8]
    return n


def check_all(orc, t, rows, labels, C, live=None, usable=None, base=0, res=None, what=""):
    n = rows.shape[0]
    labels = np.asarray(labels).astype(np.uint32)
    live = np.ones(n, bool) if live is None else live
    usable = np.ones(n, bool) if usable is None else usable
    res = t.summarize(labels, C) if res is None else res
    member = live & usable & (labels < C)
    worst = check_centroids(rows, member, labels, res["centroids"], range(C) if C <= 64 else np.unique(labels[member])[:16])
    check_dist(orc, rows, labels, C, live, usable, res)
    want = expected_summary(labels, live, usable, res["dist"], np.arange(n, dtype=np.uint64) + np.uint64(base), C)
    check_same(res, want, what)
    ok = res["measured"] > 0
    assert np.all(np.isnan(res["mean_dist"][~ok]))
    assert np.array_equal(res["mean_dist"][ok], res["spread"][ok].astype(np.float64) / res["measured"][ok].astype(np.float64) * 2.0 ** -30)
    print(f"{what}: totals {res['totals']}, largest centroid error / bound {worst:.3f}, stats {t.summarize_stats()}")
    return res


@pytest.fixture(scope="module")
def gauss(built):
    rows = np.random.default_rng(21).standard_normal((4096, DIM)).astype(np.float32)
    rows *= np.random.default_rng(22).uniform(0.1, 10.0, (4096, 1)).astype(np.float32)
    sizes = SIZES + [4096 - sum(SIZES) - 100]
    labels = np.concatenate([np.full(s, c, np.uint32) for c, s in enumerate(sizes)] + [np.full(100, NO_LABEL, np.uint32)])
    labels = labels[np.random.default_rng(23).permutation(4096)]      # members are not contiguous
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    yield rows, labels, len(sizes), t
    t.close()


# 1: segment edges
def test_segment_edges_against_the_oracle_and_the_restatement(gauss, orc):
    rows, labels, C, t = gauss
    res = check_all(orc, t, rows, labels, C, what="segment edges")
    assert res["count"].tolist() == SIZES + [4096 - sum(SIZES) - 100]
    assert res["totals"] == {"members": 3996, "outside": 100, "unusable": 0, "groups": C - 1}
    st = t.summarize_stats()
    assert st["segments"] == sum((s + 511) // 512 for s in res["count"].tolist()) and st["rows"] == 3996
    assert res["cover"][0] == NO_ID and np.isposinf(res["cover_dist"][0]) and res["odd"][0] == NO_ID
    assert res["cover"][1] == res["odd"][1] == np.flatnonzero(labels == 1)[0]       # a group of one
    order = typical_order(labels, res["dist"], C)
    for c in range(C):
        assert order[c].size == res["count"][c]
        if order[c].size:
            assert order[c][0] == res["cover"][c] and bits(res["dist"])[order[c][-1]] == bits(res["odd_dist"])[c]


# 2: identities with k-means, no tolerance
def test_one_kmeans_update_is_the_summary_of_its_assign(gauss):
    rows, _, _, t = gauss
    c0 = rows[100:164].copy()
    c0[5] = -rows[0] - rows[1]   # (far from everything: most likely an empty cluster)
    lab, d = t.assign(c0)
    res = t.kmeans(c0, max_iters=1)
    assert res["iters"] == 1
    s = t.summarize(np.where(np.isnan(d), np.uint32(NO_LABEL), lab), 64)
    filled = np.flatnonzero(s["count"])
    assert filled.size >= 32
    assert same_bits(s["centroids"][filled], res["centroids"][filled])
    assert np.array_equal(s["count"], np.bincount(lab[~np.isnan(d)].astype(np.int64), minlength=64).astype(np.uint64))


def test_converged_kmeans_is_reproduced_to_the_bit(built):
    rows, vectors, own = planted_corpus()
    rows = rows[:N_PLANTED]
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    res = t.kmeans(rows[:N_CLUSTERS].copy(), max_iters=20)
    assert res["changed"] == 0 and res["iters"] < 20
    s = t.summarize(res["labels"])
    assert s["centroids"].shape == (N_CLUSTERS, DIM)
    assert same_bits(s["centroids"], res["centroids"]) and same_bits(s["dist"], res["dist"])
    members = s["totals"]["members"]
    assert members == N_PLANTED == int(s["measured"].sum())
    mean = float(int(s["spread"].sum())) * 2.0 ** -30 / members
    print("mean dist", mean, "objective / members", res["objective"] / members)
    # w truncates d * 2^30: every member loses less than 2^-30, so does the mean
    assert abs(res["objective"] / members - mean) <= 2.0 ** -30
    t.close()


# 3: other dims; fewer rows than a wave's groups
@pytest.mark.parametrize("dim,n,C", [(128, 600, 3), (1024, 600, 3), (DIM, 7, 1)])
def test_other_dims_and_tiny_tables(built, orc, dim, n, C):
    rng = np.random.default_rng(31 + dim + n)
    rows = (rng.standard_normal((n, dim)) * rng.uniform(0.1, 10.0, (n, 1))).astype(np.float32)
    labels = rng.integers(0, C, n).astype(np.uint32)
    t = EmbeddingTable(dim, 0)
    t.insert(rows)
    check_all(orc, t, rows, labels, C, what=f"dim {dim}, {n} rows")
    t.close()


# 4: rows that do not count
def test_deleted_unusable_and_cancelling_rows(built, orc):
    rng = np.random.default_rng(41)
    n = 1500
    rows = rng.standard_normal((n, DIM)).astype(np.float32)
    labels = rng.integers(0, 4, n).astype(np.uint32)
    rows[50] = 0.0
    rows[51, 3] = np.nan
    rows[52, 7] = np.inf
    rows[53] *= np.float32(1e-30)     # the squared norm underflows to 0
    rows[54] *= np.float32(1e19)      # ... overflows to inf
    labels[50:55] = [0, 1, 2, 3, 0]
    rows[61] = -rows[60]              # a group {x, -x}: the centroid is exactly 0
    labels[60:62] = 4
    dead = np.unique(rng.integers(100, n, 200))
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    t.delete(dead)
    live, usable = np.ones(n, bool), np.ones(n, bool)
    live[dead] = False
    usable[50:55] = False
    res = check_all(orc, t, rows, labels, 5, live=live, usable=usable, what="rows that do not count")
    assert res["totals"]["unusable"] == 5 and np.all(np.isnan(res["dist"][50:55]))
    assert np.all(np.isposinf(res["dist"][dead]))
    assert not np.any(bits(res["centroids"][4])) and np.all(np.isnan(res["dist"][60:62]))
    assert res["count"][4] == 2 and res["measured"][4] == 0 and res["spread"][4] == 0
    assert res["cover"][4] == 60 and np.isnan(res["cover_dist"][4]) and res["odd"][4] == NO_ID and np.isposinf(res["odd_dist"][4])
    assert np.isnan(res["mean_dist"][4])
    # usable is the search's own verdict: the row against itself
    for r, want in ((50, False), (53, False), (54, False), (60, True), (0, True)):
        idx, d = t.knn(rows[r], 1, within=[r])
        assert (idx[0] == r and not np.isnan(d[0])) == want, r
    # the same rows without the ones that must not count: the same centroids, to the bit
    keep = live & usable
    t2 = EmbeddingTable(DIM, 0)
    t2.insert(rows[keep])
    res2 = t2.summarize(labels[keep], 5)
    assert same_bits(res["centroids"], res2["centroids"]) and same_bits(res["dist"][keep], res2["dist"])
    assert np.array_equal(res["count"], res2["count"]) and np.array_equal(res["spread"], res2["spread"])
    t.close()
    t2.close()


# 5: ties
def test_ties_go_to_the_lowest_id(built, orc):
    rng = np.random.default_rng(51)
    rows = rng.standard_normal((700, DIM)).astype(np.float32)
    labels = np.zeros(700, np.uint32)
    rows[[30, 200, 201, 650]] = rows[30]        # four copies of one row among others
    labels[600:] = 1
    labels[[650]] = 0
    rows[100:140] = rows[100]                   # a group of identical rows only
    labels[100:140] = 2
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    res = check_all(orc, t, rows, labels, 3, what="ties")
    assert len(set(bits(res["dist"][[30, 200, 201, 650]]).tolist())) == 1
    assert len(set(bits(res["dist"][100:140]).tolist())) == 1
    assert res["cover"][2] == 100 and res["odd"][2] == 100 and res["count"][2] == 40
    order = typical_order(labels, res["dist"], 3)
    assert order[2].tolist() == list(range(100, 140))
    pos = {int(r): i for i, r in enumerate(order[0])}
    assert pos[200] == pos[30] + 1 and pos[201] == pos[30] + 2 and pos[650] == pos[30] + 3
    t.close()


# 6: labels = None reads the table's group column
def test_the_group_column_is_read_in_place(gauss):
    rows, labels, C, _ = gauss
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    never = t.summarize(n_groups=3)              # a column that was never set: every row belongs to nothing
    assert not np.any(never["count"]) and np.all(never["cover"] == NO_ID) and not np.any(bits(never["centroids"]))
    assert never["totals"] == {"members": 0, "outside": 4096, "unusable": 0, "groups": 0} and np.all(np.isposinf(never["dist"]))
    assert t.summarize()["count"].shape == (1,)
    t.set_groups(labels)
    assert t.groups_info()["n_groups"] == C
    a, b = t.summarize(), t.summarize(t.groups())
    assert a["count"].shape == (C,) and same_result(a, b)
    assert same_result(a, t.summarize(labels, C))
    t.insert(rows[:300])                         # rows appended afterwards belong to nothing
    c = t.summarize()
    assert c["dist"].shape == (4396,) and np.all(np.isposinf(c["dist"][4096:]))
    assert all(same_bits(a[k], c[k]) if a[k].dtype == np.float32 else np.array_equal(a[k], c[k]) for k in ARRAYS if k != "dist")
    assert c["totals"]["outside"] == a["totals"]["outside"] + 300 and c["totals"]["members"] == a["totals"]["members"]
    assert same_result(c, t.summarize(t.groups()))
    t.close()


# 7: the largest C (the histogram sizing n_waves = 2^24 / (C + 1)) and ids that are not the rows
def test_65536_groups_and_a_base(gauss, orc):
    rows, _, _, _ = gauss
    labels = np.random.default_rng(71).integers(0, 65536, 4096).astype(np.uint32)
    labels[:8] = 65535
    labels[8:11] = 0
    base = 10 ** 12
    t = EmbeddingTable(DIM, 0)
    t.set_base(base)
    t.insert(rows)
    res = check_all(orc, t, rows, labels, 65536, base=base, what="C 65536")
    assert res["count"][65535] >= 8 and res["count"][0] >= 3 and res["totals"]["members"] == 4096
    has = res["cover"] != NO_ID
    assert np.array_equal(has, res["count"] > 0) and np.all(res["cover"][has] >= base) and np.all(res["odd"][has] >= base)
    assert res["dist"].shape == (4096,) and int(res["cover"][0]) - base in np.flatnonzero(labels == 0)
    t.close()


# 8: determinism, and errors that write nothing
def test_deterministic_across_calls_and_handles(gauss):
    rows, labels, C, t = gauss
    a, b = t.summarize(labels, C), t.summarize(labels, C)
    t2 = EmbeddingTable(DIM, 0)
    t2.insert(rows)
    c = t2.summarize(labels, C)
    t2.close()
    assert same_result(a, b) and same_result(a, c)


def test_errors_write_nothing_and_leave_the_table_usable(gauss):
    rows, labels, C, t = gauss
    mi = _lib.lib()
    want = t.summarize(labels, C)
    cent = np.full((C, DIM), -7.0, np.float32)
    u64 = [np.full(C, 7, np.uint64) for _ in range(5)]
    f32 = [np.full(C, -7.0, np.float32) for _ in range(2)]
    dist, totals = np.full(4096, -7.0, np.float32), np.full(4, 7, np.uint64)

    def call(h, c, lab=labels):
        return mi.mi_knn_summarize(h, lab.ctypes.data, c, cent.ctypes.data, u64[0].ctypes.data, u64[1].ctypes.data, f32[0].ctypes.data,
                                   u64[2].ctypes.data, f32[1].ctypes.data, u64[3].ctypes.data, u64[4].ctypes.data, dist.ctypes.data,
                                   totals.ctypes.data)

    assert call(t._h, 0) == MI_ERR_INVALID and call(t._h, 65537) == MI_ERR_UNSUPPORTED and call(None, C) == MI_ERR_INVALID
    assert len(mi.mi_last_error()) > 0
    odd = EmbeddingTable(192, 0)
    odd.insert(np.ones((4, 192), np.float32))
    assert call(odd._h, 2) == MI_ERR_UNSUPPORTED
    odd.close()
    assert np.all(cent == -7.0) and all(np.all(a == 7) for a in u64) and all(np.all(a == -7.0) for a in f32)
    assert np.all(dist == -7.0) and np.all(totals == 7)
    assert same_result(want, t.summarize(labels, C))
    # every output may be NULL; an empty table answers with the padding
    assert mi.mi_knn_summarize(t._h, labels.ctypes.data, C, *([None] * 10)) == 0
    assert call(t._h, C) == 0 and same_bits(cent, want["centroids"]) and np.array_equal(u64[1], want["cover"])
    empty = EmbeddingTable(DIM, 0)
    e = empty.summarize(n_groups=3)
    assert not np.any(e["count"]) and np.all(e["cover"] == NO_ID) and np.all(np.isposinf(e["odd_dist"])) and e["dist"].size == 0
    assert not np.any(bits(e["centroids"])) and e["totals"]["groups"] == 0
    empty.close()


# 9: the index
def test_index_overviews(built):
    rng = np.random.default_rng(91)
    themes = rng.standard_normal((3, DIM)).astype(np.float32)
    emb, paths = [], []
    for c, (folder, n) in enumerate((("trip", 7), ("home", 4), ("work/scans", 2))):
        for i in range(n):
            paths.append(f"/media/{folder}/t{c}_{i}.jpg")
            emb.append(themes[c] + 0.2 * rng.standard_normal(DIM))
    paths.append("/media/trip/stray.jpg")          # a picture of the second theme in the first folder
    emb.append(themes[1] + 0.2 * rng.standard_normal(DIM))
    ix = ImageIndex(DIM, 0, "/media/")
    ix.insert(paths, np.asarray(emb, np.float32))
    gone = "/media/trip/t0_1.jpg"
    ix.remove([gone])
    over = ix.folder_overview()
    assert [(o["folder"], o["images"]) for o in over] == [("/media/trip/", 7), ("/media/home/", 4), ("/media/work/scans/", 2)]
    s = ix.table.summarize(ix.table.groups(), ix.group_count())
    for o in over:
        g = ix.group_of("media/" + o["folder"][len("/media/"):])
        assert o["images"] == s["count"][g] and o["cover"] == ix.path(int(s["cover"][g])) and o["odd_one_out"] == ix.path(int(s["odd"][g]))
        assert np.float32(o["cover_dist"]) == s["cover_dist"][g] and np.float32(o["odd_dist"]) == s["odd_dist"][g]
        assert o["mean_dist"] == s["mean_dist"][g] and o["cover"].startswith(o["folder"]) and o["cover"] != gone
    assert over[0]["odd_one_out"] == "/media/trip/stray.jpg"
    web = ix.folder_overview(web=True)
    assert web[0]["folder"] == "media/trip/" and web[0]["cover"].startswith("media/trip/")

    row_of = {p: r for r, p in enumerate(paths)}
    res = ix.table.kmeans(3, seed=0)
    clusters = ix.cluster_overview(3, seed=0)
    assert sum(c["images"] for c in clusters) == len(paths) - 1 and [c["images"] for c in clusters] == sorted((c["images"] for c in clusters), reverse=True)
    for c in clusters:
        assert res["labels"][row_of[c["cover"]]] == c["group"] and res["labels"][row_of[c["odd_one_out"]]] == c["group"]
        assert c["images"] == int((res["labels"] == c["group"]).sum()) and c["cover"] != gone
    labels = ix.table.dbscan(0.2, 2)["labels"]
    found = ix.theme_overview(0.2, 2)
    assert [t["images"] for t in found] == [6, 5, 2]
    for th in found:
        assert labels[row_of[th["cover"]]] == th["group"] and labels[row_of[th["odd_one_out"]]] == th["group"]
        assert th["cover_dist"] - 2.0 ** -30 <= th["mean_dist"] <= th["odd_dist"]    # (the mean sums truncated weights)
    assert ix.theme_overview(1e-6, 2) == []
    ix.close()


# 10: one larger run
def test_200k_rows_1000_groups(built, orc):
    n, C = 200_000, 1000
    t = EmbeddingTable(DIM, 0)
    t.insert_synthetic(5, 0, n)
    labels = np.random.default_rng(101).integers(0, C + 50, n).astype(np.uint32)    # 50 labels beyond C
    res = t.summarize(labels, C)
    live = usable = np.ones(n, bool)
    check_same(res, expected_summary(labels, live, usable, res["dist"], np.arange(n, dtype=np.uint64), C), "200k")
    assert res["totals"]["members"] == int((labels < C).sum()) and res["totals"]["groups"] == C
    sample = np.random.default_rng(102).choice(np.flatnonzero(labels < C), 64, replace=False)
    for r in sample:
        want = orc_cosine_dist(orc, t.rows(int(r), 1)[0], res["centroids"][labels[r]][None, :])
        assert bits(want)[0] == bits(res["dist"])[r], r
    for c in (0, 499, 999):
        m = np.flatnonzero(labels == c)
        rows = np.concatenate([t.rows(int(r), 1) for r in m])
        check_centroids(rows, np.ones(m.size, bool), np.full(m.size, c), {c: res["centroids"][c]}, [c])
    print("200k:", res["totals"], t.summarize_stats())
    t.close()
