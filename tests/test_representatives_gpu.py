"""mi_knn_representatives on the GPU: every output against the numpy restatement (tests/test_representatives_host.py) over the
oracle's distances (oracle.c: the bits mi_knn_search reports), to the bit — picks, gaps, counts, reach, rep and rep_dist."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable
from test_kmeans_seed_host import oracle_dist_from
from test_page_host import dist_key
from test_representatives_host import NO_ROW, restate_representatives
from test_summary_host import MI_ERR_INVALID, MI_ERR_UNSUPPORTED, NO_LABEL

pytestmark = pytest.mark.gpu

DIM = 768
N = 1157          # 9 tiles of 128 and a ragged 5
C = 6
NO_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
NEG_INF = np.float32(-np.inf)
SIZES = {0: 600, 1: 0, 2: 1, 3: 20, 4: 260, 5: 120}      # 0 spans two segments of the walk (512 members each); 1 is empty
ARRAYS = ("rows", "gap", "n_picked", "reach", "rep", "rep_dist", "stands_for")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                 b.view(np.uint32) if b.dtype == np.float32 else b)


def same_result(a, b):
    return all(same_bits(a[k], b[k]) for k in ARRAYS) and a["totals"] == b["totals"]


def check(res, want, labels, member, m, base=0, what=""):
    """the device's dict against the restatement's, to the bit"""
    ids = np.where(want["rows"] == NO_ROW, NO_ID, want["rows"].astype(np.uint64) + np.uint64(base))
    assert np.array_equal(res["rows"], ids), (what, np.argwhere(res["rows"] != ids)[:4], res["rows"][res["rows"] != ids][:4], ids[res["rows"] != ids][:4])
    assert np.array_equal(res["n_picked"], want["n_picked"]), what
    assert np.array_equal(bits(res["gap"]), bits(want["gap"])), (what, np.argwhere(bits(res["gap"]) != bits(want["gap"]))[:4])
    assert np.array_equal(bits(res["reach"]), bits(want["reach"])), (what, res["reach"], want["reach"])
    assert np.array_equal(res["rep"], want["rep"]), (what, np.flatnonzero(res["rep"] != want["rep"])[:8])
    nan = np.isnan(want["rep_dist"])
    assert np.array_equal(np.isnan(res["rep_dist"]), nan), what
    assert np.array_equal(bits(res["rep_dist"])[~nan], bits(want["rep_dist"])[~nan]), what
    # what follows from the contract, whatever the restatement says
    n_groups = res["rows"].shape[0]
    for c in range(n_groups):
        k = int(res["n_picked"][c])
        keys = dist_key(res["gap"][c, 1:k])
        assert np.all(keys[:-1] >= keys[1:]), (what, c)
        assert np.all(np.isposinf(res["gap"][c, k:])) and np.all(res["rows"][c, k:] == NO_ID) and (k == 0 or np.isposinf(res["gap"][c, 0]))
        mem = np.flatnonzero(member & (labels == c))
        measured = mem[~np.isnan(res["rep_dist"][mem])]
        assert np.all(dist_key(res["rep_dist"][measured]) <= dist_key(res["reach"][c])), (what, c)
        assert int(res["stands_for"][c].sum()) == measured.size and not np.any(res["stands_for"][c, k:])
    has = want["rep"] != NO_LABEL
    assert np.array_equal(res["stands_for"].reshape(-1), np.bincount(labels[has].astype(np.int64) * m + want["rep"][has], minlength=n_groups * m))
    inside = member & (labels < n_groups)
    assert np.all(res["rep"][~inside] == NO_LABEL) and np.all(np.isposinf(res["rep_dist"][~inside]))
    k = res["n_picked"].astype(np.int64)
    assert res["totals"] == {"members": int(inside.sum()), "groups": int((k > 0).sum()), "picks": int(k.sum()), "rounds": int(k.max())}, what


def make_world(orc, dim, sizes, n, n_dead, seed):
    """rows, labels, live, usable, dist_from: groups of the given sizes scattered over the table, the rest unlabelled; a group
    of exact copies (group 3); one live zero row and one live row of NaN, both labelled; n_dead deleted rows"""
    rng = np.random.default_rng(seed)
    themes = rng.standard_normal((8, dim)).astype(np.float32)
    rows = (themes[rng.integers(0, 8, n)] + 0.7 * rng.standard_normal((n, dim))).astype(np.float32)
    rows *= rng.uniform(0.1, 10.0, (n, 1)).astype(np.float32)
    labels = np.concatenate([np.full(s, c, np.uint32) for c, s in sizes.items()] + [np.full(n - sum(sizes.values()), NO_LABEL, np.uint32)])
    labels = labels[rng.permutation(n)]
    copies = np.flatnonzero(labels == 3)
    rows[copies] = rows[copies[0]]
    big = max(sizes, key=sizes.get)
    zero, nan = np.flatnonzero(labels == big)[[5, 11]]
    rows[zero] = 0.0
    rows[nan] = np.nan
    dead = rng.choice(np.setdiff1d(np.arange(n), np.concatenate([copies, [zero, nan], np.flatnonzero(labels == 2)])), n_dead, replace=False)
    live = np.ones(n, bool)
    live[dead] = False
    dist_from, usable = oracle_dist_from(orc, rows)
    assert not usable[zero] and not usable[nan] and usable.sum() == n - 2
    return {"rows": rows, "labels": labels, "live": live, "member": live & usable, "dead": np.sort(dead), "dist_from": dist_from,
            "zero": int(zero), "nan": int(nan)}


def table_of(w, dim, base=0):
    t = EmbeddingTable(dim, 0)
    if base:
        t.set_base(base)
    t.insert(w["rows"])
    t.delete(w["dead"] + base)
    return t


@pytest.fixture(scope="module")
def world(built, orc):
    w = make_world(orc, DIM, SIZES, N, 40, 7)
    w["table"] = table_of(w, DIM)
    yield w
    w["table"].close()


def restate(w, n_groups, m, min_gap=NEG_INF, start=None, labels=None):
    return restate_representatives(w["dist_from"], w["labels"] if labels is None else labels, w["member"], n_groups, m, np.float32(min_gap), start)


# 1: m, against the restatement over the oracle's distances
@pytest.mark.parametrize("m", [1, 4, 16])
def test_picks_gaps_reach_and_rep_to_the_bit(world, m):
    w, t = world, world["table"]
    res = t.representatives(w["labels"], C, m, start="first")
    check(res, restate(w, C, m), w["labels"], w["member"], m, what=f"m {m}")
    assert res["n_picked"].tolist() == [m, 0, 1, min(m, 20), m, m]
    assert np.isposinf(res["reach"][1]) and res["rows"][2, 0] == np.flatnonzero(w["labels"] == 2)[0]
    assert res["rep"][w["zero"]] == NO_LABEL and np.isposinf(res["rep_dist"][w["zero"]]) and np.isposinf(res["rep_dist"][w["nan"]])
    copies = np.flatnonzero(w["labels"] == 3)
    assert res["rows"][3, :min(m, 20)].tolist() == copies[:min(m, 20)].tolist()         # exact copies: by id
    st = t.representatives_stats()
    count = np.array([int((w["member"] & (w["labels"] == c)).sum()) for c in range(C)])
    assert count[0] > 512 and st["rounds"] == m and st["segments"] == int(((count + 511) // 512).sum()) == 6
    print(f"m {m}: totals {res['totals']}, stats {st}, reach {res['reach']}")


def test_m_larger_than_the_largest_group_picks_every_measured_member(world):
    w, t = world, world["table"]
    m = 610
    res = t.representatives(w["labels"], C, m, start="first")
    check(res, restate(w, C, m), w["labels"], w["member"], m, what="m 610")
    count = np.array([int((w["member"] & (w["labels"] == c)).sum()) for c in range(C)])
    assert np.array_equal(res["n_picked"], count) and count.max() < m
    # the host stopped enqueuing once a round made no pick: at most one batch of 8 past the last pick
    assert count.max() <= t.representatives_stats()["rounds"] <= count.max() + 8
    for c in (0, 3, 4, 5):                                   # every member was picked: it stands for itself or an exact copy
        mem = np.flatnonzero(w["member"] & (w["labels"] == c))
        assert np.all(dist_key(res["rep_dist"][mem]) <= dist_key(res["reach"][c]))


# 2: min_gap
def test_min_gap_none_zero_and_exactly_a_picks_gap(world):
    w, t = world, world["table"]
    m = 16
    free = t.representatives(w["labels"], C, m, start="first")
    res = t.representatives(w["labels"], C, m, min_gap=0.0, start="first")
    check(res, restate(w, C, m, 0.0), w["labels"], w["member"], m, what="min_gap 0")
    assert res["n_picked"][3] == 1 or res["gap"][3, 1] > 0       # the copies: nothing lies above 0 (unless d(x, x) rounds above it)
    g = free["gap"][0, 7]                                        # exactly the gap of pick 7 of group 0: that pick is NOT made
    res = t.representatives(w["labels"], C, m, min_gap=float(g), start="first")
    check(res, restate(w, C, m, g), w["labels"], w["member"], m, what="min_gap = a gap")
    assert res["n_picked"][0] <= 7 and dist_key(res["reach"][0]) <= dist_key(g)
    below = np.nextafter(g, np.float32(0.0))
    res = t.representatives(w["labels"], C, m, min_gap=float(below), start="first")
    check(res, restate(w, C, m, below), w["labels"], w["member"], m, what="min_gap one ulp below")
    assert res["n_picked"][0] >= 8 and same_bits(res["rows"][0, :8], free["rows"][0, :8])


# 3: start; labels = NULL; a base
def test_start_at_the_cover_at_given_ids_and_at_the_first_member(world):
    w, t = world, world["table"]
    m = 4
    cover = t.summarize(w["labels"], C)["cover"]
    start = np.where(cover == NO_ID, 0, cover).astype(np.int64)
    res = t.representatives(w["labels"], C, m)                   # start="cover"
    check(res, restate(w, C, m, start=start), w["labels"], w["member"], m, what="cover")
    assert np.array_equal(res["rows"][:, 0], cover)
    rng = np.random.default_rng(3)
    given = np.array([rng.choice(np.flatnonzero(w["member"] & (w["labels"] == c))) if SIZES[c] else 10 ** 15 for c in range(C)])
    res = t.representatives(w["labels"], C, m, start=given)      # (the empty group's entry is no row at all)
    check(res, restate(w, C, m, start=given), w["labels"], w["member"], m, what="given")
    assert np.array_equal(res["rows"][[0, 2, 3, 4, 5], 0], given[[0, 2, 3, 4, 5]].astype(np.uint64))


def test_the_group_column_a_base_and_one_group_of_ids(world):
    w = world
    m, base = 4, 10 ** 12
    t = table_of(w, DIM, base)
    t.set_groups(w["labels"])
    want = restate(w, C, m)
    res = t.representatives(None, C, m, start="first")           # labels = NULL: the column, read where it lies
    check(res, want, w["labels"], w["member"], m, base=base, what="column + base")
    assert same_result(res, t.representatives(w["labels"], C, m, start="first"))
    cover = t.summarize()["cover"]
    assert np.all(cover[cover != NO_ID] >= base)
    res = t.representatives(m=m)                                 # the defaults: the column, n_groups from it, the cover
    start = np.where(cover == NO_ID, 0, cover - np.uint64(base)).astype(np.int64)
    check(res, restate(w, C, m, start=start), w["labels"], w["member"], m, base=base, what="defaults")
    # representatives_of: one group made of ids (deleted and unusable rows among them are no members)
    ids = np.flatnonzero(w["labels"] == 5)
    one = t.representatives_of(ids + base, m=6, start="first")
    lab = np.where(w["labels"] == 5, 0, NO_LABEL).astype(np.uint32)
    check(one, restate(w, 1, 6, labels=lab), lab, w["member"], 6, base=base, what="representatives_of")
    t.close()


# 4: other dims, on a smaller table
@pytest.mark.parametrize("dim", [128, 256])
def test_other_dims(built, orc, dim):
    sizes = {0: 40, 1: 0, 2: 1, 3: 20, 4: 17, 5: 9}
    w = make_world(orc, dim, sizes, 101, 6, 100 + dim)
    t = table_of(w, dim)
    for m, min_gap in ((5, NEG_INF), (48, NEG_INF), (48, 0.3)):     # 48: larger than the largest group
        res = t.representatives(w["labels"], C, m, min_gap=float(min_gap), start="first")
        check(res, restate(w, C, m, min_gap), w["labels"], w["member"], m, what=f"dim {dim} m {m} min_gap {min_gap}")
    t.close()


# 5: what pick 1 is, said with the search
def test_pick_1_is_the_member_the_filtered_search_ranks_last(world):
    w, t = world, world["table"]
    res = t.representatives(w["labels"], C, 2, start="first")
    for c in (0, 3, 4, 5):
        mem = np.flatnonzero(w["member"] & (w["labels"] == c))
        p0 = int(res["rows"][c, 0])
        others = mem[mem != p0]
        idx, d = t.knn(w["rows"][p0], others.size, within=others)
        ok = (idx != NO_ID) & ~np.isnan(d)
        idx, d = idx[ok], d[ok]
        assert bits(d[-1:])[0] == bits(res["gap"][c, 1:2])[0], c
        assert int(res["rows"][c, 1]) == int(idx[bits(d) == bits(d[-1:])[0]].min()), c      # the lowest id among equal keys


# 6: the same bits every time
def test_deterministic_across_calls_handles_and_the_prefilter(world):
    w, t = world, world["table"]
    a, b = t.representatives(w["labels"], C, 9), t.representatives(w["labels"], C, 9)
    t2 = table_of(w, DIM)
    c = t2.representatives(w["labels"], C, 9)
    t2.set_option("prefilter", 1)
    t2.knn(w["rows"][0], 10)
    d = t2.representatives(w["labels"], C, 9)
    t2.close()
    assert same_result(a, b) and same_result(a, c) and same_result(a, d)


# 7: errors write nothing
def test_errors_write_nothing_and_leave_the_table_usable(world):
    w, t = world, world["table"]
    mi = _lib.lib()
    m = 3
    want = t.representatives(w["labels"], C, m, start="first")
    out = {}

    def fresh():
        out.update(picks=np.full(C * m, 7, np.uint64), gap=np.full(C * m, -7.0, np.float32), n=np.full(C, 7, np.uint32),
                   reach=np.full(C, -7.0, np.float32), rep=np.full(N, 7, np.uint32), rep_dist=np.full(N, -7.0, np.float32),
                   totals=np.full(4, 7, np.uint64))

    def call(h, c=C, mm=m, min_gap=float("-inf"), start=None, lab=w["labels"]):
        return mi.mi_knn_representatives(h, lab.ctypes.data, c, mm, min_gap, start.ctypes.data if start is not None else None,
                                         out["picks"].ctypes.data, out["gap"].ctypes.data, out["n"].ctypes.data, out["reach"].ctypes.data,
                                         out["rep"].ctypes.data, out["rep_dist"].ctypes.data, out["totals"].ctypes.data)

    def untouched():
        return (np.all(out["picks"] == 7) and np.all(out["gap"] == -7.0) and np.all(out["n"] == 7) and np.all(out["reach"] == -7.0)
                and np.all(out["rep"] == 7) and np.all(out["rep_dist"] == -7.0) and np.all(out["totals"] == 7))

    fresh()
    assert call(None) == MI_ERR_INVALID and call(t._h, c=0) == MI_ERR_INVALID and call(t._h, mm=0) == MI_ERR_INVALID
    assert call(t._h, min_gap=float("nan")) == MI_ERR_INVALID
    assert call(t._h, c=65537) == MI_ERR_UNSUPPORTED and call(t._h, mm=4097) == MI_ERR_UNSUPPORTED
    assert call(t._h, c=65536, mm=65) == MI_ERR_UNSUPPORTED
    good = want["rows"][:, 0].copy()
    for c, bad_id in ((0, int(np.flatnonzero(w["labels"] == 4)[0])),          # a row of another group
                      (4, int(w["dead"][w["labels"][w["dead"]] == 4][0])),      # a deleted row of the group
                      (0, w["zero"]),                                           # an unusable row of the group
                      (5, N), (5, 2 ** 63)):                                    # no row of the table
        start = good.copy()
        start[c] = bad_id
        assert call(t._h, start=start) == MI_ERR_INVALID, (c, bad_id)
        assert b"not a member" in mi.mi_last_error()
    for dim in (64, 192):                                                       # dims the scans are not built for
        odd = EmbeddingTable(dim, 0)
        odd.insert(np.ones((4, dim), np.float32))
        assert call(odd._h, c=2) == MI_ERR_UNSUPPORTED
        odd.close()
    sh = ShardedTable(DIM, (0, 0), 64)
    sh.insert(w["rows"][:256])
    assert call(ctypes.c_void_p(mi.mi_knn_sharded_shard(sh._h, 0))) == MI_ERR_UNSUPPORTED       # a borrowed shard
    sh.close()
    assert untouched()
    assert same_result(want, t.representatives(w["labels"], C, m, start="first"))
    # every output may be NULL; an empty table answers with the padding
    assert mi.mi_knn_representatives(t._h, w["labels"].ctypes.data, C, m, float("-inf"), *([None] * 8)) == 0
    assert call(t._h) == 0 and np.array_equal(out["picks"].reshape(C, m), want["rows"]) and np.array_equal(out["rep"], want["rep"])
    empty = EmbeddingTable(DIM, 0)
    e = empty.representatives(n_groups=3, m=2)
    assert np.all(e["rows"] == NO_ID) and np.all(np.isposinf(e["gap"])) and not np.any(e["n_picked"]) and np.all(np.isposinf(e["reach"]))
    assert e["rep"].size == 0 and not np.any(e["stands_for"]) and e["totals"]["picks"] == 0
    assert empty.representatives_stats() == {"rounds": 0, "segments": 0, "rows_last_round": 0}
    empty.close()


# 8: the index
def test_index_highlights(built):
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
    over = {o["folder"]: o for o in ix.folder_overview()}
    high = ix.folder_highlights(m=3)
    assert [h["folder"] for h in high] == ["/media/trip/", "/media/home/", "/media/work/scans/"]
    res = ix.table.representatives(None, ix.group_count(), 3)
    for h in high:
        g = ix.group_of("media/" + h["folder"][len("/media/"):])
        k = int(res["n_picked"][g])
        assert h["highlights"] == [ix.path(int(r)) for r in res["rows"][g, :k]] and h["highlights"][0] == over[h["folder"]]["cover"]
        assert [np.float32(v) for v in h["gaps"][1:]] == res["gap"][g, 1:k].tolist() and np.isposinf(h["gaps"][0])
        assert gone not in h["highlights"] and all(p.startswith(h["folder"]) for p in h["highlights"])
    assert high[0]["highlights"][1] == "/media/trip/stray.jpg" and len(high[2]["highlights"]) == 2
    assert [len(h["highlights"]) for h in ix.folder_highlights(m=3, min_gap=0.5)] == [2, 1, 1]     # the stray alone lies that far off
    assert ix.folder_highlights(m=2, web=True)[0]["highlights"][0].startswith("media/trip/")
    trip = [p for p in paths if p.startswith("/media/trip/")]
    got = ix.highlights(trip + paths[-3:-1], m=3)
    want = ix.table.representatives_of(ix.rows_of(trip + paths[-3:-1]), m=3)
    assert got == [ix.path(int(r)) for r in want["rows"][0, :3]] and gone not in got and len(set(got)) == 3
    assert ix.highlights([gone], m=3) == [] and ix.highlights([], m=3) == []
    ix.close()
