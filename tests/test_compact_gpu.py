"""mi_knn_compact, mi_index_compact and mi_knn_sharded_compact_into on the GPU.  numpy is the oracle for what moves (rows by
bit pattern, columns, the id map), orc_knn over the live rows for the searches right after the call, and a FRESH table given
the survivors and their columns for everything else: every call must return the same bits on both."""
import ctypes
import os

import numpy as np
import pytest

from image_search_amd import _lib, synth
from image_search_amd._lib import MiError
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable, embed_all_images_in_dir
from oracle.binding import orc_knn
from test_representatives_gpu import SIZES, make_world
from test_summary_host import MI_ERR_INVALID, MI_ERR_UNSUPPORTED

pytestmark = pytest.mark.gpu

DIM = 768
N = 1157
S = 64            # "compact_chunk_rows": 1157 rows span 18 chunks and a ragged one
NO_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_GROUP = np.uint32(0xFFFFFFFF)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """two results of the library, to the bit (a NaN equals the NaN with the same bits)"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return a == b or (a != a and b != b)
    return a == b


@pytest.fixture(scope="module")
def world(built, orc):
    """the fixture of tests/test_representatives_gpu.py (a zero row, a NaN row, exact copies, groups with an empty one) plus
    tags and stamps on a subset of the rows"""
    w = make_world(orc, DIM, SIZES, N, 0, 11)
    rng = np.random.default_rng(5)
    g = w["labels"].astype(np.uint32)                            # NO_LABEL = NO_GROUP: the unlabelled rows hold no group
    w["groups"] = np.where(g == 2, 5, np.where(g == 5, 2, g)).astype(np.uint32)   # the highest group id holds ONE row
    w["attr_rows"] = np.sort(rng.choice(N, 500, replace=False))
    w["tags"] = np.zeros(N, np.uint64)
    w["stamps"] = np.zeros(N, np.int64)
    w["tags"][w["attr_rows"]] = rng.integers(0, 16, 500).astype(np.uint64)
    w["stamps"][w["attr_rows"]] = rng.integers(-1000, 1000, 500)
    w["queries"] = np.concatenate([w["rows"][[20, 700]], rng.standard_normal((2, DIM)).astype(np.float32)])
    return w


def patterns(w):
    rng = np.random.default_rng(9)
    every = np.arange(N)
    return {
        "none": every[:0],
        "row 0 only": every[:1],
        "last row only": every[-1:],
        "every other row": every[::2],
        "a run longer than S": every[200:200 + S + 9],
        "a run exactly S": every[200:200 + S],
        "everything": every,
        "the tail only": every[N - 90:],
        "random": np.sort(rng.choice(N, 300, replace=False)),
        # 65 rows: row 3 first (the first chunk sees one deleted row below it: staged), a run of 63 from row 400 on (behind it 64
        # rows are gone: straight), and the only row of the group with the highest id (a fresh table never hears of that
        # group); 1157 - 65 - 3 = 1089 rows move: 18 chunks of 64
        "mixed": np.unique(np.concatenate([[3], np.flatnonzero(w["groups"] == 5), np.setdiff1d(every[400:470], np.flatnonzero(w["groups"] == 5))[:63]])),
    }


PATTERNS = ["none", "row 0 only", "last row only", "every other row", "a run longer than S", "a run exactly S", "everything",
            "the tail only", "random", "mixed"]


def table_of(w, dead, base=0, chunk=S, dim=DIM):
    t = EmbeddingTable(dim, 0, base)
    t.set_option("compact_chunk_rows", chunk)
    t.insert(w["rows"])
    t.set_groups(w["groups"])
    t.set_attrs(w["attr_rows"].astype(np.uint64) + np.uint64(base), w["tags"][w["attr_rows"]], w["stamps"][w["attr_rows"]])
    if len(dead):
        t.delete(np.asarray(dead, np.uint64) + np.uint64(base))
    return t


def fresh_of(w, dead, base=0):
    """a fresh table given the survivors by insert and their columns by set_groups / set_attrs"""
    live = np.setdiff1d(np.arange(N), dead)
    t = EmbeddingTable(DIM, 0, base)
    t.set_option("compact_chunk_rows", S)
    if live.size:
        t.insert(w["rows"][live])
        t.set_groups(w["groups"][live])
        has = np.isin(live, w["attr_rows"])
        t.set_attrs(np.flatnonzero(has).astype(np.uint64) + np.uint64(base), w["tags"][live][has], w["stamps"][live][has])
    return t


def expected_map(n, dead, base=0):
    m = np.full(n, NO_ID, np.uint64)
    live = np.setdiff1d(np.arange(n), dead)
    m[live] = np.arange(live.size, dtype=np.uint64) + np.uint64(base)
    return m, live


def check_right_after(orc, w, t, res, dead, base=0, ks=(1, 10, 100)):
    want_map, live = expected_map(N, dead, base)
    L = live.size
    assert res["removed"] == len(dead) and np.array_equal(res["new_ids"], want_map)
    assert len(t) == L and t.deleted().size == 0
    if L == 0:
        return
    assert np.array_equal(bits(t.rows(0, L)), bits(w["rows"][live]))
    tags, stamps = t.get_attrs()
    assert np.array_equal(tags, w["tags"][live]) and np.array_equal(stamps, w["stamps"][live])
    assert np.array_equal(t.groups(), w["groups"][live])
    assert t.groups_info()["n_groups"] == 6                       # the high-water mark stays
    for q in w["queries"]:
        for k in ks:
            oi, od = orc_knn(orc, q, w["rows"][live], k, base=base)
            gi, gd = t.knn(q, k)
            assert np.array_equal(gi, oi) and np.array_equal(bits(gd), bits(od)), (k, gi[:5], oi[:5])


@pytest.mark.parametrize("name", PATTERNS)
def test_dead_patterns_right_after_the_call(orc, world, name):
    dead = patterns(world)[name]
    t = table_of(world, dead)
    res = t.compact()
    check_right_after(orc, world, t, res, dead)
    st = t.compact_stats()
    _, live = expected_map(N, dead)
    first = int(dead[0]) if len(dead) else N
    moved = max(live.size - first, 0) if len(dead) else 0
    assert st["removed"] == len(dead) and st["moved"] == moved
    assert st["straight"] + st["staged"] == -(-moved // S)
    if name == "none":
        assert st == {"removed": 0, "moved": 0, "straight": 0, "staged": 0}
    if name == "the tail only":
        assert st["moved"] == 0                                    # nothing moves
    if name == "mixed":
        assert st["staged"] > 0 and st["straight"] > 0 and st["straight"] + st["staged"] == 18   # both chunk kinds occur
    if name == "a run longer than S":
        assert st["staged"] == 0                                   # every chunk's first source lies beyond the chunk
    t.close()


def test_every_call_answers_as_on_a_fresh_table(orc, world):
    w = world
    dead = patterns(w)["mixed"]
    q = w["queries"]
    for pf in (1, 2):          # a mirror built BEFORE the compaction: the moved rows must be mirrored again
        t, f = table_of(w, dead), fresh_of(w, dead)
        t.set_option("prefilter", pf)
        f.set_option("prefilter", pf)
        t.knn(q[0], 10)
        t.compact()
        for k in (10, 100):
            assert same(t.knn(q, k), f.knn(q, k)), (pf, k)
        if pf == 1:
            t.close(); f.close()
    for pf in (0, 1, 2):
        t.set_option("prefilter", pf)
        f.set_option("prefilter", pf)
        for k in (1, 10, 100, 1000):
            assert same(t.knn(q, k), f.knn(q, k)), (pf, k)
    t.set_option("prefilter", 0)
    f.set_option("prefilter", 0)
    for u in range(len(q)):
        assert same(t.knn_where(q[u], 10, any_of=3, stamp=(-500, 500)), f.knn_where(q[u], 10, any_of=3, stamp=(-500, 500)))
        assert same(t.knn_where(q[u], 100, none_of=1, group=0), f.knn_where(q[u], 100, none_of=1, group=0))
        a, b = t.knn_grouped(q[u], 20, facets=True), f.knn_grouped(q[u], 20, facets=True)
        assert same(a[:5], b[:5])
        n_fresh = b[5].size                                        # the fresh table never heard of the highest group
        assert n_fresh < a[5].size and np.array_equal(a[5][:n_fresh], b[5]) and not a[5][n_fresh:].any()
        pa, pb = t.knn_page(q[u], 50), f.knn_page(q[u], 50)
        assert same(pa, pb)
        assert same(t.knn_page(q[u], 50, after=pa[3]), f.knn_page(q[u], 50, after=pb[3]))
    assert same(t.near_pairs(0.34), f.near_pairs(0.34))
    assert same(t.dbscan(0.34, 5), f.dbscan(0.34, 5))
    assert same(t.neighbors(5), f.neighbors(5))
    assert same(t.kmeans(8, max_iters=3, seed=5), f.kmeans(8, max_iters=3, seed=5))
    sa, sb = t.summarize(), f.summarize()
    assert sa.keys() == sb.keys()
    for key in sa:                                                 # per-group arrays over the fresh table's groups
        if isinstance(sa[key], np.ndarray) and sa[key].shape[:1] != sb[key].shape[:1]:
            assert same(sa[key][:sb[key].shape[0]], sb[key]), key
        else:
            assert same(sa[key], sb[key]), key
    t.close(); f.close()


def test_afterwards_the_table_is_an_ordinary_one(orc, world, mi, tmp_path):
    w = world
    base = 1000
    dead = patterns(w)["mixed"]
    t = table_of(w, dead, base)
    res = t.compact()
    check_right_after(orc, w, t, res, dead, base, ks=(10,))        # set_base is honoured: ids start at base
    _, live = expected_map(N, dead)
    L = live.size
    # an append reuses the freed rows: id base + L, live, default columns
    extra = synth.corpus_rows(3, 0, 2)
    t.insert(extra)
    assert len(t) == L + 2
    gi, gd = t.knn(extra[1], 1)
    assert gi[0] == base + L + 1
    tags, stamps = t.get_attrs()
    assert not tags[L:].any() and not stamps[L:].any() and np.all(t.groups()[L:] == NO_GROUP)
    assert t.knn_where(extra[0], 1, group=0)[0][0] != base + L     # the device column too: the reused row holds no group
    assert t.knn_where(extra[0], 5, stamp=(0, 0), none_of=0xFFFF)[0][0] == base + L   # ... and tags 0, stamp 0
    # a delete and a second compaction
    rows2 = np.concatenate([w["rows"][live], extra])
    dead2 = np.array([0, 5, L, L - 1])
    assert t.delete(dead2.astype(np.uint64) + np.uint64(base)) == 4
    res2 = t.compact()
    live2 = np.setdiff1d(np.arange(L + 2), dead2)
    assert res2["removed"] == 4 and len(t) == L - 2 and t.deleted().size == 0
    assert np.array_equal(res2["new_ids"][live2], np.arange(L - 2, dtype=np.uint64) + np.uint64(base))
    assert np.array_equal(bits(t.rows(0, L - 2)), bits(rows2[live2]))
    assert np.array_equal(t.groups(), np.concatenate([w["groups"][live], [NO_GROUP] * 2])[live2])
    oi, od = orc_knn(orc, w["queries"][0], rows2[live2], 10, base=base)
    gi, gd = t.knn(w["queries"][0], 10)
    assert np.array_equal(gi, oi) and np.array_equal(bits(gd), bits(od))
    # save writes the file of a table that never had deletions; load gives the same answers
    path = str(tmp_path / "t.miknn")
    _lib.check(mi.mi_knn_save(t._h, path.encode()))
    assert os.path.getsize(path) == 32 + (L - 2) * DIM * 4
    assert open(path, "rb").read(8) == b"MIKNNv01"
    t2 = EmbeddingTable(DIM, 0)
    _lib.check(mi.mi_knn_load(t2._h, path.encode()))
    assert len(t2) == L - 2 and same(t2.knn(w["queries"], 100), t.knn(w["queries"], 100))
    t.close(); t2.close()


def test_100k_rows_one_percent_deleted_default_chunk(orc, built):
    n = 100_000
    t = EmbeddingTable(DIM, 0)
    t.insert_synthetic(77, 0, n)
    dead = np.sort(np.random.default_rng(1).choice(n, n // 100, replace=False))
    t.delete(dead.astype(np.uint64))
    res = t.compact()
    want_map, live = expected_map(n, dead)
    assert res["removed"] == dead.size and np.array_equal(res["new_ids"], want_map)
    st = t.compact_stats()
    assert st["moved"] == live.size - dead[0] and st["straight"] + st["staged"] == -(-st["moved"] // ((64 << 20) // (DIM * 4)))
    rows = synth.corpus_rows(77, 0, n)[live]
    assert len(t) == live.size and np.array_equal(bits(t.rows(0, live.size)), bits(rows))
    for q in synth.corpus_rows(78, 0, 2):
        for k in (10, 1000):
            oi, od = orc_knn(orc, q, rows, k)
            gi, gd = t.knn(q, k)
            assert np.array_equal(gi, oi) and np.array_equal(bits(gd), bits(od)), k
    t.close()


@pytest.mark.parametrize("dim", [128, 256])
def test_other_dims(orc, built, dim):
    n = 101
    rng = np.random.default_rng(dim)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    dead = np.array([0, 7, 8, 9, 50, 99])
    t = EmbeddingTable(dim, 0)
    t.set_option("compact_chunk_rows", 16)
    t.insert(rows)
    t.delete(dead.astype(np.uint64))
    res = t.compact()
    want_map, live = expected_map(n, dead)
    assert res["removed"] == 6 and np.array_equal(res["new_ids"], want_map)
    assert np.array_equal(bits(t.rows(0, live.size)), bits(rows[live]))
    st = t.compact_stats()
    assert st["staged"] > 0 and st["straight"] + st["staged"] == -(-live.size // 16)
    oi, od = orc_knn(orc, rows[3], rows[live], 10)
    gi, gd = t.knn(rows[3], 10)
    assert np.array_equal(gi, oi) and np.array_equal(bits(gd), bits(od))
    t.close()


def test_errors_leave_the_table_untouched(world, mi):
    w = world
    dead = patterns(w)["random"]
    t = table_of(w, dead)
    small = np.zeros(N - 1, np.uint64)
    removed = ctypes.c_uint64(7)
    assert mi.mi_knn_compact(t._h, small.ctypes.data, N - 1, ctypes.byref(removed)) == MI_ERR_INVALID   # cap too small
    assert len(t) == N and np.array_equal(t.deleted(), dead.astype(np.uint64)) and np.array_equal(bits(t.rows(0, N)), bits(w["rows"]))
    assert not small.any() and removed.value == 7
    assert mi.mi_knn_compact(None, None, 0, None) == MI_ERR_INVALID                                        # a null handle
    t.close()
    # a shard borrowed from a sharded table: its ids are not its own to renumber
    sh = ShardedTable(DIM, [0, 0], 64)
    sh.insert(w["rows"][:300])
    sh.delete(np.array([1, 70, 200], np.uint64))
    shard = _lib.c_vp(mi.mi_knn_sharded_shard(sh._h, 1))
    assert mi.mi_knn_compact(shard, None, 0, None) == MI_ERR_UNSUPPORTED
    assert len(sh) == 300 and np.array_equal(sh.deleted(), [1, 70, 200]) and np.array_equal(bits(sh.rows(0, 300)), bits(w["rows"][:300]))
    sh.close()


def test_index_compact_names_the_same_paths(built, tmp_path):
    n = 60
    rows = synth.corpus_rows(90, 0, n)
    paths = [f"/m/{'abc'[i % 3]}/{'xy'[i % 2]}/img{i}.jpg" for i in range(n)]
    ix = ImageIndex(DIM, 0, "/m/")
    ix.insert(paths, rows)
    gone = [paths[i] for i in (0, 4, 5, 6, 30, 59)]
    assert ix.remove(gone) == 6
    q = synth.corpus_rows(91, 0, 2)

    def answers(x):
        text = [[(p, d) for _, p, d in x.web_search_text(v, ["media/a/x/img12.jpg"], 20)] for v in q]
        within = [[(p, d) for _, p, d in x.web_search_text(v, (), 20, folders=["media/b"])] for v in q]
        grouped = []
        for v in q:
            hits, totals, facets = x.web_search_grouped(v, (), 10, facets=True)
            grouped.append(([h[1:] for h in hits], totals, facets))
        return text, within, grouped, x.folder_overview()

    before = answers(ix)
    res = ix.compact()
    kept = [p for p in paths if p not in gone]
    want_map, live = expected_map(n, [0, 4, 5, 6, 30, 59])
    assert res["removed"] == 6 and np.array_equal(res["new_ids"], want_map)
    assert len(ix) == len(kept) == len(ix.table) and ix.table.deleted().size == 0
    assert [ix.path(i) for i in range(len(kept))] == kept
    assert ix.rows_of(kept) == list(range(len(kept))) and ix.rows_of(gone) == []
    assert ix.existing(paths) == set(kept) and ix.live_paths() == set(kept)
    assert np.array_equal(bits(ix.table.rows(0, len(kept))), bits(rows[live]))
    assert same(answers(ix), before)
    d = str(tmp_path / "ix")
    ix.save(d)
    assert os.path.getsize(os.path.join(d, "embedding.miknn")) == 32 + len(kept) * DIM * 4
    assert open(os.path.join(d, "embedding.miknn"), "rb").read(8) == b"MIKNNv01"
    ix2 = ImageIndex.load(d, 0, DIM)
    assert len(ix2) == len(kept) and [ix2.path(i) for i in range(len(kept))] == kept
    assert same(answers(ix2), before)
    assert ix2.insert(["/m/a/x/img0.jpg"], rows[:1]) == len(kept)  # the path comes back as the next row
    ix.close(); ix2.close()


def test_scan_compacts_after_a_prune_when_asked(built, tmp_path):
    class Rows:                                                    # "decode" yields the embedding itself
        def forward_images(self, images):
            return np.stack(images)

    def decode(path):
        return synth.corpus_rows(60, int(os.path.basename(path)[2:-4]), 1)[0]

    for above, compacted in ((0.0, True), (0.9, False), (None, False)):
        media = tmp_path / f"media_{above}"
        (media / "a").mkdir(parents=True)
        for i in range(6):
            (media / "a" / f"im{i}.png").write_bytes(b"")
        ix = ImageIndex(DIM, 0, str(media) + "/")
        assert embed_all_images_in_dir(Rows(), ix, str(media), image_chunk_size=4, decode=decode, shuffle_seed=1) == 6
        os.remove(media / "a" / "im1.png")
        os.remove(media / "a" / "im4.png")
        assert embed_all_images_in_dir(Rows(), ix, str(media), decode=decode, prune=True, compact_above=above) == 0
        left = {str(media / "a" / f"im{i}.png") for i in (0, 2, 3, 5)}
        assert ix.live_paths() == left
        if compacted:
            assert len(ix) == 4 == len(ix.table) and ix.table.deleted().size == 0
            assert {ix.path(i) for i in range(4)} == left
            for i in range(4):                                     # every row still stands under its own path
                assert np.array_equal(bits(ix.table.rows(i, 1)[0]), bits(decode(ix.path(i))))
        else:
            assert len(ix) == 6 and ix.table.deleted().size == 2
        ix.close()


@pytest.mark.parametrize("n_shards", [2, 3])
def test_sharded_compact_into_equals_a_fresh_sharded_table(world, n_shards):
    w = world
    dead = patterns(w)["mixed"]
    _, live = expected_map(N, dead)
    src = ShardedTable(DIM, [0] * n_shards, 64)
    src.insert(w["rows"])
    src.set_groups(w["groups"])
    src.set_attrs(w["attr_rows"].astype(np.uint64), w["tags"][w["attr_rows"]], w["stamps"][w["attr_rows"]])
    src.delete(dead.astype(np.uint64))
    q = w["queries"]
    before = (src.knn(q, 100), src.groups(), src.get_attrs(), src.deleted())
    dst = ShardedTable(DIM, [0] * n_shards, 64)
    res = dst_res = src.compact_into(dst)
    want_map, _ = expected_map(N, dead)
    assert res["removed"] == dead.size and np.array_equal(dst_res["new_ids"], want_map)
    fresh = ShardedTable(DIM, [0] * n_shards, 64)
    fresh.insert(w["rows"][live])
    fresh.set_groups(w["groups"][live])
    has = np.isin(live, w["attr_rows"])
    fresh.set_attrs(np.flatnonzero(has).astype(np.uint64), w["tags"][live][has], w["stamps"][live][has])
    assert len(dst) == live.size == len(fresh) and dst.deleted().size == 0
    assert np.array_equal(bits(dst.rows(0, live.size)), bits(w["rows"][live]))
    for k in (10, 100):
        assert same(dst.knn(q, k), fresh.knn(q, k))
    assert same(dst.get_attrs(), fresh.get_attrs()) and same(dst.groups(), fresh.groups())
    assert np.array_equal(dst.groups(), w["groups"][live]) and np.array_equal(dst.get_attrs()[0], w["tags"][live])
    # src answers as before, and a destination that holds rows is refused
    assert len(src) == N and same((src.knn(q, 100), src.groups(), src.get_attrs(), src.deleted()), before)
    with pytest.raises(MiError) as e:
        src.compact_into(dst)
    assert e.value.code == MI_ERR_INVALID and len(dst) == live.size
    src.close(); dst.close(); fresh.close()
