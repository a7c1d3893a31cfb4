"""mi_knn_sharded_summarize on the GPU: every key of the dict equals, bit for bit, what one EmbeddingTable holding the same rows
returns with the option "kmeans_fixed_sum" on — for every shard count and block size — and the result stays tied to
restatements: dist to orc_cosine_dist(row, the returned centroid) (oracle.c), the centroids of a corpus whose norms are exact
to expected_fixed_update (tests/test_kmeans_sharded_host.py).  Every shard lives on device 0."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ShardedTable, typical_order
from test_assign_gpu import DIM, NO_LABEL
from test_kmeans_sharded_gpu import LAYOUTS, exact_corpus, shard_of
from test_kmeans_sharded_host import expected_fixed_update
from test_summary_gpu import ARRAYS, NO_ID, SIZES, bits, check_dist, same_bits
from test_summary_sharded_host import MI_ERR_INVALID, MI_ERR_UNSUPPORTED, exchange_bytes

pytestmark = pytest.mark.gpu

KEYS = set(ARRAYS) | {"mean_dist", "totals"}


def assert_same(got, want, what=""):
    """every key of summarize's dict: floats by their bits, the rest for equality"""
    assert set(got) == set(want) == KEYS, (what, sorted(got))
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        if got[k].dtype == np.float32:
            assert same_bits(got[k], want[k]), (what, k, np.flatnonzero(bits(got[k]).reshape(-1) != bits(want[k]).reshape(-1))[:8])
        else:
            assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8])
    assert np.array_equal(got["mean_dist"].view(np.uint64), want["mean_dist"].view(np.uint64)), (what, "mean_dist")
    assert got["totals"] == want["totals"], (what, got["totals"], want["totals"])


def one_table(rows, dim=DIM, dead=None):
    """the reference: one table holding the same rows, the option on"""
    t = EmbeddingTable(dim, 0)
    t.insert(rows)
    if dead is not None:
        t.delete(dead)
    t.set_option("kmeans_fixed_sum", 1)
    return t


def sharded(rows, shards, block, dim=DIM):
    t = ShardedTable(dim, [0] * shards, block)
    t.insert(rows)
    return t


@pytest.fixture(scope="module")
def corpus(built):
    """the group-size corpus of tests/test_summary_gpu.py (4 096 shuffled rows, 100 unlabelled, groups of 0, 1, 2, 15, 16, 17,
    511, 512, 513 and 1 025 members and the rest), and one more group, 11, carved out of the rest group's rows of the first 64:
    they lie in one block of every layout, so on one shard.  With the one table's answer (computed once)."""
    rows = np.random.default_rng(21).standard_normal((4096, DIM)).astype(np.float32)
    rows *= np.random.default_rng(22).uniform(0.1, 10.0, (4096, 1)).astype(np.float32)
    sizes = SIZES + [4096 - sum(SIZES) - 100]
    labels = np.concatenate([np.full(s, c, np.uint32) for c, s in enumerate(sizes)] + [np.full(100, NO_LABEL, np.uint32)])
    labels = labels[np.random.default_rng(23).permutation(4096)]
    one_block = np.flatnonzero(labels[:64] == 10)
    assert one_block.size >= 8
    labels[one_block] = 11
    C = 12
    t = one_table(rows)
    want = t.summarize(labels, C)
    assert want["count"].tolist() == SIZES + [sizes[-1] - one_block.size, one_block.size]
    yield rows, labels, C, want, t
    t.close()


@pytest.fixture(scope="module")
def exact(built):
    """exact_corpus of tests/test_kmeans_sharded_gpu.py with 8 random groups (one empty), and the restatement's centroids"""
    rows, inv = exact_corpus()
    labels = np.random.default_rng(42).integers(0, 9, rows.shape[0]).astype(np.uint32)
    labels[labels == 8] = NO_LABEL
    labels[labels == 5] = 4                                          # group 5 is empty: its centroid stays all zeros
    want = expected_fixed_update(rows, inv, labels, np.zeros(rows.shape[0], np.float32), 8, np.zeros((8, DIM), np.float32))
    return rows, labels, want


# 1: the one table's bits, for every layout
@pytest.mark.parametrize("shards,block", LAYOUTS)
def test_every_layout_equals_the_one_table(corpus, exact, orc, shards, block):
    rows, labels, C, want, _ = corpus
    on = [np.unique(shard_of(np.flatnonzero(labels == c), shards, block)).size for c in range(C)]
    assert max(on) == shards, on                                     # a group with members on every shard
    assert on[11] == 1 and on[0] == 0                                # ... one on a single shard, an empty one
    st = sharded(rows, shards, block)
    got = st.summarize(labels, C)
    assert_same(got, want, (shards, block))
    live = usable = np.ones(4096, bool)
    check_dist(orc, rows, labels, C, live, usable, got)              # dist against the oracle, on the returned centroids
    stats = st.summarize_stats()
    assert stats["members"] == 3996 == got["totals"]["members"] and stats["bytes_exchanged"] == exchange_bytes(shards, C, DIM)
    assert stats["merge_launches"] == 2 * (shards - 1)               # per other shard: one chunk of sums, one fold of slots
    assert sum((int(s) + 511) // 512 for s in want["count"]) <= stats["segments"] <= C * shards + 4096 // 512
    order = typical_order(labels, got["dist"], C)                    # global rows in, global rows out
    for c in range(C):
        assert order[c].size == got["count"][c]
        if order[c].size:
            assert order[c][0] == got["cover"][c] and bits(got["dist"])[order[c][-1]] == bits(got["odd_dist"])[c]
    st.close()
    # the centroids against the restatement, where x / |x| is exact
    xrows, xlabels, xwant = exact
    xs = sharded(xrows, shards, block)
    xgot = xs.summarize(xlabels, 8)
    assert same_bits(xgot["centroids"], xwant), (shards, block)
    assert xgot["count"][5] == 0 and not np.any(bits(xgot["centroids"][5]))
    xs.close()


# 2: ties go to the lowest GLOBAL id
def test_ties_across_shards(built):
    rng = np.random.default_rng(52)
    rows = rng.standard_normal((384, DIM)).astype(np.float32)
    labels = np.full(384, 2, np.uint32)
    first = [60, 64, 130, 200]              # one vector on shards 0, 1, 2 and 0; row 64 is local row 0 of shard 1
    second = [178, 202, 270]                # the lowest id on the last shard (local row 50), then shards 0 and 1
    rows[first], rows[second] = rows[60], rows[178]
    labels[first], labels[second] = 0, 1
    assert shard_of(first, 3, 64).tolist() == [0, 1, 2, 0] and shard_of(second, 3, 64).tolist() == [2, 0, 1]
    st, t = sharded(rows, 3, 64), one_table(rows)
    got = st.summarize(labels, 3)
    assert len(set(bits(got["dist"][first]).tolist())) == 1 and len(set(bits(got["dist"][second]).tolist())) == 1
    assert not np.isnan(got["dist"][60]) and not np.isnan(got["dist"][178])
    assert got["cover"][0] == 60 and got["odd"][0] == 60, (got["cover"][0], got["odd"][0])
    assert got["cover"][1] == 178 and got["odd"][1] == 178, (got["cover"][1], got["odd"][1])
    assert got["count"].tolist() == [4, 3, 377] and got["measured"].tolist() == [4, 3, 377]
    assert_same(got, t.summarize(labels, 3))
    st.close()
    t.close()


# 3: labels = None reads every shard's part of the group column
def test_the_group_column_is_read_on_every_shard(corpus):
    rows, labels, C, want, _ = corpus
    st = sharded(rows, 3, 64)
    never = st.summarize(n_groups=3)         # a column that was never set: every row belongs to nothing
    assert not np.any(never["count"]) and np.all(never["cover"] == NO_ID) and not np.any(bits(never["centroids"]))
    assert never["totals"] == {"members": 0, "outside": 4096, "unusable": 0, "groups": 0} and np.all(np.isposinf(never["dist"]))
    assert st.summarize()["count"].shape == (1,)
    st.set_groups(labels)
    assert st.groups_info()["n_groups"] == C
    a = st.summarize()
    assert a["count"].shape == (C,)
    assert_same(a, st.summarize(labels, C))
    assert_same(a, st.summarize(st.groups()))
    assert_same(a, want)
    st.close()


# 4: rows that do not count, spread over the shards; an empty shard
@pytest.mark.parametrize("shards,block", ((3, 64), (4, 960)))
def test_rows_that_do_not_count(built, shards, block):
    rng = np.random.default_rng(41)
    n, C = 2000, 4
    rows = rng.standard_normal((n, DIM)).astype(np.float32)
    labels = rng.integers(0, C + 1, n).astype(np.uint32)             # C: beyond the groups
    bad = np.array([50, 70, 130, 1000, 1930])
    rows[50] = 0.0
    rows[70, 3] = np.nan
    rows[130, 7] = np.inf
    rows[1000] *= np.float32(1e-30)     # the squared norm underflows to 0
    rows[1930] *= np.float32(1e19)      # ... overflows to inf
    labels[bad] = [0, 1, 2, 3, 0]
    assert np.unique(shard_of(bad, shards, block)).size == 3
    dead = np.setdiff1d(np.unique(rng.integers(100, n, 300)), bad)
    assert np.unique(shard_of(dead, shards, block)).size == 3
    t, st = one_table(rows, dead=dead), sharded(rows, shards, block)
    st.delete(dead.astype(np.uint64))
    if shards == 4:
        assert st.shard_rows(3) == 0 and st.shard_rows(2) > 0        # an empty shard takes part with zeros
    got = st.summarize(labels, C)
    assert_same(got, t.summarize(labels, C), (shards, block))
    live, usable = np.ones(n, bool), np.ones(n, bool)
    live[dead], usable[bad] = False, False
    inside = live & (labels < C)
    assert got["totals"] == {"members": int((inside & usable).sum()), "outside": int((live & (labels >= C)).sum()), "unusable": 5,
                             "groups": C}
    assert np.all(np.isnan(got["dist"][bad])) and np.all(np.isposinf(got["dist"][~inside]))
    assert not np.any(np.isnan(got["dist"][inside & usable])) and np.all(np.isfinite(got["centroids"]))
    assert np.array_equal(got["count"], np.bincount(labels[inside & usable].astype(np.int64), minlength=C).astype(np.uint64))
    assert not np.isin(got["cover"], dead).any() and not np.isin(got["odd"], bad).any()
    t.close()
    st.close()


# 5: a group that cancels across two shards
def test_a_cancelling_group_across_shards(built):
    rng = np.random.default_rng(53)
    rows = rng.standard_normal((256, DIM)).astype(np.float32)
    labels = rng.integers(0, 4, 256).astype(np.uint32)
    rows[70] = -rows[10]                # x on shard 0, -x on shard 1
    labels[[10, 70]] = 4
    st, t = sharded(rows, 3, 64), one_table(rows)
    got = st.summarize(labels, 5)
    assert not np.any(bits(got["centroids"][4])) and np.all(np.isnan(got["dist"][[10, 70]]))
    assert got["count"][4] == 2 and got["measured"][4] == 0 and got["spread"][4] == 0 and np.isnan(got["mean_dist"][4])
    assert got["cover"][4] == 10 and np.isnan(got["cover_dist"][4]) and got["odd"][4] == NO_ID and np.isposinf(got["odd_dist"][4])
    assert got["totals"]["unusable"] == 0 and got["totals"]["members"] == 256
    assert_same(got, t.summarize(labels, 5))
    st.close()
    t.close()


# 6: the step after k-means
def test_after_kmeans(corpus):
    # 64 planted themes far apart: k-means from one row of each stops within its 4 iterations with nothing changed
    rng = np.random.default_rng(61)
    themes = rng.standard_normal((64, DIM))
    own = np.arange(3072) % 64
    rows = ((themes[own] + 0.1 * rng.standard_normal((3072, DIM))) * rng.uniform(0.1, 10.0, (3072, 1))).astype(np.float32)
    st = sharded(rows, 3, 64)
    res = st.kmeans(rows[:64].copy(), max_iters=4)
    assert 1 <= res["iters"] <= 4 and res["changed"] == 0 and np.array_equal(res["labels"], own)
    s = st.summarize(res["labels"])
    assert s["centroids"].shape == (64, DIM)
    assert same_bits(s["centroids"], res["centroids"]) and same_bits(s["dist"], res["dist"])
    members = s["totals"]["members"]
    assert members == 3072 == int(s["measured"].sum())
    mean = float(int(s["spread"].sum())) * 2.0 ** -30 / members
    # w truncates d * 2^30: every member loses less than 2^-30, so does the mean
    assert abs(res["objective"] / members - mean) <= 2.0 ** -30, (res["objective"] / members, mean)
    st.close()
    # not converged (the Gaussian corpus, C = 64): update 4 is the summary of the assign behind update 3
    g = corpus[0]
    st = sharded(g, 3, 64)
    c0 = g[200:264].copy()
    three, four = st.kmeans(c0, max_iters=3), st.kmeans(c0, max_iters=4)
    assert three["iters"] == 3 and four["iters"] == 4
    s = st.summarize(np.where(np.isnan(three["dist"]), np.uint32(NO_LABEL), three["labels"]), 64)
    filled = np.flatnonzero(s["count"])
    assert filled.size >= 32 and same_bits(s["centroids"][filled], four["centroids"][filled])
    stayed = three["labels"] == four["labels"]          # (their distance is to the same centroid in both)
    print(f"{int(stayed.sum())} of 4096 rows kept their label in iteration 4")
    assert stayed.any() and same_bits(s["dist"][stayed], four["dist"][stayed])
    st.close()


# 7: more sums than one merge chunk holds
def test_more_than_one_merge_chunk(built):
    n, C = 3000, 4096
    assert C * DIM > 2 ** 21
    rng = np.random.default_rng(71)
    rows = rng.standard_normal((n, DIM)).astype(np.float32)
    labels = rng.integers(0, C, n).astype(np.uint32)
    labels[:9] = C - 1                  # the last group, in the second chunk, with members on both shards
    labels[200:209] = C - 1
    st, t = sharded(rows, 2, 128), one_table(rows)
    got = st.summarize(labels, C)
    assert_same(got, t.summarize(labels, C))
    assert got["count"][C - 1] >= 18 and np.unique(shard_of(np.flatnonzero(labels == C - 1), 2, 128)).size == 2
    stats = st.summarize_stats()
    assert stats["bytes_exchanged"] == exchange_bytes(2, C, DIM) == C * (8 * DIM + 36) + 4 * C * DIM
    assert stats["merge_launches"] == 2 + 1 and stats["members"] == n
    st.close()
    t.close()


# 8: other dims, tiny and empty tables, determinism, errors
@pytest.mark.parametrize("dim,n,C,shards", [(128, 600, 3, 3), (1024, 600, 3, 3), (DIM, 7, 1, 4)])
def test_other_dims_and_tiny_tables(built, orc, dim, n, C, shards):
    rng = np.random.default_rng(31 + dim + n)
    rows = (rng.standard_normal((n, dim)) * rng.uniform(0.1, 10.0, (n, 1))).astype(np.float32)
    labels = rng.integers(0, C, n).astype(np.uint32)
    st, t = sharded(rows, shards, 64, dim), one_table(rows, dim)
    got = st.summarize(labels, C)
    assert_same(got, t.summarize(labels, C), (dim, n))
    check_dist(orc, rows, labels, C, np.ones(n, bool), np.ones(n, bool), got)
    st.close()
    t.close()


def test_an_empty_table_answers_with_the_padding(built):
    st = ShardedTable(DIM, [0, 0, 0], 64)
    e = st.summarize(n_groups=3)
    assert not np.any(e["count"]) and np.all(e["cover"] == NO_ID) and np.all(np.isposinf(e["odd_dist"])) and e["dist"].size == 0
    assert not np.any(bits(e["centroids"])) and e["totals"] == {"members": 0, "outside": 0, "unusable": 0, "groups": 0}
    assert e["centroids"].shape == (3, DIM) and np.all(np.isposinf(e["cover_dist"])) and np.all(np.isnan(e["mean_dist"]))
    assert st.summarize_stats() == {"segments": 0, "bytes_exchanged": 0, "merge_launches": 0, "members": 0}
    one = EmbeddingTable(DIM, 0)
    assert_same(e, one.summarize(n_groups=3))
    one.close()
    st.close()


def test_deterministic_across_calls_and_handles(corpus):
    rows, labels, C, want, _ = corpus
    st, other = sharded(rows, 4, 64), sharded(rows, 4, 64)
    a, b, c = st.summarize(labels, C), st.summarize(labels, C), other.summarize(labels, C)
    assert_same(a, b)
    assert_same(a, c)
    assert_same(a, want)
    assert st.summarize_stats() == other.summarize_stats()
    st.close()
    other.close()


def test_errors_write_nothing_and_every_output_may_be_null(corpus):
    rows, labels, C, want, _ = corpus
    mi = _lib.lib()
    st = sharded(rows, 3, 64)

    def buffers():
        return [np.full((C, DIM), -7.0, np.float32), np.full(C, 7, np.uint64), np.full(C, 7, np.uint64), np.full(C, -7.0, np.float32),
                np.full(C, 7, np.uint64), np.full(C, -7.0, np.float32), np.full(C, 7, np.uint64), np.full(C, 7, np.uint64),
                np.full(4096, -7.0, np.float32), np.full(4, 7, np.uint64)]

    def untouched(bufs):
        return all(np.all(b == (-7.0 if b.dtype == np.float32 else 7)) for b in bufs)

    def call(h, c, bufs, lab=labels):
        return mi.mi_knn_sharded_summarize(h, lab.ctypes.data, c, *(None if b is None else b.ctypes.data for b in bufs))

    bufs = buffers()
    assert call(st._h, 0, bufs) == MI_ERR_INVALID and call(st._h, 65537, bufs) == MI_ERR_UNSUPPORTED
    assert call(None, C, bufs) == MI_ERR_INVALID and len(mi.mi_last_error()) > 0
    odd = ShardedTable(192, [0, 0], 64)
    odd.insert(np.ones((4, 192), np.float32))
    assert call(odd._h, 2, bufs) == MI_ERR_UNSUPPORTED
    odd.close()
    assert untouched(bufs)
    assert_same(st.summarize(labels, C), want)                       # the table is as usable as before
    names = ("centroids", "count", "cover", "cover_dist", "odd", "odd_dist", "measured", "spread", "dist")
    assert call(st._h, C, bufs) == 0
    for name, b in zip(names, bufs):
        assert same_bits(b, want[name]) if b.dtype == np.float32 else np.array_equal(b, want[name]), name
    assert bufs[9].tolist() == [want["totals"][k] for k in ("members", "outside", "unusable", "groups")]
    # every output pointer NULL in turn: the others are written as before
    for gone in range(10):
        bufs = buffers()
        assert call(st._h, C, [None if i == gone else b for i, b in enumerate(bufs)]) == 0, gone
        assert untouched([bufs[gone]])
        for i, (name, b) in enumerate(zip(names, bufs)):
            if i != gone:
                assert same_bits(b, want[name]) if b.dtype == np.float32 else np.array_equal(b, want[name]), (gone, name)
    assert mi.mi_knn_sharded_summarize(st._h, labels.ctypes.data, C, *([None] * 10)) == 0
    out = (ctypes.c_uint64 * 4)()
    assert mi.mi_knn_sharded_summarize_stats(st._h, out) == 0 and out[3] == want["totals"]["members"]
    st.close()
