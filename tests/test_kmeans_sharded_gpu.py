"""k-means across the shards on the GPU (mi_knn_sharded_kmeans) and the fixed-point sum it rests on (option "kmeans_fixed_sum"):
centroids, labels, dist, iterations, changed count and objective equal, bit for bit, what one EmbeddingTable holding the same rows
returns with the option on — for every shard count and block size — and both equal the numpy restatement of
tests/test_kmeans_sharded_host.py (expected_fixed_update) on a corpus whose norms are exact.  Every shard lives on device 0."""
import numpy as np
import pytest

from image_search_amd._lib import MiError
from image_search_amd.search import EmbeddingTable, ShardedTable
from test_assign_gpu import DIM, N_PLANTED, NO_LABEL, planted_corpus
from test_kmeans_gpu import check_invariants, same_bits
from test_kmeans_sharded_host import expected_fixed_update, fixed_bound

pytestmark = pytest.mark.gpu

LAYOUTS = ((1, 4096), (3, 64), (2, 128), (4, 64), (2, 960))          # (shards, block rows)
ITERS = (0, 1, 4)


def sharded_of(rows, shards, block):
    t = ShardedTable(DIM, [0] * shards, block)
    t.insert(rows)
    return t


def shard_of(rows, shards, block):
    return (np.asarray(rows) // block) % shards


def assert_same_result(got, want, what=""):
    """everything the call's contract names, by bits"""
    assert same_bits(got["centroids"], want["centroids"]), what
    assert np.array_equal(got["labels"], want["labels"]), what
    assert same_bits(got["dist"], want["dist"]), what
    assert (got["iters"], got["changed"]) == (want["iters"], want["changed"]), what
    assert np.float64(got["objective"]).view(np.uint64) == np.float64(want["objective"]).view(np.uint64), what


@pytest.fixture(scope="module")
def gauss(built):
    """the Gaussian corpus of test_kmeans_gpu.py on one table, its k-means from before the option was ever touched, and the
    results with the option on that every layout must equal: {(C, max_iters): result}"""
    rows = np.random.default_rng(21).standard_normal((4096, DIM)).astype(np.float32)
    rows *= np.random.default_rng(22).uniform(0.1, 10.0, (4096, 1)).astype(np.float32)
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    starts = {64: rows[200:264].copy(), 4: rows[:4].copy()}
    float_path = t.kmeans(starts[64], max_iters=4)
    first = {C: t.assign(c0) for C, c0 in starts.items()}
    want = {(C, it): t.kmeans(c0, max_iters=it, fixed_sum=True) for C, c0 in starts.items() for it in ITERS}
    yield rows, t, starts, first, want, float_path
    t.close()


# 1: the one table's bits, for every layout
@pytest.mark.parametrize("shards,block", LAYOUTS)
def test_equals_the_one_table_to_the_bit(gauss, shards, block):
    rows, _, starts, first, want, _ = gauss
    # C = 4: every cluster has several segments of 512 members, and members on every shard
    lab4 = first[4][0]
    for c in range(4):
        members = np.flatnonzero(lab4 == c)
        assert members.size > 512, (c, members.size)
        assert np.unique(shard_of(members, shards, block)).size == shards, (c, shards, block)
    st = sharded_of(rows, shards, block)
    for (C, it), w in want.items():
        got = st.kmeans(starts[C], max_iters=it)
        assert_same_result(got, w, (shards, block, C, it))
        if it == 0:
            assert got["iters"] == 0 and same_bits(got["centroids"], starts[C]) and got["changed"] == rows.shape[0]
    assert want[(64, 4)]["iters"] == 4 and want[(4, 4)]["iters"] == 4
    st.close()


def exact_corpus():
    """1536 rows whose fp32 sum of squares is 4^e exactly in any summation order (so inv = 2^-e and v = x * inv are exact): 256
    entries of +-2^-4 at random places, every other entry k * 2^-40 with |k| < 2048 (v * 2^30 = k / 1024: the ties 0.5, 1.5,
    -0.5, -1.5 among them, and their neighbours), the row times 2^e.  The squares of the small entries, at most 2^-58 each,
    vanish below half an ulp (2^-32 or more) of any partial sum that holds a large one."""
    rng = np.random.default_rng(41)
    n = 1536
    rows = np.zeros((n, DIM), np.float64)
    e = rng.integers(-3, 4, n)
    for r in range(n):
        big = rng.choice(DIM, 256, replace=False)
        small = np.setdiff1d(np.arange(DIM), big)
        k = rng.integers(-2047, 2048, small.size)
        k[:6] = (512, 1536, -512, -1536, 513, 511)
        rows[r, small] = rng.permutation(k) * 2.0 ** -40
        rows[r, big] = rng.choice((-1.0, 1.0), 256) * 2.0 ** -4
        rows[r] *= 2.0 ** e[r]
    rows32 = rows.astype(np.float32)
    assert np.array_equal(rows32.astype(np.float64), rows)
    frac = np.mod(rows / 2.0 ** e[:, None] * 2.0 ** 30, 1.0) != 0
    assert frac.mean() > 0.6
    return rows32, (2.0 ** -e).astype(np.float32)


# 2: the restatement to the bit
def test_equals_the_restatement_on_exact_norms(built):
    rows, inv = exact_corpus()
    C = 8
    c0 = rows[:C].copy()
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    st = sharded_of(rows, 3, 64)
    cs = [c0]
    for i in range(3):
        lab, d = t.assign(cs[i])
        assert not np.isnan(d).any()
        cs.append(expected_fixed_update(rows, inv, lab, d, C, cs[i]))
    assert not same_bits(cs[1], cs[0])
    for i in range(3):
        one = t.kmeans(c0, max_iters=i + 1, fixed_sum=True)
        assert 1 <= one["iters"] <= i + 1 and (one["iters"] == i + 1 or one["changed"] == 0)
        assert same_bits(one["centroids"], cs[one["iters"]]), i
        assert_same_result(st.kmeans(c0, max_iters=i + 1), one, i)
    t.close()
    st.close()


# 3: accuracy without an n_c term
@pytest.mark.parametrize("C", (64, 4))
def test_one_update_against_fp64_means(gauss, C):
    rows, _, _, first, want, _ = gauss
    lab, d = first[C]
    res = want[(C, 1)]
    assert res["iters"] == 1
    unit = rows.astype(np.float64) / np.linalg.norm(rows.astype(np.float64), axis=1, keepdims=True)
    worst = 0.0
    for c in range(C):
        m = (lab == c) & ~np.isnan(d)
        assert m.any()
        mean = unit[m].mean(axis=0)
        err, bound = np.abs(res["centroids"][c].astype(np.float64) - mean), fixed_bound(unit[m], mean)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (c, int(m.sum()), float(np.max(err / bound)))
    print(f"C = {C}: largest error / bound: {worst:.3f}")


# 4: rows that must not count, across shards
@pytest.mark.parametrize("shards,block", ((3, 64), (4, 960)))
def test_deleted_and_nan_rows_across_shards(built, shards, block):
    rng = np.random.default_rng(27)
    rows = rng.standard_normal((2000, DIM)).astype(np.float32)
    rows[50] = 0.0            # NaN distance to everything
    rows[51, 3] = np.inf
    dead = np.arange(100, 400)
    c0 = rows[1000:1008].copy()
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    t.delete(dead)
    st = sharded_of(rows, shards, block)
    st.delete(dead.astype(np.uint64))
    if shards == 4:
        assert st.shard_rows(3) == 0 and st.shard_rows(2) > 0      # an empty shard takes part with zeros
    want = t.kmeans(c0, max_iters=3, fixed_sum=True)
    got = st.kmeans(c0, max_iters=3)
    assert want["iters"] == 3
    assert_same_result(got, want, (shards, block))
    assert np.all(got["labels"][dead] == NO_LABEL) and np.all(np.isnan(got["dist"][[50, 51]]))
    assert np.all(np.isfinite(got["centroids"]))
    check_invariants(st, got)
    t.close()
    st.close()


# 5: a cluster that lives on one shard, and an empty cluster
def test_a_cluster_on_one_shard_and_an_empty_cluster(gauss):
    base = gauss[0].astype(np.float64)
    rng = np.random.default_rng(43)
    d = rng.standard_normal(DIM)
    d /= np.linalg.norm(d)
    rows = base - np.outer(base @ d, d)                        # no row has a component along d ...
    e = -(rows[0] + rows[1])
    e /= np.linalg.norm(e)                                     # (orthogonal to d, as rows 0 and 1 are)
    rows[2:] -= np.outer(rows[2:] @ e, e)                      # ... and only rows 0 and 1 one along e, a negative one
    rows[10:20] += 3.0 * np.linalg.norm(rows[10:20], axis=1, keepdims=True) * d     # ... but ten rows of the first block
    rows = rows.astype(np.float32)
    c0 = rows[200:264].copy()
    c0[7] = d.astype(np.float32)
    c0[9] = -rows[0] - rows[1]
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    lab, _ = t.assign(c0)
    members = np.flatnonzero(lab == 7)
    assert members.size >= 10 and members.max() < 128          # shard 1 of 2 x 128 contributes n = 0 for cluster 7
    assert not np.any(lab == 9)
    want = t.kmeans(c0, max_iters=1, fixed_sum=True)
    st = sharded_of(rows, 2, 128)
    got = st.kmeans(c0, max_iters=1)
    assert got["iters"] == 1
    assert_same_result(got, want)
    assert same_bits(got["centroids"][9], c0[9]) and not same_bits(got["centroids"][7], c0[7])
    t.close()
    st.close()


# 6: calling again, layout independence, and what crossed between the shards
def test_calling_again_layouts_and_stats(gauss):
    rows, _, starts, _, want, _ = gauss
    C, c0 = 64, starts[64]
    a3, a4 = sharded_of(rows, 3, 64), sharded_of(rows, 4, 64)
    first, again, other = a3.kmeans(c0, max_iters=4), a3.kmeans(c0, max_iters=4), a4.kmeans(c0, max_iters=4)
    assert_same_result(again, first)
    assert_same_result(other, first)
    assert_same_result(first, want[(64, 4)])
    for st, S in ((a3, 3), (a4, 4)):
        stats = st.kmeans_stats()
        iters = first["iters"]
        assert stats["updates"] == iters == 4
        assert stats["bytes_exchanged"] == iters * (S - 1) * C * (8 * DIM + 4) + iters * (S - 1) * C * DIM * 4, stats
        assert stats["merge_launches"] == iters * (S - 1), stats
        assert C <= stats["segments"] <= S * C + 4096 // 512, stats
    a3.kmeans(c0, max_iters=0)
    assert a3.kmeans_stats() == {"updates": 0, "bytes_exchanged": 0, "segments": 0, "merge_launches": 0}
    a3.close()
    a4.close()


# 7: the option on the one table
def test_the_option_on_one_table(gauss):
    rows, _, starts, first, want, float_path = gauss
    c0 = starts[64]
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    assert_same_result(t.kmeans(c0, max_iters=4), float_path)
    fixed = t.kmeans(c0, max_iters=4, fixed_sum=True)
    assert_same_result(fixed, want[(64, 4)])
    assert not same_bits(fixed["centroids"], float_path["centroids"])
    assert_same_result(t.kmeans(c0, max_iters=4), float_path)        # the call restored the option
    t.set_option("kmeans_fixed_sum", 1)
    assert_same_result(t.kmeans(c0, max_iters=4), want[(64, 4)])
    assert_same_result(t.kmeans(c0, max_iters=4, fixed_sum=False), float_path)
    assert_same_result(t.kmeans(c0, max_iters=4), want[(64, 4)])
    # summarize returns k-means' centroids under the option too
    lab = first[64][0]
    s = t.summarize(lab, 64)
    one = want[(64, 1)]
    for c in range(64):
        if np.any(lab == c):
            assert same_bits(s["centroids"][c], one["centroids"][c]), c
    with pytest.raises(MiError):
        t.set_option("kmeans_fixed_sum", 2)
    with pytest.raises(MiError):
        t.set_option("kmeans_fixed_sum", -1)
    assert_same_result(t.kmeans(c0, max_iters=4), want[(64, 4)])      # a refused value changed nothing
    t.set_option("kmeans_fixed_sum", 0)
    assert_same_result(t.kmeans(c0, max_iters=4), float_path)
    s0, one0 = t.summarize(lab, 64), t.kmeans(c0, max_iters=1)
    for c in range(64):
        if np.any(lab == c):
            assert same_bits(s0["centroids"][c], one0["centroids"][c]), c
    t.close()


# 8: k rows picked from a seed
def test_seeded_start_on_the_planted_corpus(built):
    rows = planted_corpus()[0][:N_PLANTED]
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    st = sharded_of(rows, 3, 64)
    want = t.kmeans(16, seed=3, fixed_sum=True)
    got = st.kmeans(16, seed=3)
    assert want["iters"] >= 1
    assert_same_result(got, want)
    check_invariants(st, got)
    with pytest.raises(ValueError, match="across shards"):
        st.kmeans(16, init="kmeans++")
    t.close()
    st.close()
