"""mi_knn_kmeans on the GPU: spherical Lloyd's iterations on top of mi_knn_assign, deterministic to the bit."""
import numpy as np
import pytest

from image_search_amd.search import EmbeddingTable, ImageIndex
from test_assign_gpu import DIM, N_CLUSTERS, N_PLANTED, NO_LABEL, planted_corpus

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_invariants(t, res):
    """3: labels / dist == assign(returned centroids) to the bit; objective = the float64 sum of dist over non-NaN live rows"""
    lab, d = t.assign(res["centroids"])
    assert np.array_equal(lab, res["labels"]) and same_bits(d, res["dist"])
    ok = (lab != NO_LABEL) & ~np.isnan(d)
    want = float(np.sum(d[ok].astype(np.float64)))
    assert abs(res["objective"] - want) <= 1e-9 * max(abs(want), 1e-300), (res["objective"], want)


@pytest.fixture(scope="module")
def gauss(built):
    rows = np.random.default_rng(21).standard_normal((4096, DIM)).astype(np.float32)
    rows *= np.random.default_rng(22).uniform(0.1, 10.0, (4096, 1)).astype(np.float32)
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    yield rows, t
    t.close()


# 1: max_iters = 0 is one assign, the centroids untouched
def test_zero_iterations_is_one_assign(gauss):
    rows, t = gauss
    c0 = rows[:64].copy()
    res = t.kmeans(c0, max_iters=0)
    assert same_bits(res["centroids"], c0) and res["iters"] == 0 and res["changed"] == rows.shape[0]
    check_invariants(t, res)


# 2: one update against the fp64 means of x / |x| grouped by assign(initial)
def test_one_update_against_fp64_means(gauss):
    rows, t = gauss
    c0 = rows[100:164].copy()
    c0[5] = -rows[0] - rows[1]   # (far from everything: most likely an empty cluster)
    lab, d = t.assign(c0)
    res = t.kmeans(c0, max_iters=1)
    assert res["iters"] == 1
    unit = rows.astype(np.float64) / np.linalg.norm(rows.astype(np.float64), axis=1, keepdims=True)
    worst = 0.0
    for c in range(64):
        m = (lab == c) & ~np.isnan(d)
        n_c = int(m.sum())
        if n_c == 0:
            assert same_bits(res["centroids"][c], c0[c])
            continue
        want = unit[m].mean(axis=0)
        # gamma_n of an fp32 sum of n_c terms in any order, x 4 for the normalisation's roundings and the division
        bound = 4.0 * (n_c + 8) * 2.0 ** -24 * np.abs(unit[m]).mean(axis=0)
        err = np.abs(res["centroids"][c].astype(np.float64) - want)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (c, n_c, float(np.max(err / bound)))
    print(f"largest error / bound: {worst:.3f}")
    check_invariants(t, res)


# 4: planted clusters
def test_planted_clusters_are_found(built):
    rows, vectors, own = planted_corpus()
    rows = rows[:N_PLANTED]
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    res = t.kmeans(rows[:N_CLUSTERS].copy(), max_iters=20)   # row i < 16 is a member of cluster i
    print("planted:", res["iters"], res["changed"], res["objective"])
    assert res["changed"] == 0 and res["iters"] < 20
    assert np.array_equal(res["labels"], own.astype(np.uint32))
    check_invariants(t, res)
    t.close()


# 5: determinism
def test_deterministic_across_calls_and_handles(gauss):
    rows, t = gauss
    c0 = rows[200:264].copy()
    a = t.kmeans(c0, max_iters=4)
    b = t.kmeans(c0, max_iters=4)
    t2 = EmbeddingTable(DIM, 0)
    t2.insert(rows)
    c = t2.kmeans(c0, max_iters=4)
    t2.close()
    for other in (b, c):
        assert same_bits(a["centroids"], other["centroids"]) and np.array_equal(a["labels"], other["labels"])
        assert same_bits(a["dist"], other["dist"])
        assert (a["iters"], a["changed"]) == (other["iters"], other["changed"])
        assert np.float64(a["objective"]).view(np.uint64) == np.float64(other["objective"]).view(np.uint64)
    check_invariants(t, a)


# 6: the objective does not rise
def test_objective_is_monotone(gauss):
    rows, t = gauss
    c0 = rows[300:364].copy()
    obj = [t.kmeans(c0, max_iters=i)["objective"] for i in range(6)]
    print("objective:", obj)
    for i in range(5):
        assert obj[i + 1] <= obj[i] + rows.shape[0] * 1e-6, (i, obj)
    assert obj[5] < obj[0]


# 7: deleted rows and NaN-distance rows feed no centroid and no objective
def test_deleted_and_nan_rows_contribute_nothing(built):
    rng = np.random.default_rng(27)
    rows = rng.standard_normal((2000, DIM)).astype(np.float32)
    rows[50] = 0.0            # NaN distance to everything
    rows[51, 3] = np.inf
    dead = np.arange(100, 400)
    c0 = rows[1000:1008].copy()
    t = EmbeddingTable(DIM, 0)
    t.insert(rows)
    t.delete(dead)
    keep = np.ones(2000, bool)
    keep[dead] = False
    keep[[50, 51]] = False
    t2 = EmbeddingTable(DIM, 0)    # the same rows without the ones that must not count, in the same order
    t2.insert(rows[keep])
    a, b = t.kmeans(c0, max_iters=3), t2.kmeans(c0, max_iters=3)
    assert same_bits(a["centroids"], b["centroids"])
    assert np.array_equal(a["labels"][keep], b["labels"]) and same_bits(a["dist"][keep], b["dist"])
    assert np.all(a["labels"][dead] == NO_LABEL) and np.all(np.isnan(a["dist"][[50, 51]]))
    assert a["objective"] == b["objective"]
    check_invariants(t, a)
    t.close()
    t2.close()


def test_image_index_label_and_clusters(built):
    rng = np.random.default_rng(28)
    themes = rng.standard_normal((3, DIM)).astype(np.float32)
    sizes = (7, 4, 2)
    emb, paths, theme_of = [], [], {}
    for c, n in enumerate(sizes):
        for i in range(n):
            p = f"/media/{'trip' if i % 2 else 'home'}/t{c}_{i}.jpg"
            paths.append(p)
            theme_of[p] = c
            emb.append(themes[c] + 0.2 * rng.standard_normal(DIM))
    ix = ImageIndex(DIM, 0, "/media")
    ix.insert(paths, np.asarray(emb, np.float32))
    gone = "/media/trip/t0_1.jpg"
    ix.remove([gone])
    tags = ix.label(themes, names=["dog", "receipt", "beach"])
    assert gone not in tags and set(tags) == set(paths) - {gone}
    for p, (name, dist) in tags.items():
        assert name == ["dog", "receipt", "beach"][theme_of[p]] and 0.0 <= dist < 0.2
    assert ix.label(themes)[paths[0]][0] == 0
    web = ix.label(themes, web=True)
    assert all(p.startswith("media/") for p in web) and len(web) == len(tags)
    for seed in range(3):
        groups = ix.clusters(3, seed=seed)
        assert sorted(p for g in groups for p in g) == sorted(set(paths) - {gone})
        assert [len(g) for g in groups] == sorted((len(g) for g in groups), reverse=True)
    ix.close()
