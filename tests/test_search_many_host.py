"""mi_knn_search_many / mi_knn_neighbors / mi_knn_sharded_search_many without a GPU: the bindings, drop_self, and a numpy
emulation of stage 1's two passes (search_many_kernels.h).  Threshold pass: the sampled column tiles (every s-th) are cut
into segments, every segment keeps per query m slots (slot j = the maximum coarse cosine over its columns c with
c % m == j), the segments' slots are folded by maximum; t = the minimum over the folded slots (-inf while one is empty).
Emit pass: (query, c) is emitted iff coarse >= t - 2 eps2, over ALL columns.  The emulation shows that the exact top m is
always inside the emitted set — on the worst-case rows of tests/test_join_bound.py (tests/test_assign_multi_host.py's
hard_corpus construction) — and prints what stage 1 hands over on the GPU test's corpus."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import NO_ID, EmbeddingTable, ImageIndex, ShardedTable, drop_self
from test_join_bound import DIM, EPS2, bf16_rne, worst_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi_knn_search_many", "mi_knn_search_many_stats", "mi_knn_neighbors", "mi_knn_sharded_search_many"]
MI_ERR_INVALID = -1
TILE = 128
INF = np.float32(np.inf)


def test_header_bindings_and_library_carry_the_new_symbols(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert _lib.SYMBOLS["mi_knn_neighbors"][1][1:4] == [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    assert mi.mi_abi_version() == 4


def test_python_surface():
    for cls, names in ((EmbeddingTable, ("knn_many", "neighbors", "search_many_stats")), (ShardedTable, ("knn_many", "neighbors")),
                       (ImageIndex, ("related", "best_per_label"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    for cls in (EmbeddingTable, ShardedTable):
        p = inspect.signature(cls.neighbors).parameters
        assert list(p)[1:] == ["k", "first", "n"] and p["first"].default == 0 and p["n"].default is None
    p = inspect.signature(ImageIndex.related).parameters
    assert p["k"].default == 10 and p["web"].default is False
    p = inspect.signature(ImageIndex.best_per_label).parameters
    assert p["names"].default is None and p["k"].default == 10 and p["web"].default is False


def test_null_handles_are_refused_without_a_device(mi):
    q = np.zeros((2, 768), np.float32)
    idx, d = np.zeros(8, np.uint64), np.zeros(8, np.float32)
    out = (ctypes.c_uint64 * 4)()
    assert mi.mi_knn_search_many(None, q.ctypes.data, 2, 4, idx.ctypes.data, d.ctypes.data) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert mi.mi_knn_search_many_stats(None, out) == MI_ERR_INVALID
    assert mi.mi_knn_neighbors(None, 0, 2, 4, idx.ctypes.data, d.ctypes.data) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_search_many(None, q.ctypes.data, 2, 4, idx.ctypes.data, d.ctypes.data) == MI_ERR_INVALID


def test_drop_self():
    N = NO_ID
    idx = np.array([[4, 0, 9, 2],        # own id (0) in the middle
                    [5, 6, 7, 8],        # own id (1) absent: the last entry goes
                    [N, N, N, N],        # only padding (a zero-norm row, a deleted row)
                    [0, 1, 2, 4],        # row 5 with k + 1 = 4 exact copies at lower ids: the first k of them stay
                    [6, 3, N, N],        # own id (6) first, padding behind the last hit
                    [3, 7, N, N]], np.uint64)   # own id last before the padding
    dist = np.array([[0.1, 0.2, 0.3, 0.4],
                     [0.1, 0.2, 0.3, 0.4],
                     [INF, INF, INF, INF],
                     [0.0, 0.0, 0.0, 0.0],
                     [0.0, 0.5, INF, INF],
                     [0.2, 0.2, INF, INF]], np.float32)
    gi, gd = drop_self(idx, dist, [0, 1, 2, 5, 6, 7])
    assert gi.dtype == np.uint64 and gd.dtype == np.float32 and gi.shape == gd.shape == (6, 3)
    assert gi.tolist() == [[4, 9, 2], [5, 6, 7], [N, N, N], [0, 1, 2], [3, N, N], [3, N, N]]
    assert gd.tolist() == [[np.float32(0.1), np.float32(0.3), np.float32(0.4)], [np.float32(0.1), np.float32(0.2), np.float32(0.3)],
                           [INF, INF, INF], [0.0, 0.0, 0.0], [0.5, INF, INF], [np.float32(0.2), INF, INF]]
    e = drop_self(np.empty((0, 3), np.uint64), np.empty((0, 3), np.float32), [])
    assert e[0].shape == (0, 2) and e[1].shape == (0, 2)


def cosines(rows, vec):
    """(coarse, exact) cosines [rows, C]: coarse = the bf16-rounded operands' product over the unrounded norms (stage 1),
    exact = the fp32 rows' (stage 2 decides by it); float64 arithmetic, whose own error is far inside eps2's fp32 terms"""
    norm = np.sqrt(np.sum(rows.astype(np.float64) ** 2, 1))[:, None] * np.sqrt(np.sum(vec.astype(np.float64) ** 2, 1))[None, :]
    coarse = bf16_rne(rows).astype(np.float64) @ bf16_rne(vec).astype(np.float64).T / norm
    exact = rows.astype(np.float64) @ vec.astype(np.float64).T / norm
    return coarse, exact


def thresholds(coarse, m, segments, stride):
    """the threshold pass: t [queries]"""
    n, C = coarse.shape
    sampled = list(range(0, (C + TILE - 1) // TILE, stride))
    segments = min(segments, len(sampled))
    folded = np.full((n, m), -np.inf)
    for y in range(segments):
        slots = np.full((n, m), -np.inf)   # the workgroup's own
        for bj in sampled[y * len(sampled) // segments:(y + 1) * len(sampled) // segments]:
            cols = np.arange(bj * TILE, min(C, (bj + 1) * TILE))
            for j in range(m):
                mine = cols[cols % m == j]
                if mine.size:
                    slots[:, j] = np.maximum(slots[:, j], coarse[:, mine].max(axis=1))
        folded = np.maximum(folded, slots)
    return folded.min(axis=1)


def emitted(coarse, m, segments, stride):
    """the emit pass over all columns: boolean [queries, C]"""
    return coarse >= (thresholds(coarse, m, segments, stride) - 2.0 * EPS2)[:, None]


def hard_corpus(seed):
    """tests/test_assign_multi_host.py's: 64 queries, 32 at the rounding's worst case, each with its worst-case partner and
    six bf16-exact vectors around the partner's cosine among the columns (the coarse order of those differs from the exact
    one), and 32 Gaussian ones; 300 columns = two full tiles and a ragged one"""
    rng = np.random.default_rng(seed)
    rows, vec = [], []
    for i in range(32):
        x, y = worst_pair(rng, +1)
        rows.append(x)
        vec.append(y)
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        cos_xy = x64 @ y64 / np.sqrt((x64 @ x64) * (y64 @ y64))
        noise = rng.standard_normal(DIM) * np.sqrt(np.mean(x64 ** 2))
        for delta in (-2e-3, -5e-4, 5e-4, 1e-3, 2e-3, 4e-3):   # z: bf16-exact, its exact cosine to x delta below y's
            lo, hi = 0.0, 4.0
            for _ in range(40):
                mid = 0.5 * (lo + hi)
                z = bf16_rne((x64 + mid * noise).astype(np.float32)).astype(np.float64)
                lo, hi = (mid, hi) if x64 @ z / np.sqrt((x64 @ x64) * (z @ z)) > cos_xy - delta else (lo, mid)
            vec.append(z.astype(np.float32))
    rows += list(rng.standard_normal((32, DIM)).astype(np.float32))
    vec += list(rng.standard_normal((300 - len(vec), DIM)).astype(np.float32))
    vec = np.asarray(vec, np.float32)
    return np.asarray(rows, np.float32), vec[rng.permutation(vec.shape[0])]


@pytest.fixture(scope="module")
def hard():
    rows, vec = hard_corpus(17)
    return cosines(rows, vec)


@pytest.mark.parametrize("m", [1, 3, 16])
def test_two_pass_rule_keeps_the_exact_top_m(hard, m):
    coarse, exact = hard
    assert np.max(np.abs(coarse - exact)) <= EPS2
    assert np.max(np.abs(coarse - exact)[:32]) > 0.5 * 2.0 ** -7      # the worst-case rows do come close to the bound
    mth = np.sort(exact, axis=1)[:, -m]                              # the exact m-th best; ties with it belong to the top m
    top = exact >= mth[:, None]
    full = None
    for segments in (1, 2, 5):
        for stride in (1, 2, 8):
            got = emitted(coarse, m, segments, stride)
            assert np.all(got[top]), (m, segments, stride)
            if stride == 1:   # the fold of the segments' slots is the one workgroup's slots
                full = got if full is None else full
                assert np.array_equal(got, full)
            else:             # a sample's thresholds are lower: a superset
                assert np.all(got[full])
    print(f"m {m}: emitted {full[32:].mean():.3f} of all pairs on the Gaussian queries, {full[:32].mean():.3f} on the worst-case ones; "
          f"stride 8: {emitted(coarse, m, 1, 8)[32:].mean():.3f}")
    assert full[32:].mean() < 0.9   # the rule is not vacuous


def test_candidates_on_the_gpu_tests_corpus():
    """what stage 1 hands over on tests/test_search_many_gpu.py's corpus (its cap: an eighth of all pairs)"""
    from test_search_many_gpu import N_QUERIES, N_ROWS, corpus_and_queries
    rows, queries = corpus_and_queries()
    coarse, exact = cosines(queries, rows)
    assert coarse.shape == (N_QUERIES, N_ROWS)
    for k in (4, 16):
        mth = np.sort(exact, axis=1)[:, -k]
        for stride in (1, 8):
            got = emitted(coarse, k, 5, stride)
            assert np.all(got[exact >= mth[:, None]])
            per = got.sum(axis=1)
            print(f"k {k} stride {stride}: {per.mean():.1f} candidates per query ({got.mean():.4f} of all pairs), planted queries "
                  f"{per[:16].mean():.1f}, Gaussian queries {per[16:].mean():.1f}, the largest {per.max()}")
            if stride == 1:   # inside the GPU test's cap (an eighth) with a fifth to spare, for each of its query counts
                for nq in (1, 127, 129, 300):
                    assert got[:nq].mean() < 0.8 / 8, (k, nq, got[:nq].mean())
