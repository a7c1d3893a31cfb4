"""mi_knn_assign_multi / mi_knn_sharded_assign_multi without a GPU: the bindings, rows_of_labels, and a numpy emulation of
stage 1's threshold rule (assign_multi_kernels.h): per row m slots, slot j the maximum coarse cosine over the columns c
seen so far with c % m == j, t = the minimum over the slots (-inf until all are filled), (row, c) emitted iff
coarse >= t - 2 eps2.  The emulation shows that the exact top m is always inside the emitted set, whatever the order of
the tiles — on the worst-case rows of tests/test_join_bound.py (both operands lose almost 2^-8 to the rounding, all terms
aligned) and on random rows."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import NO_LABEL, EmbeddingTable, ImageIndex, ShardedTable, rows_of_labels
from test_join_bound import DIM, EPS2, bf16_rne, worst_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi_knn_assign_multi", "mi_knn_assign_multi_stats", "mi_knn_sharded_assign_multi"]
MI_ERR_INVALID = -1
TILE = 128


def test_header_bindings_and_library_carry_the_new_symbols(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert _lib.SYMBOLS["mi_knn_assign_multi"][1][3:5] == [ctypes.c_uint32, ctypes.c_float]
    assert mi.mi_abi_version() == 4


def test_python_surface():
    for cls, names in ((EmbeddingTable, ("assign_multi", "assign_multi_stats")), (ShardedTable, ("assign_multi",)),
                       (ImageIndex, ("tags",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    p = inspect.signature(ImageIndex.tags).parameters
    assert p["names"].default is None and p["m"].default == 5 and p["max_dist"].default == float("inf") and p["web"].default is False
    assert inspect.signature(EmbeddingTable.assign_multi).parameters["max_dist"].default == float("inf")


def test_null_handles_are_refused_without_a_device(mi):
    v = np.zeros((2, 768), np.float32)
    lab, d = np.zeros(8, np.uint32), np.zeros(8, np.float32)
    out = (ctypes.c_uint64 * 4)()
    assert mi.mi_knn_assign_multi(None, v.ctypes.data, 2, 2, np.inf, lab.ctypes.data, d.ctypes.data) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert mi.mi_knn_assign_multi_stats(None, out) == MI_ERR_INVALID
    assert mi.mi_knn_sharded_assign_multi(None, v.ctypes.data, 2, 2, np.inf, lab.ctypes.data, d.ctypes.data) == MI_ERR_INVALID


def test_rows_of_labels():
    labels = np.array([[2, 0, NO_LABEL],
                       [NO_LABEL, NO_LABEL, NO_LABEL],
                       [0, 2, 3],
                       [3, NO_LABEL, NO_LABEL],
                       [2, 3, 0]], np.uint32)
    got = rows_of_labels(labels, 5)
    assert [g.tolist() for g in got] == [[0, 2, 4], [], [0, 2, 4], [2, 3, 4], []]
    assert all(g.dtype == np.uint64 for g in got)
    # one label per row, as assign reports them
    assert [g.tolist() for g in rows_of_labels(np.array([1, NO_LABEL, 1, 0], np.uint32), 2)] == [[3], [0, 2]]
    assert [g.tolist() for g in rows_of_labels(np.empty((0, 4), np.uint32), 2)] == [[], []]
    with pytest.raises(ValueError):
        rows_of_labels(np.array([[5]], np.uint32), 5)


def cosines(rows, vec):
    """(coarse, exact) cosines [rows, C]: coarse = the bf16-rounded operands' product over the unrounded norms (stage 1),
    exact = the fp32 rows' (stage 2 decides by it); float64 arithmetic, whose own error is far inside eps2's fp32 terms"""
    norm = np.sqrt(np.sum(rows.astype(np.float64) ** 2, 1))[:, None] * np.sqrt(np.sum(vec.astype(np.float64) ** 2, 1))[None, :]
    coarse = bf16_rne(rows).astype(np.float64) @ bf16_rne(vec).astype(np.float64).T / norm
    exact = rows.astype(np.float64) @ vec.astype(np.float64).T / norm
    return coarse, exact


def emitted(coarse, m, tiles):
    """the kernel's rule, the column tiles visited in the order given: boolean [rows, C]"""
    n, C = coarse.shape
    slots = np.full((n, m), -np.inf)
    out = np.zeros((n, C), bool)
    for bj in tiles:
        cols = np.arange(bj * TILE, min(C, (bj + 1) * TILE))
        for j in range(m):
            mine = cols[cols % m == j]
            if mine.size:
                slots[:, j] = np.maximum(slots[:, j], coarse[:, mine].max(axis=1))
        t = slots.min(axis=1)
        out[:, cols] = coarse[:, cols] >= (t - 2.0 * EPS2)[:, None]
    return out


def hard_corpus(seed):
    """64 rows: 32 at the rounding's worst case, each with its worst-case partner and six bf16-exact vectors around the
    partner's cosine among the columns (the coarse order of those differs from the exact one), and 32 Gaussian rows; 300
    columns = two full tiles and a ragged one"""
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


@pytest.mark.parametrize("m", [1, 3, 16])
def test_threshold_rule_keeps_the_exact_top_m_in_any_tile_order(m):
    rows, vec = hard_corpus(17)
    coarse, exact = cosines(rows, vec)
    assert np.max(np.abs(coarse - exact)) <= EPS2
    assert np.max(np.abs(coarse - exact)[:32]) > 0.5 * 2.0 ** -7      # the worst-case rows do come close to the bound
    # the premise: on the worst-case rows the coarse order is not the exact one (the partner loses 2^-7, the others 2^-8)
    flipped = int(np.sum(np.any(np.sort(np.argsort(-coarse[:32], axis=1)[:, :3]) != np.sort(np.argsort(-exact[:32], axis=1)[:, :3]), axis=1)))
    assert flipped >= 16, flipped
    mth = np.sort(exact, axis=1)[:, -m]                              # the exact m-th best; ties with it belong to the top m
    top = exact >= mth[:, None]
    n_tiles = (vec.shape[0] + TILE - 1) // TILE
    for tiles in (list(range(n_tiles)), list(range(n_tiles))[::-1], [1, 2], [2]):   # two orders, and pieces that see some columns
        got = emitted(coarse, m, tiles)
        seen = np.zeros(vec.shape[0], bool)
        for bj in tiles:
            seen[bj * TILE:(bj + 1) * TILE] = True
        # (a piece owes every member of the overall top m among the columns it sees: those are in its own top m too)
        assert np.all(got[:, seen][top[:, seen]]), (m, tiles)
        assert not np.any(got[:, ~seen])
    # the rule is not vacuous: the Gaussian rows emit a part of the columns only
    full = emitted(coarse, m, list(range(n_tiles)))
    print(f"m {m}: emitted {full[32:].mean():.3f} of all pairs on the Gaussian rows, {full[:32].mean():.3f} on the worst-case rows")
    assert full[32:].mean() < 0.9
