"""mi_knn_representatives without a GPU: the numpy restatement of the contract in include/mi355clip.h (farthest-first picks of
every group, on distance keys), hand-made cases for each of its rules, one planted case that shows what the call is for, and
the bindings.  tests/test_representatives_gpu.py holds the device to this restatement bit for bit."""
import ctypes
import os

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import EmbeddingTable, ImageIndex, typical_order
from test_kmeans_seed_host import oracle_dist_from
from test_page_host import INF, bits, dist_key, key_dist
from test_summary_host import MI_ERR_INVALID, MI_ERR_UNSUPPORTED, NO_LABEL

NEW = ["mi_knn_representatives", "mi_knn_representatives_stats", "mi_index_folder_highlights"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.float32(np.nan)
NAN_KEY = np.uint32(0xFFFFFFFF)
NO_ROW = -1


# ---- the restatement ------------------------------------------------------------------------------------------------

def restate_representatives(dist_from, labels, member, C, m, min_gap, start=None):
    """dist_from(p) [rows]: d(p, .), the distances the search reports with q = row p; labels [rows]; member [rows] bool (live,
    usable; the label is judged here); start: None or [C] local rows.  -> dict(rows [C, m] local rows (NO_ROW = none), gap,
    n_picked, reach, rep, rep_dist), or ValueError for a start that is no member of its non-empty group."""
    labels = np.asarray(labels).astype(np.uint32)
    n = labels.size
    member = np.asarray(member, bool) & (labels < C)
    gap_key = dist_key(np.float32(min_gap))
    bounded = not np.isneginf(min_gap)
    rows = np.full((C, m), NO_ROW, np.int64)
    gap = np.full((C, m), INF, np.float32)
    n_picked, reach = np.zeros(C, np.uint32), np.full(C, INF, np.float32)
    rep, K = np.full(n, NO_LABEL, np.uint32), np.full(n, NAN_KEY, np.uint32)
    for c in range(C):
        mem = np.flatnonzero(member & (labels == c))
        if mem.size == 0:
            continue
        if start is not None and int(start[c]) not in mem.tolist():
            raise ValueError(f"start[{c}] is no member")
    for c in range(C):
        mem = np.flatnonzero(member & (labels == c))          # ascending by row = ascending by id
        if mem.size == 0:
            continue
        picked = np.zeros(mem.size, bool)
        p = int(start[c]) if start is not None else int(mem[0])
        for j in range(m):
            rows[c, j] = p
            picked[mem == p] = True
            n_picked[c] = j + 1
            key = dist_key(dist_from(p)[mem])
            lower = key < K[mem]                              # strict: rep keeps the lowest pick that attains K
            K[mem[lower]] = key[lower]
            rep[mem[lower]] = j
            if j + 1 == m:
                break
            cand = ~picked & (K[mem] != NAN_KEY)
            if not cand.any():
                break
            best = K[mem][cand].max()
            if bounded and not best > gap_key:
                break
            p = int(mem[cand & (K[mem] == best)][0])          # the lowest id among equal keys
            gap[c, j + 1] = key_dist(best)
        number = K[mem] != NAN_KEY
        if number.any():
            reach[c] = key_dist(K[mem][number].max())
    rep_dist = np.full(n, INF, np.float32)
    rep_dist[member] = key_dist(K[member])
    rep_dist[member & (K == NAN_KEY)] = NAN
    return {"rows": rows, "gap": gap, "n_picked": n_picked, "reach": reach, "rep": rep, "rep_dist": rep_dist}


def table_of(D):
    """dist_from over a hand-made matrix D [n, n]: D[p, r] = d(p, r)"""
    D = np.asarray(D, np.float32)
    return lambda p: D[p]


def line(points):
    """|x_p - x_r| for points on a line: a metric to think in"""
    x = np.asarray(points, np.float32)
    return np.abs(x[:, None] - x[None, :]).astype(np.float32)


def run(D, labels, C, m, min_gap=-np.inf, start=None, member=None):
    labels = np.asarray(labels, np.uint32)
    member = np.ones(labels.size, bool) if member is None else member
    return restate_representatives(table_of(D), labels, member, C, m, np.float32(min_gap), start)


# ---- hand-written cases ------------------------------------------------------------------------------------------------

def test_farthest_first_on_a_line_and_the_tie_goes_to_the_lowest_id():
    #          0    1    2    3    4
    D = line([0.0, 1.0, 5.0, 9.0, 10.0])
    r = run(D, np.zeros(5), 1, 5)
    assert r["rows"][0].tolist() == [0, 4, 2, 1, 3]           # 10; 5 (|5-0| = |5-10|); then 1 and 3 tie at 1: the lower id
    assert r["gap"][0].tolist() == [np.inf, 10.0, 5.0, 1.0, 1.0]
    assert r["rep"].tolist() == [0, 3, 2, 4, 1] and not np.any(r["rep_dist"]) and r["reach"][0] == 0.0
    r = run(D, np.zeros(5), 1, 3)
    assert r["rows"][0].tolist() == [0, 4, 2] and r["rep"].tolist() == [0, 0, 2, 1, 1]
    assert r["rep_dist"].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0] and r["reach"][0] == 1.0 and r["n_picked"][0] == 3
    # equal keys for pick 1: rows 1 and 3 are both 4 away from the start
    r = run(line([4.0, 0.0, 4.5, 8.0]), np.zeros(4), 1, 2, start=[0])
    assert r["rows"][0].tolist() == [0, 1] and r["gap"][0, 1] == 4.0
    assert r["rep"].tolist() == [0, 1, 0, 0]                  # row 3 is 4 from pick 0 and 8 from pick 1


def test_exact_copies_are_picked_by_id_without_a_bound_and_once_with_min_gap_zero():
    D = np.zeros((6, 6), np.float32)
    r = run(D, np.zeros(6), 1, 4)
    assert r["rows"][0].tolist() == [0, 1, 2, 3] and r["gap"][0].tolist() == [np.inf, 0.0, 0.0, 0.0] and r["n_picked"][0] == 4
    assert r["rep"].tolist() == [0] * 6                       # pick 0 attains every K first
    r = run(D, np.zeros(6), 1, 4, min_gap=0.0)
    assert r["rows"][0].tolist() == [0, NO_ROW, NO_ROW, NO_ROW] and r["n_picked"][0] == 1 and np.all(np.isposinf(r["gap"][0]))
    assert r["reach"][0] == 0.0 and r["rep"].tolist() == [0] * 6


def test_min_gap_on_a_picks_key_and_one_ulp_below():
    D = line([0.0, 1.0, 5.0, 9.0, 10.0])
    five = np.float32(5.0)
    r = run(D, np.zeros(5), 1, 5, min_gap=five)               # a pick is made only ABOVE the bound
    assert r["rows"][0].tolist() == [0, 4, NO_ROW, NO_ROW, NO_ROW] and r["n_picked"][0] == 2 and r["reach"][0] == 5.0
    r = run(D, np.zeros(5), 1, 5, min_gap=np.nextafter(five, np.float32(0.0)))
    assert r["rows"][0].tolist() == [0, 4, 2, NO_ROW, NO_ROW] and r["gap"][0, 2] == 5.0 and r["reach"][0] == 1.0


def test_minus_zero_comes_before_plus_zero():
    # from pick 0: row 1 at -0, row 2 at +0.  +0 is the larger key: row 2 is pick 1, and min_gap = -0 lets it through
    D = np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, -0.0]], np.float32)
    D[0, 0] = -0.0
    r = run(D, np.zeros(3), 1, 2)
    assert r["rows"][0].tolist() == [0, 2] and bits(r["gap"][0, 1]) == bits(np.float32(0.0))
    assert run(D, np.zeros(3), 1, 2, min_gap=-0.0)["n_picked"][0] == 2
    assert run(D, np.zeros(3), 1, 2, min_gap=0.0)["n_picked"][0] == 1
    assert bits(r["reach"][0]) == bits(np.float32(-0.0))      # after pick 1 every K is -0


def test_a_member_with_only_nan_distances_is_never_picked():
    D = line([0.0, 1.0, 2.0, 7.0])
    D[:, 2] = NAN                                             # nobody measures row 2 ...
    D[2, :] = NAN                                             # ... and it measures nobody
    r = run(D, np.zeros(4), 1, 4)
    assert r["rows"][0].tolist() == [0, 3, 1, NO_ROW] and r["n_picked"][0] == 3
    assert r["rep"][2] == NO_LABEL and np.isnan(r["rep_dist"][2]) and r["reach"][0] == 0.0
    # a group of nothing else: pick 0 alone, and no reach
    r = run(np.full((2, 2), NAN), np.zeros(2), 1, 3)
    assert r["rows"][0].tolist() == [0, NO_ROW, NO_ROW] and np.isposinf(r["reach"][0]) and np.all(np.isnan(r["rep_dist"]))


def test_a_singleton_an_empty_group_rows_outside_and_m_larger_than_the_group():
    D = line([0.0, 3.0, 4.0, 9.0, 1.0])
    labels = np.array([0, 2, 2, NO_LABEL, 7], np.uint32)       # group 1 is empty; 7 >= C belongs to nothing
    member = np.array([True, True, True, True, True])
    r = restate_representatives(table_of(D), labels, member, 3, 4, np.float32(-np.inf))
    assert r["rows"].tolist() == [[0, NO_ROW, NO_ROW, NO_ROW], [NO_ROW] * 4, [1, 2, NO_ROW, NO_ROW]]
    assert r["n_picked"].tolist() == [1, 0, 2] and np.isposinf(r["reach"][1]) and r["reach"][0] == 0.0
    assert r["gap"][2].tolist() == [np.inf, 1.0, np.inf, np.inf]
    assert r["rep"].tolist() == [0, 0, 1, NO_LABEL, NO_LABEL] and np.all(np.isposinf(r["rep_dist"][3:]))
    # a row that is no member (deleted, unusable) is never picked and stands behind nothing
    member[2] = False
    r = restate_representatives(table_of(D), labels, member, 3, 4, np.float32(-np.inf))
    assert r["rows"][2].tolist() == [1, NO_ROW, NO_ROW, NO_ROW] and r["rep"][2] == NO_LABEL and np.isposinf(r["rep_dist"][2])


def test_a_start_that_is_no_member_is_refused_and_an_empty_groups_entry_is_not_looked_at():
    D = line([0.0, 3.0, 4.0, 9.0])
    labels = np.array([0, 0, 2, 2], np.uint32)
    assert run(D, labels, 3, 2, start=[1, 99, 3])["rows"].tolist() == [[1, 0], [NO_ROW, NO_ROW], [3, 2]]
    with pytest.raises(ValueError):
        run(D, labels, 3, 2, start=[2, 0, 3])                 # row 2 belongs to group 2
    with pytest.raises(ValueError):
        run(D, labels, 3, 2, start=[0, 0, 3], member=np.array([True, True, True, False]))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gaps_never_rise_and_every_member_lies_within_reach(seed):
    rng = np.random.default_rng(seed)
    n, C, m = 120, 4, 12
    x = rng.standard_normal((n, 8)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    D = (1.0 - x @ x.T).astype(np.float32)                    # (not symmetric to the bit in general; here it is)
    labels = rng.integers(0, C + 1, n).astype(np.uint32)
    for min_gap in (-np.inf, 0.5):
        r = run(D, labels, C, m, min_gap=min_gap)
        for c in range(C):
            k = int(r["n_picked"][c])
            keys = dist_key(r["gap"][c, 1:k])
            assert np.all(keys[:-1] >= keys[1:]), (c, r["gap"][c])
            mem = np.flatnonzero(labels == c)
            assert np.all(dist_key(r["rep_dist"][mem]) <= dist_key(r["reach"][c]))
            assert np.all(r["rep"][mem] < k) and sorted(set(r["rows"][c, :k].tolist())) == sorted(r["rows"][c, :k].tolist())
            if k < m and k < mem.size:                        # stopped by the bound: nothing left lies beyond it
                assert r["reach"][c] <= np.float32(min_gap)
            for j in range(k):                                # a pick stands for itself
                assert r["rep_dist"][r["rows"][c, j]] <= r["reach"][c]


# ---- the point of the call: a folder that is 90 % beach --------------------------------------------------------------------

def planted_folder(noise=0.02, n=200, dim=256):
    rng = np.random.default_rng(5)
    centres = np.linalg.qr(rng.standard_normal((dim, 4)))[0].T.astype(np.float32)      # four orthogonal directions
    sizes = [n * 90 // 100, n * 5 // 100, n * 3 // 100, n * 2 // 100]
    sub = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)])
    sub = sub[rng.permutation(n)]
    rows = centres[sub] + noise * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)
    return rows.astype(np.float32), sub


def test_four_picks_hit_all_four_sub_clusters_where_the_nearest_of_the_centroid_are_all_beach(orc):
    rows, sub = planted_folder()
    n = rows.shape[0]
    dist_from, usable = oracle_dist_from(orc, rows)
    assert usable.all()
    # what the data promises: the gap between sub-clusters exceeds twice the radius within one
    D = np.stack([dist_from(p) for p in range(n)])
    same = sub[:, None] == sub[None, :]
    within, between = float(D[same].max()), float(D[~same].min())
    assert between > 2.0 * within, (within, between)
    labels = np.zeros(n, np.uint32)
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    to_centroid = (1.0 - unit @ unit.mean(axis=0) / np.linalg.norm(unit.mean(axis=0))).astype(np.float32)
    nearest = typical_order(labels, to_centroid, 1)[0][:4]
    assert sub[nearest].tolist() == [0, 0, 0, 0]               # typical_order: four pictures of the beach
    cover = int(nearest[0])
    for start in (None, [cover]):
        r = restate_representatives(dist_from, labels, usable, 1, 4, np.float32(-np.inf), start)
        assert sorted(sub[r["rows"][0]].tolist()) == [0, 1, 2, 3], r["rows"]
        assert r["reach"][0] <= np.float32(within) and np.all(r["gap"][0, 1:] >= np.float32(between))
        assert np.array_equal(sub[r["rows"][0][r["rep"]]], sub)            # every row stands behind a pick of its own kind
        stands_for = np.bincount(r["rep"], minlength=4)
        assert sorted(stands_for.tolist()) == sorted(np.bincount(sub).tolist())
    # a fifth pick would fall inside a sub-cluster: min_gap = the radius within stops after four
    r = restate_representatives(dist_from, labels, usable, 1, 9, np.float32(within), [cover])
    assert r["n_picked"][0] == 4


# ---- the bindings -----------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_the_abi_version_stays(mi):
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(mi, name), name
    assert mi.mi_abi_version() == 4
    assert len(_lib.SYMBOLS["mi_knn_representatives"][1]) == 13 and len(_lib.SYMBOLS["mi_index_folder_highlights"][1]) == 8
    for cls, names in ((EmbeddingTable, ("representatives", "representatives_of", "representatives_stats")),
                       (ImageIndex, ("folder_highlights", "highlights"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    build = open(os.path.join(ROOT, "image_search_amd", "build.py")).read()
    assert '"representatives.hip"' in build
    for text in ("gap[c][1] >= gap[c][2]", "K_r > key(min_gap)", "MI_KNN_NO_LABEL and NaN"):
        assert text in header, text


def test_argument_errors_return_codes_without_a_device_and_write_nothing(mi):
    C, m = 3, 4
    picks, gap = np.full(C * m, 7, np.uint64), np.full(C * m, -7.0, np.float32)
    n_picked, reach = np.full(C, 7, np.uint32), np.full(C, -7.0, np.float32)
    rep, rep_dist, totals = np.full(16, 7, np.uint32), np.full(16, -7.0, np.float32), np.full(4, 7, np.uint64)
    labels = np.zeros(16, np.uint32)

    def call(h, c, mm, min_gap=float("-inf")):
        return mi.mi_knn_representatives(h, labels.ctypes.data, c, mm, min_gap, None, picks.ctypes.data, gap.ctypes.data,
                                         n_picked.ctypes.data, reach.ctypes.data, rep.ctypes.data, rep_dist.ctypes.data, totals.ctypes.data)

    fake = ctypes.c_void_p(16)          # a handle that is never followed: every case below is refused in front of it
    assert call(None, C, m) == MI_ERR_INVALID
    assert b"null" in mi.mi_last_error()
    assert call(fake, 0, m) == MI_ERR_INVALID
    assert b"C must be" in mi.mi_last_error()
    assert call(fake, C, 0) == MI_ERR_INVALID
    assert b"m must be" in mi.mi_last_error()
    assert call(fake, C, m, float("nan")) == MI_ERR_INVALID
    assert b"NaN" in mi.mi_last_error()
    assert call(fake, 65537, 1) == MI_ERR_UNSUPPORTED
    assert call(fake, 1, 4097) == MI_ERR_UNSUPPORTED
    assert call(fake, 4096, 1025) == MI_ERR_UNSUPPORTED        # C * m = 2^22 + 4096
    assert b"2^22" in mi.mi_last_error()
    assert call(fake, 0xFFFFFFFF, 0xFFFFFFFF) == MI_ERR_UNSUPPORTED
    assert mi.mi_knn_representatives_stats(None, (ctypes.c_uint64 * 4)()) == MI_ERR_INVALID
    assert mi.mi_knn_representatives_stats(fake, None) == MI_ERR_INVALID
    n = ctypes.c_uint32(7)
    assert mi.mi_index_folder_highlights(None, C, m, float("-inf"), picks.ctypes.data, gap.ctypes.data, n_picked.ctypes.data,
                                         ctypes.byref(n)) == MI_ERR_INVALID
    assert mi.mi_index_folder_highlights(fake, C, m, float("-inf"), picks.ctypes.data, gap.ctypes.data, n_picked.ctypes.data,
                                         None) == MI_ERR_INVALID
    assert np.all(picks == 7) and np.all(gap == -7.0) and np.all(n_picked == 7) and np.all(reach == -7.0)
    assert np.all(rep == 7) and np.all(rep_dist == -7.0) and np.all(totals == 7) and n.value == 7


def test_host_helpers_under_the_sanitizers(tmp_path):
    """tests/cpp/test_representatives_host.cpp: a stand-alone program over csrc/representatives_host.h — the argument rules,
    the candidate word, the min_gap window, the start translation and the decoding of the per-group arrays — built with the
    address and undefined-behaviour sanitizers; it needs neither the library nor a GPU"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "test_representatives_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_representatives_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
