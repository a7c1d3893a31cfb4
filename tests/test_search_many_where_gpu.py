"""mi_knn_search_many_where / mi_knn_neighbors_where / mi_knn_sharded_search_many_where / mi_knn_propose_groups on the GPU.
The narrowed many-query search is held against a loop of mi_knn_search_where (NaN entries stripped) and against the oracle
(orc_cosine_dist, the search's order); the vote against tests/test_search_many_where_host.py's numpy restatement over oracle
distances.  Ids are compared for equality and distances on their bits: there is no tolerance anywhere in this file.

The corpus: dim 768, 1 157 rows = 9 full column tiles + a ragged 5 and 18 bitmap words + a ragged 5 bits; planted clusters
and Gaussian rows, shuffled as tests/test_search_many_gpu.py's corpus_and_queries (and for its reason); 40 rows deleted; one
live row of zeros; tags, stamps and groups on every row."""
import ctypes

import numpy as np
import pytest

from image_search_amd import _lib
from image_search_amd.search import NO_GROUP, EmbeddingTable, ImageIndex, ShardedTable, drop_self, make_where
from test_search_many_gpu import NO_ID, dist_keys, oracle_many, oracle_matrix, same, strip_nan
from test_search_many_where_host import propose

pytestmark = pytest.mark.gpu

DIM = 768
N_ROWS, N_QUERIES, N_CLUSTERS = 1157, 129, 16
MI_ERR_INVALID, MI_ERR_UNSUPPORTED = -1, -5
ZERO_ROW = 77
HIDDEN, FAVOURITE, FEW, SIXTEENTH, NOBODY = 1 << 0, 1 << 1, 1 << 41, 1 << 42, 1 << 40
N_GROUPS = 5

# the predicates (make_where's keywords) and the rows they keep among the live ones
PREDICATES = {
    "all": dict(stamp=(None, None)),
    "tags+stamp": dict(all_of=FAVOURITE, none_of=HIDDEN, stamp=(150, 820)),
    "group": dict(group=3),
    "never": dict(stamp=(5, 4)),
    "nobody": dict(all_of=NOBODY),
    "few": dict(all_of=FEW),
    "sixteenth": dict(all_of=SIXTEENTH),
}


class Corpus:
    def __init__(self, orc):
        rng = np.random.default_rng(31)
        centres = rng.standard_normal((N_CLUSTERS, DIM)).astype(np.float32)
        n_planted = 1024
        own = np.arange(n_planted) % N_CLUSTERS
        planted = (centres[own] + rng.uniform(0.1, 1.5, n_planted)[:, None] * rng.standard_normal((n_planted, DIM))) * \
            rng.uniform(0.1, 10.0, n_planted)[:, None]
        rows = np.concatenate([planted.astype(np.float32), rng.standard_normal((N_ROWS - n_planted, DIM)).astype(np.float32)])
        rows = rows[rng.permutation(N_ROWS)]
        rows[ZERO_ROW] = 0.0
        self.rows = rows
        self.queries = np.concatenate([centres, rng.standard_normal((N_QUERIES - N_CLUSTERS, DIM)).astype(np.float32)])
        r = np.arange(N_ROWS)
        self.dead = np.sort(np.append(rng.permutation(np.setdiff1d(r, [ZERO_ROW, 0, 16, 131, 200]))[:39], 131))
        self.live = np.ones(N_ROWS, bool)
        self.live[self.dead] = False
        tags = np.where(rng.random(N_ROWS) < 0.1, HIDDEN, 0) | np.where(rng.random(N_ROWS) < 0.5, FAVOURITE, 0)
        tags = tags | np.where(r % 16 == 0, SIXTEENTH, 0) | np.where(np.isin(r, [3, 130, 500, 901, 1156]), FEW, 0)
        self.tags = tags.astype(np.uint64)
        self.stamps = rng.integers(0, 1000, N_ROWS).astype(np.int64)
        groups = rng.integers(0, N_GROUPS, N_ROWS).astype(np.uint32)
        groups[rng.random(N_ROWS) < 0.35] = NO_GROUP
        groups[ZERO_ROW] = NO_GROUP
        self.groups = groups
        self.D = oracle_matrix(orc, self.queries, rows)   # [queries, rows]
        self.S = oracle_matrix(orc, rows, rows)           # [rows, rows]: row r as the query

    def keeps(self, name):
        """the rows a predicate keeps: live and qualifying"""
        p = PREDICATES[name]
        t, s = self.tags, self.stamps
        ok = self.live.copy()
        ok &= (t & np.uint64(p.get("all_of", 0))) == np.uint64(p.get("all_of", 0))
        ok &= (t & np.uint64(p.get("none_of", 0))) == 0
        lo, hi = p.get("stamp", (None, None))
        ok &= (s >= (-(1 << 63) if lo is None else lo)) & (s <= ((1 << 63) - 1 if hi is None else hi))
        if "group" in p:
            ok &= self.groups == np.uint32(p["group"])
        return ok

    def fill(self, t):
        t.insert(self.rows)
        t.delete(self.dead)
        t.set_attrs(np.arange(N_ROWS), self.tags, self.stamps)
        t.set_groups(self.groups)
        return t


@pytest.fixture(scope="module")
def corpus(built, orc):
    return Corpus(orc)


@pytest.fixture(scope="module")
def table(corpus):
    t = corpus.fill(EmbeddingTable(DIM, 0))
    yield t
    t.close()


def where_loop(t, queries, k, pred):
    """a loop of mi_knn_search_where, NaN entries stripped"""
    out = [t.knn_where(queries[q0:q0 + 16], k, **pred) for q0 in range(0, queries.shape[0], 16)]
    idx, dist = strip_nan(np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]))
    return (idx, dist), out[0][2]


def test_the_corpus_is_what_the_cases_need(corpus):
    n = {name: int(corpus.keeps(name).sum()) for name in PREDICATES}
    print(n)
    assert n["all"] == N_ROWS - 40 and 0.2 * N_ROWS < n["tags+stamp"] < 0.4 * N_ROWS and n["group"] > 100
    assert n["never"] == n["nobody"] == 0 and 1 <= n["few"] < 16 and 60 <= n["sixteenth"] <= 73
    assert np.all(np.isnan(corpus.S[ZERO_ROW])) and corpus.live[ZERO_ROW]


# 1: the narrowed search against the loop of single searches and against the oracle
# (the one-residue mask is the case of m = 16)
@pytest.mark.parametrize("nq,k,pred", [(nq, k, pred) for pred in PREDICATES for k in (1, 16) for nq in (1, 129)
                                       if pred != "sixteenth" or k == 16])
def test_equals_a_loop_of_search_where(corpus, table, nq, k, pred):
    keep = corpus.keeps(pred)
    got = table.knn_many_where(corpus.queries[:nq], k, **PREDICATES[pred])
    st = table.search_many_stats()
    want, matched = where_loop(table, corpus.queries[:nq], k, PREDICATES[pred])
    print(f"{pred} nq {nq} k {k}: matched {got[2]}, stats {st}")
    same(got[:2], want, f"{pred} nq {nq} k {k} against search_where")
    same(got[:2], oracle_many(corpus.D[:nq], k, keep), f"{pred} nq {nq} k {k} against the oracle")
    assert got[2] == matched == int(keep.sum())
    assert st["hits"] == int(np.sum(want[0] != NO_ID)) == nq * min(k, int((keep & ~np.isnan(corpus.D[0])).sum()))
    if got[2] == 0:
        assert st["launches"] == 0 and st["tiles"] == 0 and np.all(got[0] == NO_ID) and np.all(np.isposinf(got[1]))
    else:
        assert st["launches"] >= 1 and st["hits"] <= st["candidates"] <= nq * got[2]


def test_without_a_predicate_it_is_search_many(corpus, table):
    mi = _lib.lib()
    q = corpus.queries
    for k in (1, 16):
        want = table.knn_many(q, k)
        st_want = table.search_many_stats()
        idx, dist = np.empty((N_QUERIES, k), np.uint64), np.empty((N_QUERIES, k), np.float32)
        matched = ctypes.c_uint64()
        assert mi.mi_knn_search_many_where(table._h, q.ctypes.data, N_QUERIES, k, None, idx.ctypes.data, dist.ctypes.data,
                                           ctypes.byref(matched)) == 0
        same((idx, dist), want, f"w = NULL, k {k}")
        assert table.search_many_stats() == st_want and matched.value == N_ROWS - 40
        same(table.knn_many_where(q, k)[:2], want, "no keywords")
        # ... and the all-pass predicate gives the same answers through the mask
        same(table.knn_many_where(q, k, **PREDICATES["all"])[:2], want, "all-pass")
    want = table.neighbors(5, 100, 60)
    st_want = table.search_many_stats()
    same(table.neighbors_where(5, 100, 60), want, "neighbors, no keywords")
    assert table.search_many_stats() == st_want


# 2: segments, the sampled threshold pass and a buffer at its floor change nothing under a mask
def test_options_give_identical_results_under_a_mask(corpus):
    t = corpus.fill(EmbeddingTable(DIM, 0))
    q, pred, k = corpus.queries, PREDICATES["tags+stamp"], 16
    want = oracle_many(corpus.D, k, corpus.keeps("tags+stamp"))
    for cap in (0, 1 << 14):
        if cap:
            t.set_option("join_cap", cap)   # the floor: 16 384 pairs < 129 queries x the rows kept
        for segments in (1, 2, 1000):
            for sample in (1, 8):
                t.set_option("many_segments", segments)
                t.set_option("many_sample", sample)
                same(t.knn_many_where(q, k, **pred)[:2], want, f"cap {cap} segments {segments} sample {sample}")
                st = t.search_many_stats()
                print(f"cap {cap} segments {segments} sample {sample}: {st}")
                if cap:   # the pairs do not fit the buffer at once: the threshold pass ran
                    assert st["launches"] >= 2
                else:     # they do: one emit launch, whatever the options
                    assert st["launches"] == 1 and st["candidates"] <= N_QUERIES * int(corpus.keeps("tags+stamp").sum())
    # the vote through the threshold pass and the pieces
    res = t.propose_groups(5)
    check_vote(corpus, res, int(NO_GROUP), None, 5, np.inf, "the vote, buffer at its floor")
    st = t.propose_groups_stats()
    print("the vote, buffer at its floor:", st)
    assert st["launches"] >= 2 and st["strips"] == 1
    # the one-residue mask with thresholds that never form: 257 queries x 70 rows overflow the buffer and go in pieces
    t.set_option("many_segments", 0)
    t.set_option("many_sample", 0)
    qs = np.concatenate([corpus.queries, corpus.rows[:128]])
    keep = corpus.keeps("sixteenth")
    assert 257 * int(keep.sum()) > 1 << 14
    Dq = np.concatenate([corpus.D, corpus.S[:128]])
    got = t.knn_many_where(qs, 16, **PREDICATES["sixteenth"])
    st = t.search_many_stats()
    print("one residue, 257 queries:", st)
    same(got[:2], oracle_many(Dq, 16, keep), "one residue in pieces")
    same(got[:2], where_loop(t, qs, 16, PREDICATES["sixteenth"])[0], "one residue in pieces against search_where")
    assert st["launches"] > 2 and st["candidates"] >= 256 * int(keep.sum())
    t.close()


# 3: the kNN graph with the answers narrowed
@pytest.mark.parametrize("k", [1, 5, 15])
def test_neighbors_where(corpus, table, k):
    pred, keep = PREDICATES["tags+stamp"], corpus.keeps("tags+stamp")
    first, n = 100, 60   # crosses the tile edge at row 128
    ids = np.arange(first, first + n, dtype=np.uint64)
    dead_in = [int(r) for r in corpus.dead if first <= r < first + n]
    sl = slice(first, first + n)
    assert dead_in and np.any(keep[sl]) and np.any(~keep[sl] & corpus.live[sl])
    got = table.neighbors_where(k, first, n, **pred)
    want = drop_self(*oracle_many(corpus.S[sl], k + 1, keep), ids)
    want[0][~corpus.live[sl]], want[1][~corpus.live[sl]] = NO_ID, np.inf
    same(got, want, f"neighbors_where k {k} against the oracle")
    many = table.knn_many_where(corpus.rows[sl], k + 1, **pred)
    mine = drop_self(many[0], many[1], ids)
    mine[0][~corpus.live[sl]], mine[1][~corpus.live[sl]] = NO_ID, np.inf
    same(got, mine, f"neighbors_where k {k} against knn_many_where minus self")
    assert not np.any(got[0] == ids[:, None]) and np.all(keep[got[0][got[0] != NO_ID].astype(np.int64)])
    for r in dead_in:
        assert np.all(got[0][r - first] == NO_ID) and np.all(np.isposinf(got[1][r - first]))
    whole = table.neighbors_where(k, **pred)
    same((whole[0][sl], whole[1][sl]), got, "a slice of the whole")
    assert np.all(whole[0][ZERO_ROW] == NO_ID)
    none = table.neighbors_where(k, first, n, **PREDICATES["nobody"])
    assert np.all(none[0] == NO_ID) and np.all(np.isposinf(none[1])) and table.search_many_stats()["launches"] == 0


# 4: the vote
def check_vote(corpus, res, ask_group, voters_name, k, max_dist, what):
    voters = None if voters_name is None else corpus.keeps(voters_name)
    g, v, h, d, tot = propose(corpus.S, corpus.groups, corpus.live, ask_group, voters, k, max_dist)
    assert np.array_equal(res["group"], g), (what, np.nonzero(res["group"] != g)[0][:8])
    assert np.array_equal(res["votes"], v) and np.array_equal(res["heard"], h), what
    assert np.array_equal(res["dist"].view(np.uint32), d.view(np.uint32)), what
    assert res["totals"] == tot, (what, res["totals"], tot)
    return g, v, h, d, tot


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("ask_group", [int(NO_GROUP), 2])
@pytest.mark.parametrize("voters", [None, "tags+stamp"])
def test_propose_groups_equals_the_restatement(corpus, table, k, ask_group, voters):
    before = table.groups()
    pred = {} if voters is None else PREDICATES[voters]
    res = table.propose_groups(k, ask_group=ask_group, **pred)
    st = table.propose_groups_stats()
    g, v, h, d, tot = check_vote(corpus, res, ask_group, voters, k, np.inf, f"k {k} ask {ask_group} voters {voters}")
    print(f"k {k} ask {ask_group} voters {voters}: totals {tot}, stats {st}")
    assert tot["askers"] > 100 and tot["voters"] > 100 and 0 < tot["proposed"] <= tot["askers"]
    assert res["group"][ZERO_ROW] == NO_GROUP and res["heard"][ZERO_ROW] == 0 and np.isposinf(res["dist"][ZERO_ROW])
    assert np.all(res["group"][corpus.dead] == NO_GROUP)
    assert st["strips"] == 1 and st["launches"] >= 1 and st["tiles"] >= 10 * 10 and int(h.sum()) <= st["candidates"] <= tot["askers"] * tot["voters"]
    assert np.array_equal(table.groups(), before) and np.array_equal(before, corpus.groups)
    # a window that ends exactly on one entry's distance: that entry is heard
    asker = int(np.nonzero(h == k)[0][0])
    cols = np.nonzero(corpus.live & (corpus.groups != NO_GROUP) & (corpus.groups != np.uint32(ask_group)) &
                      (True if voters is None else corpus.keeps(voters)))[0]
    edge = np.sort(corpus.S[asker, cols])[min(k, 3) - 1]
    res = table.propose_groups(k, max_dist=float(edge), ask_group=ask_group, **pred)
    g2, v2, h2, d2, tot2 = check_vote(corpus, res, ask_group, voters, k, edge, f"window, k {k} ask {ask_group} voters {voters}")
    assert h2[asker] == min(k, 3) and tot2["proposed"] <= tot["proposed"]
    assert np.all(dist_keys(res["dist"][res["group"] != NO_GROUP]) <= dist_keys(np.float32([edge]))[0])


def test_propose_groups_identities(corpus, table):
    voters = corpus.live & (corpus.groups != NO_GROUP)
    ids = np.nonzero(voters)[0].astype(np.uint64)
    res = table.propose_groups(1)
    askers = np.nonzero(corpus.live & (corpus.groups == NO_GROUP))[0]
    # (a) k = 1: the group of the nearest voter, as the filtered search finds it
    for r in askers[:48]:
        idx, dist = table.knn(corpus.rows[r], 1, within=ids)
        if idx[0] == NO_ID or np.isnan(dist[0]):
            assert res["group"][r] == NO_GROUP and r == ZERO_ROW
            continue
        assert res["group"][r] == corpus.groups[int(idx[0])] and res["votes"][r] == res["heard"][r] == 1
        assert res["dist"][r].view(np.uint32) == dist[0].view(np.uint32)
    assert ZERO_ROW in askers[:48]
    # (b) every voter in one group: every asker that hears anybody is proposed that group, unanimously
    t = EmbeddingTable(DIM, 0)
    t.insert(corpus.rows)
    t.delete(corpus.dead)
    one = np.where(corpus.groups == NO_GROUP, NO_GROUP, np.uint32(4)).astype(np.uint32)
    t.set_groups(one)
    res = t.propose_groups(7)
    heard_some = res["heard"] > 0
    assert np.all(res["group"][heard_some] == 4) and np.all(res["votes"][heard_some] == res["heard"][heard_some])
    assert np.all(res["heard"][askers[askers != ZERO_ROW]] == 7) and not heard_some[ZERO_ROW] and not np.any(heard_some[voters])
    assert res["totals"]["proposed"] == res["totals"]["unanimous"] == int(heard_some.sum()) == askers.size - 1
    # nobody to ask / nobody to vote: padding and the counts, no tile
    for kwargs, (n_ask, n_vote) in ((dict(ask_group=9), (0, int(voters.sum()))), (dict(ask_group=4), (int(voters.sum()), 0)),
                                    (dict(all_of=NOBODY), (askers.size, 0)), (dict(stamp=(5, 4)), (askers.size, 0))):
        res = t.propose_groups(3, **kwargs)
        assert np.all(res["group"] == NO_GROUP) and not res["votes"].any() and not res["heard"].any() and np.all(np.isposinf(res["dist"]))
        assert res["totals"] == {"askers": n_ask, "proposed": 0, "voters": n_vote, "unanimous": 0}, kwargs
        assert t.propose_groups_stats() == {"candidates": 0, "launches": 0, "tiles": 0, "strips": 0}
    t.close()
    # a table whose group column was never set: every live row asks, nobody votes
    t = EmbeddingTable(DIM, 0)
    t.insert(corpus.rows[:200])
    res = t.propose_groups(3)
    assert res["totals"] == {"askers": 200, "proposed": 0, "voters": 0, "unanimous": 0} and np.all(res["group"] == NO_GROUP)
    t.close()


# 5: sharded
@pytest.mark.parametrize("n_shards", [1, 2, 3])
def test_sharded_equals_the_single_table(corpus, table, n_shards):
    st = ShardedTable(DIM, (0,) * n_shards, 64)
    st.insert(corpus.rows)
    st.delete(corpus.dead)
    st.set_attrs(np.arange(N_ROWS), corpus.tags, corpus.stamps)
    st.set_groups(corpus.groups)
    for name in ("tags+stamp", "group", "few", "nobody", "never"):
        for k in (1, 16):
            got = st.knn_many_where(corpus.queries, k, **PREDICATES[name])
            want = table.knn_many_where(corpus.queries, k, **PREDICATES[name])
            same(got[:2], want[:2], f"{n_shards} shards, {name}, k {k}")
            assert got[2] == want[2] == int(corpus.keeps(name).sum())
    same(st.knn_many_where(corpus.queries, 4)[:2], table.knn_many(corpus.queries, 4), "sharded, no keywords")
    st.close()


# 6: the index
def test_index_suggest_folders_and_hidden_pictures(built):
    rng = np.random.default_rng(12)
    themes = rng.standard_normal((2, DIM)).astype(np.float32)
    n = 90
    theme = np.arange(n) % 2
    emb = (themes[theme] + 0.5 * rng.standard_normal((n, DIM))).astype(np.float32)
    # 30 sorted pictures per folder (dogs: theme 0, beach: theme 1), 30 of both themes in the inbox
    folder = ["inbox" if i >= 60 else ("dogs", "beach")[theme[i]] for i in range(n)]
    paths = [f"/media/{folder[i]}/p{i}.jpg" for i in range(n)]
    ix = ImageIndex(DIM, 0, "/media/")
    ix.insert(paths, emb)
    ix.remove([paths[61]])
    got = ix.suggest_folders("media/inbox", k=5)
    assert set(got) == set(paths[60:]) - {paths[61]}
    for i in range(60, n):
        if i != 61:
            name, votes, heard, dist = got[paths[i]]
            assert name == ix.group_name(ix.group_of(("media/dogs", "media/beach")[theme[i]]), web=False) and votes == heard == 5 and 0 < dist < 1
    assert all(v[0] in ("media/dogs/", "media/beach/") for v in ix.suggest_folders("media/inbox", k=5, web=True).values())
    assert ix.suggest_folders("media/inbox", k=5, max_dist=1e-6) == {} and ix.suggest_folders("media/inbox", k=5, min_votes=6) == {}
    # hidden pictures do not vote, and show up under no tag
    hidden = [p for i, p in enumerate(paths[:60]) if theme[i] == 0]   # every dog
    ix.set_attrs(hidden, tags=[HIDDEN] * len(hidden))
    got = ix.suggest_folders("media/inbox", k=5, none_of=HIDDEN)
    assert set(got) == set(paths[60:]) - {paths[61]} and all(v[0] == ix.group_name(ix.group_of("media/beach"), web=False) for v in got.values())
    best = ix.best_per_label(themes, names=["dog", "beach"], k=6)
    narrowed = ix.best_per_label_where(themes, names=["dog", "beach"], k=6, none_of=HIDDEN)
    assert set(p for p, _ in best["dog"]) & set(hidden) and not (set(p for p, _ in narrowed["dog"]) | set(p for p, _ in narrowed["beach"])) & set(hidden)
    assert narrowed["beach"] == [e for e in ix.best_per_label(themes, names=["dog", "beach"], k=16)["beach"] if e[0] not in hidden][:6]
    rel = ix.related_where(k=3, none_of=HIDDEN)
    assert set(rel) == set(paths) - {paths[61]} and hidden[0] in rel
    assert not set(q for hits in rel.values() for q, _ in hits) & (set(hidden) | {paths[61]}) and all(len(h) == 3 for h in rel.values())
    ix.close()


# 7: the errors
def test_errors(corpus, table):
    mi = _lib.lib()
    q = corpus.queries.ctypes.data
    idx, d = np.full((4, 17), 7, np.uint64), np.full((4, 17), 7.0, np.float32)
    g, v, h = (np.full(N_ROWS, 7, np.uint32) for _ in range(3))
    dd = np.full(N_ROWS, 7.0, np.float32)
    tot = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    matched = ctypes.c_uint64(7)
    ok, bad = make_where(all_of=FAVOURITE), make_where(all_of=FAVOURITE)
    bad.flags = 2
    W, B, M = ctypes.byref(ok), ctypes.byref(bad), ctypes.byref(matched)

    def err(rc, code):
        assert rc == code
        assert len(mi.mi_last_error()) > 0

    err(mi.mi_knn_search_many_where(table._h, q, 4, 17, W, idx.ctypes.data, d.ctypes.data, M), MI_ERR_UNSUPPORTED)
    err(mi.mi_knn_search_many_where(table._h, q, 4, 0, W, idx.ctypes.data, d.ctypes.data, M), MI_ERR_INVALID)
    err(mi.mi_knn_search_many_where(table._h, q, 0, 4, W, idx.ctypes.data, d.ctypes.data, M), MI_ERR_INVALID)
    err(mi.mi_knn_search_many_where(table._h, None, 4, 4, W, idx.ctypes.data, d.ctypes.data, M), MI_ERR_INVALID)
    err(mi.mi_knn_search_many_where(table._h, q, 4, 4, W, None, d.ctypes.data, M), MI_ERR_INVALID)
    err(mi.mi_knn_search_many_where(table._h, q, 4, 4, B, idx.ctypes.data, d.ctypes.data, M), MI_ERR_INVALID)
    err(mi.mi_knn_neighbors_where(table._h, 0, 4, 16, W, idx.ctypes.data, d.ctypes.data), MI_ERR_UNSUPPORTED)
    err(mi.mi_knn_neighbors_where(table._h, 0, 4, 0, W, idx.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_neighbors_where(table._h, 0, 4, 4, B, idx.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    err(mi.mi_knn_neighbors_where(table._h, 0, 4, 4, W, None, d.ctypes.data), MI_ERR_INVALID)
    for first, n in ((N_ROWS, 1), (N_ROWS - 3, 8), (1 << 50, 1)):
        err(mi.mi_knn_neighbors_where(table._h, first, n, 4, W, idx.ctypes.data, d.ctypes.data), MI_ERR_INVALID)
    assert mi.mi_knn_neighbors_where(table._h, N_ROWS, 0, 4, W, None, None) == 0

    def vote(k=4, max_dist=np.inf, ask=int(NO_GROUP), w=None, group=g.ctypes.data, handle=table._h):
        return mi.mi_knn_propose_groups(handle, k, max_dist, ask, w, group, v.ctypes.data, h.ctypes.data, dd.ctypes.data, tot)

    err(vote(k=0), MI_ERR_INVALID)
    err(vote(k=17), MI_ERR_UNSUPPORTED)
    err(vote(max_dist=np.nan), MI_ERR_INVALID)
    err(vote(max_dist=-1e-9), MI_ERR_INVALID)
    err(vote(ask=1 << 24), MI_ERR_INVALID)
    err(vote(ask=0xFFFFFFFE), MI_ERR_INVALID)
    err(vote(w=B), MI_ERR_INVALID)
    err(vote(group=None), MI_ERR_INVALID)
    err(mi.mi_knn_propose_groups_stats(table._h, None), MI_ERR_INVALID)
    odd = EmbeddingTable(192, 0)
    odd.insert(np.ones((4, 192), np.float32))
    err(mi.mi_knn_search_many_where(odd._h, q, 4, 4, W, idx.ctypes.data, d.ctypes.data, M), MI_ERR_UNSUPPORTED)
    err(vote(handle=odd._h), MI_ERR_UNSUPPORTED)
    odd.close()
    sh = ShardedTable(DIM, (0, 0), 64)
    sh.insert(corpus.rows[:300])
    borrowed = ctypes.c_void_p(mi.mi_knn_sharded_shard(sh._h, 1))
    err(vote(handle=borrowed), MI_ERR_UNSUPPORTED)
    err(mi.mi_knn_neighbors_where(borrowed, 0, 4, 4, W, idx.ctypes.data, d.ctypes.data), MI_ERR_UNSUPPORTED)
    err(mi.mi_knn_sharded_search_many_where(sh._h, q, 4, 17, W, idx.ctypes.data, d.ctypes.data, M), MI_ERR_UNSUPPORTED)
    err(mi.mi_knn_sharded_search_many_where(sh._h, q, 4, 4, B, idx.ctypes.data, d.ctypes.data, M), MI_ERR_INVALID)
    sh.close()
    # no error wrote anything
    assert np.all(idx == 7) and np.all(d == 7.0) and matched.value == 7 and list(tot) == [7, 7, 7, 7]
    assert all(np.all(a == 7) for a in (g, v, h, dd))
    # max_dist = -0 is a window, not an error; NULL for everything but `group` is allowed
    assert vote(max_dist=-0.0) == 0 and list(tot)[1] == 0
    assert mi.mi_knn_propose_groups(table._h, 4, np.inf, int(NO_GROUP), None, g.ctypes.data, None, None, None, None) == 0
    assert np.array_equal(g, table.propose_groups(4)["group"])
    # the empty table: padding (there is none to write), zero counts
    empty = EmbeddingTable(DIM, 0)
    i2, d2, m2 = empty.knn_many_where(corpus.queries[:3], 4, **PREDICATES["all"])
    assert np.all(i2 == NO_ID) and np.all(np.isposinf(d2)) and m2 == 0
    assert empty.neighbors_where(4, **PREDICATES["all"])[0].shape == (0, 4)
    res = empty.propose_groups(4)
    assert res["group"].size == 0 and res["totals"] == {"askers": 0, "proposed": 0, "voters": 0, "unanimous": 0}
    empty.close()
