"""Host-side mirror of the reference's query/refine loop and kNN statement
(/root/reference/server/src/search.rs) on top of the C ABI.

`average_slices` and `refine_query` keep the reference's names, argument meaning
and error behaviour (search.rs:127-150, :60-67); `EmbeddingTable` stands where the
SurrealDB table `image` + index `mt_pts` stood (clip.rs:135-143) and its
`knn()` is the `embedding <|K|> $reference` statement (search.rs:70-86).
`ShardedTable` is the multi-GPU form: one process per GPU, rows split
contiguously, per-shard top-k all-gathered (RCCL over xGMI via torch.distributed)
and merged identically on every rank.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from ._lib import MI_KNN_WHERE_GROUP, KnnWhere, c_f, c_vp, check, lib

K_REFERENCE = 1000  # `<|1000|>` in server/src/search.rs:76
NO_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_LABEL = np.uint32(0xFFFFFFFF)  # MI_KNN_NO_LABEL: the label of a deleted row


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


COMPOUND_MODES = {"all": 0, "any": 1}   # MI_COMPOUND_ALL / MI_COMPOUND_ANY


def _compound_args(dim: int, terms, mode, without, without_within):
    """(pos [n_pos, dim], mode code, neg or None, thresholds or None, n_neg) as mi_knn_search_compound takes them"""
    if mode not in COMPOUND_MODES:
        raise ValueError(f"mode must be 'all' or 'any' (got {mode!r})")
    pos = _f32(terms).reshape(-1, dim)
    if without is None:
        if without_within is not None:
            raise ValueError("without_within given without `without`")
        return pos, COMPOUND_MODES[mode], None, None, 0
    neg = _f32(without).reshape(-1, dim)
    if without_within is None:
        raise ValueError("`without` needs without_within: one cosine distance per negative term (or one for all)")
    w = _f32(without_within).reshape(-1)
    if w.size == 1 and neg.shape[0] != 1:
        w = np.repeat(w, neg.shape[0])
    if w.size != neg.shape[0]:
        raise ValueError(f"{w.size} thresholds for {neg.shape[0]} negative terms")
    return pos, COMPOUND_MODES[mode], neg, _f32(w), neg.shape[0]


def _among(within):
    """(pointer or None, count, the array to keep alive) of an id list; an empty list is an empty row set, not every row"""
    if within is None:
        return None, 0, None
    a = _ids(within)
    keep = a if a.size else np.zeros(1, np.uint64)
    return keep.ctypes.data, a.size, keep


def _page_call(fn, handle, dim, lead, reference, k, after, max_dist, tail_ptr=None, within=None):
    """one mi_*_search_page call -> (idx [k], dist [k], counts dict, next): `lead` = the arguments between the query and k
    (the index's references and folders), within = the id list of the table calls; next = the (dist, id) cursor of the last hit,
    None when the page came back short (nothing is left behind it)"""
    q = _f32(reference).reshape(-1)
    if q.size != dim:
        raise ValueError(f"a query of {q.size} floats for dim {dim}")
    k = int(k)
    idx, dist = np.empty(max(k, 1), np.uint64), np.empty(max(k, 1), np.float32)
    counts = (ctypes.c_uint64 * 4)()
    a_dist, a_id = (0.0, int(NO_ID)) if after is None else (float(after[0]), int(after[1]))
    args = [handle, q.ctypes.data] + list(lead) + [k, a_dist, a_id, float(max_dist)]
    if tail_ptr is None:
        ids, n_ids, _keep = _among(within)
        args += [ids, n_ids, idx.ctypes.data, dist.ctypes.data, counts]
    else:
        args += [idx.ctypes.data, dist.ctypes.data, tail_ptr, counts]
    check(fn(*args))
    idx, dist = idx[:k], dist[:k]
    full = k > 0 and idx[k - 1] != NO_ID
    nxt = (dist[k - 1], int(idx[k - 1])) if full else None   # the np.float32 itself: -0 and +0 are different cursors
    return idx, dist, {"before": counts[0], "window": counts[1], "beyond": counts[2], "nan": counts[3]}, nxt


NO_GROUP = np.uint32(0xFFFFFFFF)  # MI_KNN_NO_GROUP: a row that belongs to no group


def _set_groups(fn, h, groups, ids):
    g = np.ascontiguousarray(np.asarray(groups, dtype=np.uint32).reshape(-1))
    a = None if ids is None else _ids(ids)
    if a is not None and a.size != g.size:
        raise ValueError(f"{g.size} groups for {a.size} ids")
    check(fn(h, a.ctypes.data if a is not None and a.size else None, g.size, g.ctypes.data if g.size else None))


def _get_groups(fn, h, ids, rows):
    a = None if ids is None else _ids(ids)
    n = rows if a is None else a.size
    out = np.empty(max(n, 1), np.uint32)
    check(fn(h, a.ctypes.data if a is not None and a.size else None, n, out.ctypes.data))
    return out[:n]


def _grouped_call(fn, handle, dim, lead, reference, k, max_dist, n_groups, facets, tail_ptr=None, within=None):
    """one mi_*_search_grouped call -> (idx [k], dist [k], group [k], members [k], totals dict[, facets [n_groups]]): `lead` =
    the arguments between the query and k (the index's references and folders), within = the id list of the table calls"""
    q = _f32(reference).reshape(-1)
    if q.size != dim:
        raise ValueError(f"a query of {q.size} floats for dim {dim}")
    k = int(k)
    idx, dist = np.empty(max(k, 1), np.uint64), np.empty(max(k, 1), np.float32)
    group, members = np.empty(max(k, 1), np.uint32), np.empty(max(k, 1), np.uint64)
    totals = (ctypes.c_uint64 * 4)()
    fac = np.zeros(max(int(n_groups), 1), np.uint64) if facets else None
    args = [handle, q.ctypes.data] + list(lead) + [k, float(max_dist)]
    if tail_ptr is None:
        ids, n_ids, _keep = _among(within)
        args += [ids, n_ids, idx.ctypes.data, dist.ctypes.data, group.ctypes.data, members.ctypes.data]
    else:
        args += [idx.ctypes.data, dist.ctypes.data, group.ctypes.data, members.ctypes.data, tail_ptr]
    args += [fac.ctypes.data if facets else None, int(n_groups) if facets else 0, totals]
    check(fn(*args))
    out = (idx[:k], dist[:k], group[:k], members[:k],
           {"groups": totals[0], "window": totals[1], "beyond": totals[2], "nan": totals[3]})
    return out + (fac[:int(n_groups)],) if facets else out


STAMP_MIN, STAMP_MAX = -(1 << 63), (1 << 63) - 1


def make_where(all_of=0, any_of=0, none_of=0, stamp=(None, None), group=None) -> KnnWhere:
    """The predicate of the *_where calls (mi_knn_where).  all_of / any_of / none_of: masks over the 64 tag bits (any_of = 0:
    clause absent); stamp = (lo, hi), inclusive and signed, None = open on that side, lo > hi matches nothing; group: None (any)
    or a group id — NO_GROUP selects the rows without a group, and a table without a group column matches nothing."""
    lo, hi = stamp
    w = KnnWhere(int(all_of) & 0xFFFFFFFFFFFFFFFF, int(any_of) & 0xFFFFFFFFFFFFFFFF, int(none_of) & 0xFFFFFFFFFFFFFFFF,
                 STAMP_MIN if lo is None else int(lo), STAMP_MAX if hi is None else int(hi), 0, 0)
    if group is not None:
        w.group, w.flags = int(group), MI_KNN_WHERE_GROUP
    return w


def _set_attrs(fn, h, ids, tags, stamps):
    a = _ids(ids)
    tg = None if tags is None else np.ascontiguousarray(np.asarray(tags, dtype=np.uint64).reshape(-1))
    st = None if stamps is None else np.ascontiguousarray(np.asarray(stamps, dtype=np.int64).reshape(-1))
    for name, col in (("tags", tg), ("stamps", st)):
        if col is not None and col.size != a.size:
            raise ValueError(f"{col.size} {name} for {a.size} ids")
    check(fn(h, a.ctypes.data if a.size else None, a.size, tg.ctypes.data if tg is not None and tg.size else None,
             st.ctypes.data if st is not None and st.size else None))


def _get_attrs(fn, h, ids, rows):
    a = np.arange(rows, dtype=np.uint64) if ids is None else _ids(ids)
    tags, stamps = np.zeros(max(a.size, 1), np.uint64), np.zeros(max(a.size, 1), np.int64)
    check(fn(h, a.ctypes.data if a.size else None, a.size, tags.ctypes.data, stamps.ctypes.data))
    return tags[:a.size], stamps[:a.size]


def _count_where(fn, h, where) -> int:
    n = ctypes.c_uint64()
    check(fn(h, ctypes.byref(where), ctypes.byref(n)))
    return n.value


def _search_where(fn, h, dim, reference, k, where):
    """one mi_*_search_where call -> (idx, dist, matched); reference [dim] or [nq, dim]"""
    q = _f32(reference)
    single = q.ndim == 1
    q = q.reshape(-1, dim)
    k = int(k)
    idx, dist = np.empty((q.shape[0], max(k, 1)), np.uint64), np.empty((q.shape[0], max(k, 1)), np.float32)
    matched = ctypes.c_uint64()
    check(fn(h, q.ctypes.data, q.shape[0], k, ctypes.byref(where), idx.ctypes.data, dist.ctypes.data, ctypes.byref(matched)))
    idx, dist = idx[:, :k], dist[:, :k]
    return (idx[0], dist[0], matched.value) if single else (idx, dist, matched.value)


MI_KNN_ORDER_DESC, MI_KNN_ORDER_AFTER = 1, 2


def _where_or_null(predicate):
    """the keyword arguments of make_where -> a pointer to the structure, or None (NULL: every live row) when there are none"""
    if not predicate:
        return None, None
    w = make_where(**predicate)
    return ctypes.byref(w), w


def _many_where(fn, h, dim, queries, k, predicate):
    """one mi_*_search_many_where call -> (idx [nq, k], dist [nq, k], matched)"""
    q = _f32(queries).reshape(-1, dim)
    idx, dist = np.empty((q.shape[0], int(k)), np.uint64), np.empty((q.shape[0], int(k)), np.float32)
    matched = ctypes.c_uint64()
    wp, _w = _where_or_null(predicate)
    check(fn(h, q.ctypes.data, q.shape[0], int(k), wp, idx.ctypes.data, dist.ctypes.data, ctypes.byref(matched)))
    return idx, dist, matched.value


def _ordered_call(fn, handle, dim, lead, reference, k, max_dist, descending, after, predicate, n_found=False):
    """one mi_*_search_ordered call -> (idx [k], dist [k], stamps [k], counts dict): `lead` = the arguments between the query and
    k (the index's references); after = None or the (stamp, id) of the previous page's last hit"""
    q = _f32(reference).reshape(-1)
    if q.size != dim:
        raise ValueError(f"a query of {q.size} floats for dim {dim}")
    k = int(k)
    idx, dist, stamps = np.empty(max(k, 1), np.uint64), np.empty(max(k, 1), np.float32), np.empty(max(k, 1), np.int64)
    counts = (ctypes.c_uint64 * 4)()
    wp, _keep = _where_or_null(predicate)
    flags = (MI_KNN_ORDER_DESC if descending else 0) | (MI_KNN_ORDER_AFTER if after is not None else 0)
    a_stamp, a_id = (0, 0) if after is None else (int(after[0]), int(after[1]))
    args = [handle, q.ctypes.data] + list(lead) + [k, float(max_dist), wp, flags, a_stamp, a_id, idx.ctypes.data, dist.ctypes.data,
                                                    stamps.ctypes.data]
    if n_found:
        args.append(None)
    check(fn(*(args + [counts])))
    return idx[:k], dist[:k], stamps[:k], {"within": counts[0], "before": counts[1], "beyond": counts[2], "nan": counts[3]}


def _timeline(page, k):
    """page(after) -> (idx, dist, stamps, counts), called until a page comes back short: yields each with the padding cut off"""
    after = None
    while True:
        idx, dist, stamps, counts = page(after)
        n = int((idx != NO_ID).sum())
        if n:
            yield idx[:n], dist[:n], stamps[:n], counts
        if n < int(k):
            return
        after = (int(stamps[n - 1]), int(idx[n - 1]))


def _stamp_histogram(fn, handle, dim, lead, reference, edges, max_dist, predicate):
    q = _f32(reference).reshape(-1)
    if q.size != dim:
        raise ValueError(f"a query of {q.size} floats for dim {dim}")
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1))
    hist = np.zeros(e.size + 1, np.uint64)
    wp, _keep = _where_or_null(predicate)
    check(fn(*([handle, q.ctypes.data] + list(lead) + [float(max_dist), wp, e.ctypes.data if e.size else None, e.size, hist.ctypes.data])))
    return hist


def _pairs_call(fn, lead, cap: int):
    """fn(*lead, a, b, dist, cap, &count) of the join calls -> (a, b, dist) cut to the pairs found"""
    a, b = np.empty(cap, np.uint64), np.empty(cap, np.uint64)
    dist = np.empty(cap, np.float32)
    n = ctypes.c_uint64()
    check(fn(*lead, a.ctypes.data if cap else None, b.ctypes.data if cap else None, dist.ctypes.data if cap else None, cap,
             ctypes.byref(n)))
    return a[:n.value].copy(), b[:n.value].copy(), dist[:n.value].copy()


def _dbscan_call(fn, lead, n: int) -> dict:
    """fn(*lead, cluster, via, via_dist, counts, summary) of the dbscan calls over n rows -> EmbeddingTable.dbscan's dict"""
    cluster, via = np.empty(n, np.uint64), np.empty(n, np.uint64)
    via_dist, counts = np.empty(n, np.float32), np.empty(n, np.uint32)
    summary = np.zeros(4, np.uint64)
    check(fn(*lead, cluster.ctypes.data, via.ctypes.data, via_dist.ctypes.data, counts.ctypes.data, summary.ctypes.data))
    return {"labels": dense_labels(cluster), "cluster": cluster, "via": via, "via_dist": via_dist, "counts": counts,
            "summary": dict(zip(("clusters", "core", "border", "noise"), (int(v) for v in summary)))}


def _ptrs(vecs):
    arr = (c_f * len(vecs))()
    for i, v in enumerate(vecs):
        arr[i] = v.ctypes.data_as(c_f)
    return arr


def average_slices(vectors: Sequence[np.ndarray]) -> np.ndarray:
    """fn average_slices(vectors: &Vec<&Vec<f32>>) -> Vec<f32>  (search.rs:127-150).
    Panics in the reference on empty input / ragged lengths; raises here."""
    if len(vectors) == 0:
        raise AssertionError("Input must not be empty")
    vecs = [_f32(v).reshape(-1) for v in vectors]
    n = vecs[0].size
    if any(v.size != n for v in vecs):
        raise AssertionError("All vectors must have the same length")
    out = np.empty(n, np.float32)
    check(lib().mi_average_slices(_ptrs(vecs), len(vecs), n, out.ctypes.data_as(c_f)))
    return out


def refine_query(text_embedding: np.ndarray, selected: Sequence[np.ndarray]) -> np.ndarray:
    """search.rs:28,:60-67 — no marked image found: the text vector itself; else
    average_slices([average_slices(selected), text])."""
    text = _f32(text_embedding).reshape(-1)
    sel = [_f32(v).reshape(-1) for v in selected]
    if any(v.size != text.size for v in sel):
        raise AssertionError("All vectors must have the same length")
    out = np.empty_like(text)
    check(lib().mi_refine(text.ctypes.data_as(c_f), _ptrs(sel), len(sel), text.size, out.ctypes.data_as(c_f)))
    return out


class EmbeddingTable:
    """One row-shard of `image.embedding` resident in HBM (mi_knn)."""

    def __init__(self, dim: int = 768, device: int = 0, base: int = 0):
        self._h = c_vp()
        self.dim, self.device = dim, device
        check(lib().mi_knn_create(dim, device, ctypes.byref(self._h)))
        if base:
            self.set_base(base)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().mi_knn_free(self._h)
            self._h = c_vp()

    __del__ = close

    def __len__(self) -> int:
        n = ctypes.c_uint64()
        check(lib().mi_knn_size(self._h, ctypes.byref(n)))
        return n.value

    def set_base(self, base: int):
        check(lib().mi_knn_set_base(self._h, base))
        self._base_id = int(base)

    def reserve(self, rows: int):
        check(lib().mi_knn_reserve(self._h, rows))

    def set_option(self, key: str, value: int):
        """mi_knn_set_option: "prefilter" = 1 turns on the two-stage exact search (bf16 mirror, + 50 % memory)."""
        check(lib().mi_knn_set_option(self._h, key.encode(), int(value)))
        self._options = {**getattr(self, "_options", {}), key: int(value)}   # (what a call that overrides one restores)

    def prefilter_stats(self):
        """(rows re-evaluated by stage 2, fell back to the single pass) of the most recent single-query search"""
        c, f = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib().mi_knn_prefilter_stats(self._h, ctypes.byref(c), ctypes.byref(f)))
        return c.value, bool(f.value)

    def prefilter_state(self):
        """mi_knn_prefilter_state: the two-stage search's view of itself"""
        out = (ctypes.c_uint32 * 4)()
        check(lib().mi_knn_prefilter_state(self._h, out))
        return {"skips_left": out[0], "consecutive_fallbacks": out[1], "searches_skipped": out[2], "scales_taken_at_rows": out[3]}

    def insert(self, embeddings: np.ndarray):
        """db.insert("image").content(rows) (clip.rs:125-137): ids are insertion ordinals."""
        e = _f32(embeddings).reshape(-1, self.dim)
        check(lib().mi_knn_append(self._h, e.ctypes.data, e.shape[0]))

    def insert_device(self, d_ptr: int, n: int, stream: int = 0):
        check(lib().mi_knn_append_device(self._h, d_ptr, n, stream))

    def insert_synthetic(self, seed: int, first_row: int, n: int):
        check(lib().mi_knn_append_synthetic(self._h, seed, first_row, n))

    def rows(self, first: int, n: int) -> np.ndarray:
        out = np.empty((n, self.dim), np.float32)
        check(lib().mi_knn_get_rows(self._h, first, n, out.ctypes.data))
        return out

    def delete(self, ids) -> int:
        """`DELETE FROM image WHERE id IN $ids` (mi_knn_delete): the rows keep their ids and storage, no later search
        returns them.  All ids must be rows of the table (else nothing changes).  Returns the rows that were live."""
        return _delete(lib().mi_knn_delete, self._h, ids)

    def deleted(self) -> np.ndarray:
        """ids of the deleted rows, ascending (mi_knn_deleted)"""
        return _deleted(lib().mi_knn_deleted, self._h)

    def compact(self) -> dict:
        """The deleted rows leave the table physically (mi_knn_compact): the survivors close up in order and take new ids,
        their groups, tags and stamps travel with them, and every search runs the code of a table without deletions
        again.  Returns {"removed": rows reclaimed, "new_ids": [rows before the call] uint64, the new id of every old
        row, NO_ID for a deleted one}.  Ids held outside the table (label arrays, page / ordered cursors) must be mapped
        through new_ids."""
        return _compact(lib().mi_knn_compact, self._h, len(self))

    def compact_stats(self) -> dict:
        """mi_knn_compact_stats, of the last compact on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_compact_stats(self._h, out))
        return {"removed": out[0], "moved": out[1], "straight": out[2], "staged": out[3]}

    def knn(self, reference: np.ndarray, k: int = K_REFERENCE, within=None):
        """`WHERE embedding <|k|> $reference` (search.rs:70-77): (ids, cosine distances),
        ascending distance then id.  reference: [dim] or [nq,dim].
        within: ids (any order, duplicates allowed): the k nearest among those rows only
        (mi_knn_search_filtered; deleted rows left out, k <= 4096)."""
        q = _f32(reference)
        single = q.ndim == 1
        q = q.reshape(-1, self.dim)
        idx = np.empty((q.shape[0], k), np.uint64)
        dist = np.empty((q.shape[0], k), np.float32)
        if within is None:
            check(lib().mi_knn_search(self._h, q.ctypes.data, q.shape[0], k, idx.ctypes.data, dist.ctypes.data))
        else:
            ids = _ids(within)
            check(lib().mi_knn_search_filtered(self._h, q.ctypes.data, q.shape[0], k, ids.ctypes.data if ids.size else None,
                                               ids.size, idx.ctypes.data, dist.ctypes.data))
        return (idx[0], dist[0]) if single else (idx, dist)

    def knn_device(self, d_q: int, nq: int, k: int, d_idx: int, d_dist: int, stream: int = 0, batched: bool = False):
        fn = lib().mi_knn_search_batched_device if batched else lib().mi_knn_search_device
        check(fn(self._h, d_q, nq, k, d_idx, d_dist, stream))

    def near_pairs(self, max_dist: float, first_new: int = 0, cap: int = 1 << 20):
        """Near-duplicates (mi_knn_near_pairs): every pair of live rows a < b with cosine distance <= max_dist as
        (a, b, dist), ascending by (a, b); dist is what knn(row a) reports for row b, bit for bit.  first_new: only pairs
        with b >= first_new.  More than `cap` pairs: MiError (MI_ERR_UNSUPPORTED) — lower max_dist or raise cap."""
        a, b = np.empty(cap, np.uint64), np.empty(cap, np.uint64)
        dist = np.empty(cap, np.float32)
        n = ctypes.c_uint64()
        check(lib().mi_knn_near_pairs(self._h, float(max_dist), int(first_new), a.ctypes.data if cap else None,
                                      b.ctypes.data if cap else None, dist.ctypes.data if cap else None, cap, ctypes.byref(n)))
        return a[:n.value].copy(), b[:n.value].copy(), dist[:n.value].copy()

    def near_pairs_stats(self):
        """mi_knn_near_pairs_stats, of the last near_pairs on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_near_pairs_stats(self._h, out))
        return {"candidates": out[0], "pairs": out[1], "strips": out[2], "tiles": out[3]}

    def near_pairs_with(self, other: "EmbeddingTable", max_dist: float, cap: int = 1 << 20):
        """The join with another table (mi_knn_near_pairs_between): every pair of a live row of this table and a live row of
        `other` with cosine distance <= max_dist as (a, b, dist) — a: ids of this table, b: ids of `other`, ascending by
        (a, b); dist is what other.knn(row a of this table) reports for row b, bit for bit.  Neither table changes.  More
        than `cap` pairs: MiError (MI_ERR_UNSUPPORTED)."""
        return _pairs_call(lib().mi_knn_near_pairs_between, (self._h, other._h, float(max_dist)), cap)

    def near_pairs_with_stats(self):
        """mi_knn_near_pairs_between_stats, of the last near_pairs_with on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_near_pairs_between_stats(self._h, out))
        return {"candidates": out[0], "pairs": out[1], "launches": out[2], "tiles": out[3]}

    def neighbor_counts(self, max_dist: float) -> np.ndarray:
        """How crowded is it around every row (mi_knn_density): counts [rows] uint32 = the pairs of near_pairs(max_dist) that
        contain the row, the row itself not counted; 0 for a deleted row — and for an outlier.  No pair list is built."""
        counts = np.empty(len(self), np.uint32)
        check(lib().mi_knn_density(self._h, float(max_dist), counts.ctypes.data))
        return counts

    def dbscan(self, max_dist: float, min_pts: int = 5) -> dict:
        """Density clusters without a k (mi_knn_dbscan) over the pairs of near_pairs(max_dist), which never leave the device.
        A row is a core when it has at least min_pts - 1 neighbours within max_dist (scikit-learn's min_samples: the row
        itself counts); clusters are the components of the core rows; a non-core row beside a core is a border row of the
        cluster of its nearest core (distance key, then row); the rest is noise.  Arrays by local row:
        labels (int64: 0 .. C - 1 in the order of the clusters' smallest core ids, -1 noise or deleted, as scikit-learn numbers
        them), cluster (uint64: the id of the cluster's smallest core row, NO_ID), via (uint64: a core's own id, the core a
        border row joined through, NO_ID), via_dist (float32: +0, that pair's distance bits, +inf), counts (uint32: the
        neighbours within), summary {"clusters", "core", "border", "noise"}.
        labels.astype(np.uint32) fits set_groups (-1 becomes NO_GROUP: a row of its own), so knn_grouped then answers "the best
        picture of each theme"."""
        return _dbscan_call(lib().mi_knn_dbscan, (self._h, float(max_dist), int(min_pts)), len(self))

    def near_pairs_window(self, max_dist: float, window: int, first_new: int = 0, cap: int = 1 << 20):
        """Bursts (mi_knn_near_pairs_window): the pairs of near_pairs(max_dist, first_new) whose stamps (set_attrs) lie within
        `window` of each other — |stamp_a - stamp_b| <= window, taken exactly over the whole int64 range; window 0: equal stamps,
        2**64 - 1: every pair.  Same ids, order and distance bits; a table without stamps: near_pairs itself."""
        return _pairs_call(lib().mi_knn_near_pairs_window, (self._h, float(max_dist), int(window), int(first_new)), cap)

    def neighbor_counts_window(self, max_dist: float, window: int) -> np.ndarray:
        """neighbor_counts over the pairs of near_pairs_window(max_dist, window) (mi_knn_density_window)"""
        counts = np.empty(len(self), np.uint32)
        check(lib().mi_knn_density_window(self._h, float(max_dist), int(window), counts.ctypes.data))
        return counts

    def dbscan_window(self, max_dist: float, window: int, min_pts: int = 5) -> dict:
        """Events (mi_knn_dbscan_window): dbscan whose neighbourhood is "within max_dist and within `window` in time" (ST-DBSCAN)
        — dbscan's contract and dict over the pairs of near_pairs_window(max_dist, window): "beach 2019" and "beach 2023" come
        out as two clusters."""
        return _dbscan_call(lib().mi_knn_dbscan_window, (self._h, float(max_dist), int(window), int(min_pts)), len(self))

    def window_stats(self) -> dict:
        """mi_knn_window_stats, of the last near_pairs_window / neighbor_counts_window / dbscan_window on this table; per pass
        tiles + tiles_skipped = the triangle's tiles"""
        out = (ctypes.c_uint64 * 8)()
        check(lib().mi_knn_window_stats(self._h, out))
        return dict(zip(("candidates_pass1", "pairs", "tiles_pass1", "tiles_skipped_pass1", "candidates_pass2", "tiles_pass2",
                         "tiles_skipped_pass2", "launches"), (int(v) for v in out)))

    def neighbor_counts_levels(self, max_dists) -> np.ndarray:
        """neighbor_counts at several distances from one tile pass (mi_knn_density_levels): counts [L, rows] uint32, row l =
        neighbor_counts(max_dists[l]).  max_dists: strictly ascending, at most LEVELS_MAX of them."""
        d = _levels(max_dists)
        counts = np.empty((d.size, len(self)), np.uint32)
        check(lib().mi_knn_density_levels(self._h, d.ctypes.data, d.size, counts.ctypes.data))
        return counts

    def dbscan_levels(self, max_dists, min_pts: int = 5) -> dict:
        """dbscan at several distances from the two tile passes one call runs (mi_knn_dbscan_levels): "tighter / looser
        themes".  max_dists: strictly ascending, at most LEVELS_MAX of them.  Every array is [L, rows] and its row l is what
        dbscan(max_dists[l], min_pts) returns, to the bit: labels (int64, dense per level), cluster, via, via_dist, counts;
        dense_labels = labels; summary = a list of L dicts {"clusters", "core", "border", "noise"}.
        tree: for l < L - 1 an int64 array that maps the dense label of a level-l cluster to the dense label of its parent at
        level l + 1 — the cluster its core rows lie in there (mi_dbscan_levels_tree).  The tree is over clusters through
        their core rows: a border row may sit in a level-(l + 1) cluster that is not the parent of its level-l cluster."""
        d = _levels(max_dists)
        L, n = d.size, len(self)
        cluster, via = np.empty((L, n), np.uint64), np.empty((L, n), np.uint64)
        via_dist, counts = np.empty((L, n), np.float32), np.empty((L, n), np.uint32)
        summary = np.zeros((L, 4), np.uint64)
        check(lib().mi_knn_dbscan_levels(self._h, d.ctypes.data, L, int(min_pts), cluster.ctypes.data, via.ctypes.data,
                                         via_dist.ctypes.data, counts.ctypes.data, summary.ctypes.data))
        labels = np.stack([dense_labels(c) for c in cluster]) if L else np.empty((0, n), np.int64)
        level, child, parent = dbscan_levels_tree(cluster, counts, min_pts)
        names = [np.unique(c[c != NO_ID]) for c in cluster]
        tree = [np.searchsorted(names[l + 1], parent[level == l]).astype(np.int64) for l in range(L - 1)]
        return {"labels": labels, "dense_labels": labels, "cluster": cluster, "via": via, "via_dist": via_dist, "counts": counts,
                "summary": [dict(zip(("clusters", "core", "border", "noise"), (int(v) for v in row))) for row in summary],
                "tree": tree}

    def dbscan_stats(self) -> dict:
        """mi_knn_dbscan_stats, of the last neighbor_counts / dbscan / neighbor_counts_levels / dbscan_levels on this table
        (after a *_levels call: pairs = those of the top level, unions_merged = summed over the levels)"""
        out = (ctypes.c_uint64 * 8)()
        check(lib().mi_knn_dbscan_stats(self._h, out))
        return dict(zip(("candidates_pass1", "pairs", "tiles_pass1", "candidates_pass2", "tiles_visited", "tiles_skipped",
                         "unions_merged", "launches"), (int(v) for v in out)))

    def assign(self, vectors: np.ndarray):
        """Label every row by the nearest of C vectors (mi_knn_assign): (labels [rows] uint32, dist [rows] f32) — for a live
        row what a table of the vectors answers to knn(row, 1), id and distance bits; NO_LABEL / +inf for a deleted row."""
        v = _f32(vectors).reshape(-1, self.dim)
        n = len(self)
        labels, dist = np.empty(n, np.uint32), np.empty(n, np.float32)
        check(lib().mi_knn_assign(self._h, v.ctypes.data, v.shape[0], labels.ctypes.data, dist.ctypes.data))
        return labels, dist

    def assign_stats(self):
        """mi_knn_assign_stats, of the last assign (or the last assign inside kmeans) on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_assign_stats(self._h, out))
        return {"candidates": out[0], "rows": out[1], "launches": out[2], "tiles": out[3]}

    def assign_multi(self, vectors: np.ndarray, m: int, max_dist: float = float("inf")):
        """Up to m labels per row (mi_knn_assign_multi): (labels [rows, m] uint32, dist [rows, m] f32) — for a live row what a
        table of the vectors answers to knn(row, m) without the entries whose distance is NaN or > max_dist, ids and distance
        bits; NO_LABEL / +inf behind a row's last hit and for a deleted row."""
        v = _f32(vectors).reshape(-1, self.dim)
        n = len(self)
        labels, dist = np.empty((n, int(m)), np.uint32), np.empty((n, int(m)), np.float32)
        check(lib().mi_knn_assign_multi(self._h, v.ctypes.data, v.shape[0], int(m), float(max_dist), labels.ctypes.data,
                                        dist.ctypes.data))
        return labels, dist

    def assign_multi_stats(self):
        """mi_knn_assign_multi_stats, of the last assign_multi on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_assign_multi_stats(self._h, out))
        return {"candidates": out[0], "hits": out[1], "launches": out[2], "tiles": out[3]}

    def knn_many(self, queries: np.ndarray, k: int):
        """The k <= 16 nearest live rows for each of many queries (mi_knn_search_many): (idx [nq, k] uint64, dist [nq, k] f32)
        — per query what knn(query, k) answers without the entries whose distance is NaN, ids and distance bits; NO_ID /
        +inf behind a query's last hit."""
        q = _f32(queries).reshape(-1, self.dim)
        idx, dist = np.empty((q.shape[0], int(k)), np.uint64), np.empty((q.shape[0], int(k)), np.float32)
        check(lib().mi_knn_search_many(self._h, q.ctypes.data, q.shape[0], int(k), idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def neighbors(self, k: int, first: int = 0, n: Optional[int] = None):
        """A slice of the kNN graph (mi_knn_neighbors): for the rows with ids first .. first + n - 1 (n = None: to the
        table's end) the k <= 15 nearest OTHER live rows, (idx [n, k] uint64, dist [n, k] f32); a deleted row gets NO_ID /
        +inf.  On a table with a base (set_base) the first id is the base."""
        if n is None:
            n = max(int(getattr(self, "_base_id", 0)) + len(self) - int(first), 0)
        idx, dist = np.empty((int(n), int(k)), np.uint64), np.empty((int(n), int(k)), np.float32)
        check(lib().mi_knn_neighbors(self._h, int(first), int(n), int(k), idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def search_many_stats(self):
        """mi_knn_search_many_stats, of the last knn_many / neighbors on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_search_many_stats(self._h, out))
        return {"candidates": out[0], "hits": out[1], "launches": out[2], "tiles": out[3]}

    def knn_many_where(self, queries: np.ndarray, k: int, **predicate):
        """knn_many among the rows a predicate keeps (mi_knn_search_many_where): (idx [nq, k], dist [nq, k], matched) — per
        query what knn_where(query, k, **predicate) answers without the entries whose distance is NaN, ids and distance bits.
        predicate: make_where's keywords (all_of / any_of / none_of / stamp / group); none = every live row, exactly
        knn_many.  matched = the qualifying rows."""
        return _many_where(lib().mi_knn_search_many_where, self._h, self.dim, queries, k, predicate)

    def neighbors_where(self, k: int, first: int = 0, n: Optional[int] = None, **predicate):
        """neighbors with the candidates narrowed (mi_knn_neighbors_where): every row of the slice asks, whether or not it
        qualifies itself; only the rows the predicate keeps may answer.  (idx [n, k], dist [n, k])."""
        if n is None:
            n = max(int(getattr(self, "_base_id", 0)) + len(self) - int(first), 0)
        idx, dist = np.empty((int(n), int(k)), np.uint64), np.empty((int(n), int(k)), np.float32)
        wp, _w = _where_or_null(predicate)
        check(lib().mi_knn_neighbors_where(self._h, int(first), int(n), int(k), wp, idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def propose_groups(self, k: int = 10, max_dist: float = float("inf"), ask_group=None, **voters_predicate) -> dict:
        """"Where do my unsorted pictures go?" — a k-nearest vote that carries the group column forward
        (mi_knn_propose_groups).  The askers are the live rows of ask_group (None: the rows without a group); the voters are
        the live rows of every other group that the predicate keeps (make_where's keywords; none: all of them).  Every asker
        hears its k <= 16 nearest voters within max_dist; the group with the most of them wins, the nearest among equal
        counts.  Returns {"group" [rows] uint32 (NO_GROUP: no proposal), "votes" (the winner's count), "heard" (voters
        heard), "dist" (the winner's nearest voter, +inf: none), "totals": {"askers", "proposed", "voters", "unanimous"}}.
        The column itself is not written: set_groups applies what the caller accepts."""
        n = len(self)
        group, votes, heard = (np.empty(max(n, 1), np.uint32) for _ in range(3))
        dist = np.empty(max(n, 1), np.float32)
        totals = (ctypes.c_uint64 * 4)()
        wp, _w = _where_or_null(voters_predicate)
        ask = int(NO_GROUP) if ask_group is None else int(ask_group)
        check(lib().mi_knn_propose_groups(self._h, int(k), float(max_dist), ask, wp, group.ctypes.data, votes.ctypes.data,
                                          heard.ctypes.data, dist.ctypes.data, totals))
        return {"group": group[:n], "votes": votes[:n], "heard": heard[:n], "dist": dist[:n],
                "totals": {"askers": totals[0], "proposed": totals[1], "voters": totals[2], "unanimous": totals[3]}}

    def propose_groups_stats(self):
        """mi_knn_propose_groups_stats, of the last propose_groups on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_propose_groups_stats(self._h, out))
        return {"candidates": out[0], "launches": out[1], "tiles": out[2], "strips": out[3]}

    def knn_diverse(self, reference: np.ndarray, k: int, min_gap: float, pool: Optional[int] = None, within=None):
        """The k best DISTINCT results (mi_knn_search_diverse): the list knn(reference, pool, within) walked in order, an
        entry within cosine distance min_gap (the bits near_pairs reports) of an earlier KEPT entry hidden behind it.
        Returns (idx [k] uint64, dist [k] f32, hidden [k] uint32 = look-alikes behind each kept entry, rep [pool] uint32 =
        per pool rank the slot it was kept in or hidden behind, NO_LABEL when left over or beyond the pool's end); NO_ID /
        +inf / 0 behind the last kept entry.  pool = None: min(4096, max(4 * k, 64))."""
        q = _f32(reference).reshape(-1)
        k = int(k)
        pool = min(4096, max(4 * k, 64)) if pool is None else int(pool)
        idx, dist = np.empty(max(k, 0), np.uint64), np.empty(max(k, 0), np.float32)
        hidden, rep = np.empty(max(k, 0), np.uint32), np.empty(max(pool, 0), np.uint32)
        ids, n_ids = None, 0
        if within is not None:
            a = _ids(within)
            n_ids = a.size
            if a.size == 0:   # an empty row set, not "the whole table"
                a = np.zeros(1, np.uint64)
            ids = a.ctypes.data
        check(lib().mi_knn_search_diverse(self._h, q.ctypes.data, k, pool, float(min_gap), ids, n_ids, idx.ctypes.data if k else None,
                                          dist.ctypes.data if k else None, hidden.ctypes.data if k else None,
                                          rep.ctypes.data if pool > 0 else None, None))
        return idx, dist, hidden, rep

    def knn_diverse_stats(self):
        """mi_knn_search_diverse_stats, of the last knn_diverse on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_search_diverse_stats(self._h, out))
        return {"pool": out[0], "candidates": out[1], "conflicts": out[2], "hidden": out[3]}

    def knn_compound(self, terms: np.ndarray, mode: str = "all", without=None, without_within=None, k: int = 10, within=None,
                     term_dist: bool = False):
        """All-of / any-of / none-of terms in one exact pass (mi_knn_search_compound).  terms [n_pos, dim]: mode "all" scores a
        row by its LARGEST distance to them (near every term), "any" by its smallest (near at least one); without [n_neg, dim]
        with without_within (one cosine distance per negative term, or one for all): a row within that distance of a negative
        term is excluded.  Every per-term distance has the bits knn(term) reports.  within: ids, as for knn().  Returns
        (idx [k] uint64, score [k] f32) ascending by (score, id), NO_ID / +inf behind the last hit; term_dist=True adds
        [k, n_pos + n_neg] f32: the result rows' distances to every term, positives first.  n_pos + n_neg <= 8, k <= 4096."""
        pos, code, neg, w, n_neg = _compound_args(self.dim, terms, mode, without, without_within)
        k = int(k)
        T = pos.shape[0] + n_neg
        idx, dist = np.empty(max(k, 1), np.uint64), np.empty(max(k, 1), np.float32)
        td = np.empty((max(k, 1), max(T, 1)), np.float32) if term_dist else None
        ids, n_ids, _keep = _among(within)
        check(lib().mi_knn_search_compound(self._h, pos.ctypes.data if pos.size else None, pos.shape[0], code,
                                           neg.ctypes.data if n_neg else None, w.ctypes.data if n_neg else None, n_neg, k, ids, n_ids,
                                           idx.ctypes.data, dist.ctypes.data, td.ctypes.data if term_dist else None))
        return (idx[:k], dist[:k], td[:k, :T]) if term_dist else (idx[:k], dist[:k])

    def knn_compound_stats(self):
        """mi_knn_search_compound_stats, of the last knn_compound on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_search_compound_stats(self._h, out))
        return {"scanned": out[0], "excluded": out[1], "nan": out[2], "results": out[3]}

    def set_groups(self, groups, ids=None):
        """The group column (mi_knn_set_groups): groups[i] for row ids[i], ids=None: for the first len(groups) rows.  A group id
        is < 2^24 or NO_GROUP (the row is a group of its own); appended rows start as NO_GROUP; the column is not saved."""
        _set_groups(lib().mi_knn_set_groups, self._h, groups, ids)

    def groups(self, ids=None) -> np.ndarray:
        """the group of the rows `ids` (None: of every row) — NO_GROUP where none was set"""
        return _get_groups(lib().mi_knn_get_groups, self._h, ids, len(self))

    def groups_info(self) -> dict:
        info = (ctypes.c_uint64 * 2)()
        check(lib().mi_knn_groups_info(self._h, info))
        return {"n_groups": info[0], "rows": info[1]}

    def knn_grouped(self, reference: np.ndarray, k: int = 10, max_dist: float = float("inf"), within=None, facets: bool = False):
        """The best hit per group (mi_knn_search_grouped): of every group the row nearest to `reference` within max_dist, the k
        nearest of those; rows without a group stand for themselves.  within: None or the ids to search among.  Returns
        (idx [k], dist [k], group [k], members [k], totals) with members = the group's rows within max_dist and totals =
        {"groups": representatives within max_dist, "window", "beyond", "nan"}; NO_ID / +inf / NO_GROUP / 0 behind the last
        hit.  facets=True appends the array of every group's count.  Exact over the whole table; k <= 4096."""
        return _grouped_call(lib().mi_knn_search_grouped, self._h, self.dim, (), reference, k, max_dist,
                             self.groups_info()["n_groups"] if facets else 0, facets, within=within)

    def set_attrs(self, ids, tags=None, stamps=None):
        """The attribute columns (mi_knn_set_attrs): tags[i] (64 flags, uint64) and stamps[i] (an ordered int64: a capture time,
        a rating) for row ids[i]; None keeps that column.  Rows start with 0 / 0; the columns grow with the table and are not
        saved (get_attrs() reads them back).  An id that is no row raises and writes nothing."""
        _set_attrs(lib().mi_knn_set_attrs, self._h, ids, tags, stamps)

    def get_attrs(self, ids=None):
        """(tags, stamps) of the rows `ids` (None: of every row) — 0 / 0 where none was set"""
        first = int(getattr(self, "_base_id", 0))
        return _get_attrs(lib().mi_knn_get_attrs, self._h, np.arange(first, first + len(self), dtype=np.uint64) if ids is None else ids, 0)

    def count_where(self, all_of=0, any_of=0, none_of=0, stamp=(None, None), group=None) -> int:
        """how many live rows the predicate keeps (mi_knn_count_where; make_where for the arguments)"""
        return _count_where(lib().mi_knn_count_where, self._h, make_where(all_of, any_of, none_of, stamp, group))

    def rows_where(self, all_of=0, any_of=0, none_of=0, stamp=(None, None), group=None) -> np.ndarray:
        """the ids of the live rows the predicate keeps, ascending (mi_knn_rows_where)"""
        w = make_where(all_of, any_of, none_of, stamp, group)
        n = ctypes.c_uint64()
        ids = np.empty(max(len(self), 1), np.uint64)
        check(lib().mi_knn_rows_where(self._h, ctypes.byref(w), ids.ctypes.data, len(self), ctypes.byref(n)))
        return ids[:n.value].copy()

    def knn_where(self, reference: np.ndarray, k: int = 10, all_of=0, any_of=0, none_of=0, stamp=(None, None), group=None):
        """The k nearest among the live rows a predicate keeps (mi_knn_search_where): "like this, among my favourites, taken
        2019-2021, not hidden, in this group".  The predicate runs on the device over the attribute columns — no id list.
        Returns (idx, dist, matched): bit for bit what knn(reference, k, within=rows_where(...)) returns, and the number of
        qualifying rows; NO_ID / +inf behind the last hit; k <= 4096."""
        return _search_where(lib().mi_knn_search_where, self._h, self.dim, reference, k, make_where(all_of, any_of, none_of, stamp, group))

    def knn_page(self, reference: np.ndarray, k: int = 100, after=None, max_dist: float = float("inf"), within=None):
        """The k nearest rows AFTER a cursor and WITHIN a distance (mi_knn_search_page).  after: None (from the start) or the
        (dist, id) of the previous page's last hit — pass back what came out, the bits of dist matter; its row may have been
        deleted since.  max_dist: inclusive bound on the cosine distance.  within: ids, as for knn().  Returns (idx [k] uint64,
        dist [k] f32, counts, next): ascending by (distance, id), NO_ID / +inf behind the last hit, NaN distances never
        returned; counts = {"before", "window", "beyond", "nan"} of the candidates (they add up to their number); next = the
        cursor for the following page, None when this page came back short.  k <= 4096."""
        return _page_call(lib().mi_knn_search_page, self._h, self.dim, (), reference, k, after, max_dist, within=within)

    def knn_ordered(self, reference: np.ndarray, k: int = 100, max_dist: float = float("inf"), descending: bool = False, after=None,
                    **predicate):
        """The rows within max_dist of the reference in the order of their stamps (mi_knn_search_ordered): ascending, or newest
        first with descending=True; equal stamps by ascending id.  after: None (from the start) or the (stamp, id) of the
        previous page's last hit — its row may have been deleted since.  predicate: the keyword arguments of make_where (none:
        every live row).  Returns (idx, dist, stamps, counts): the hits in order, NO_ID / +inf / 0 behind them, and counts =
        {"within", "before", "beyond", "nan"} ("101-200 of within").  k <= 4096."""
        return _ordered_call(lib().mi_knn_search_ordered, self._h, self.dim, (), reference, k, max_dist, descending, after, predicate)

    def timeline(self, reference: np.ndarray, k: int = 100, max_dist: float = float("inf"), descending: bool = False, **predicate):
        """knn_ordered after knn_ordered until one comes back short: yields (idx, dist, stamps, counts) with the padding cut off.
        Rows appended or deleted between two pages are honoured as they stand when each page is asked for."""
        return _timeline(lambda after: self.knn_ordered(reference, k, max_dist, descending, after, **predicate), k)

    def stamp_histogram(self, reference: np.ndarray, edges, max_dist: float = float("inf"), **predicate) -> np.ndarray:
        """The timeline facet (mi_knn_stamp_histogram): hist[b] = the rows within max_dist (and the predicate) with exactly b of
        the strictly ascending edges <= stamp; [len(edges) + 1] uint64, summing to knn_ordered's counts["within"]."""
        return _stamp_histogram(lib().mi_knn_stamp_histogram, self._h, self.dim, (), reference, edges, max_dist, predicate)

    def pages(self, reference: np.ndarray, k: int = 100, max_dist: float = float("inf"), within=None):
        """knn_page after knn_page until one comes back short: yields (idx, dist, counts) with the padding cut off.  Rows
        appended or deleted between two pages are honoured as they stand when each page is asked for."""
        after = None
        while True:
            idx, dist, counts, after = self.knn_page(reference, k, after, max_dist, within)
            n = int((idx != NO_ID).sum())
            if n:
                yield idx[:n], dist[:n], counts
            if after is None:
                return

    def kmeans_seed(self, k: int, seed: int = 0, among=None) -> dict:
        """k-means++ seeding on the device (mi_knn_kmeans_seed): k rows, each drawn with probability proportional to its
        cosine distance from the nearest row drawn so far; exact and deterministic in `seed`.  among: ids (any order,
        duplicates allowed) to draw from, None = every live row.  Returns dict(rows [k] uint64 in pick order, centroids
        [k, dim] = those rows' values, potential = the k-means++ potential of the seeds)."""
        k = int(k)
        rows, cent = np.empty(max(k, 0), np.uint64), np.empty((max(k, 0), self.dim), np.float32)
        pot = ctypes.c_double()
        ids, n_ids = None, 0
        if among is not None:
            a = _ids(among)
            n_ids = a.size
            if a.size == 0:   # an empty set of candidates, not "every row"
                a = np.zeros(1, np.uint64)
            ids = a.ctypes.data
        check(lib().mi_knn_kmeans_seed(self._h, k, int(seed), ids, n_ids, rows.ctypes.data if k else None,
                                       cent.ctypes.data if k else None, ctypes.byref(pot)))
        return {"rows": rows, "centroids": cent, "potential": pot.value}

    def kmeans_seed_stats(self):
        """mi_knn_kmeans_seed_stats, of the last kmeans_seed on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_kmeans_seed_stats(self._h, out))
        return {"candidates": out[0], "passes": out[1], "fallbacks": out[2]}

    def kmeans(self, k_or_centroids, max_iters: int = 20, seed: int = 0, init: str = "uniform", sample: Optional[int] = None,
               fixed_sum: Optional[bool] = None) -> dict:
        """Spherical k-means over the live rows (mi_knn_kmeans).  fixed_sum: None leaves the table's option
        "kmeans_fixed_sum" as it is; a bool sets it for this call (True: the update on exact integer sums, what
        ShardedTable.kmeans computes) and restores what set_option last set.  k_or_centroids: the initial centroids [C, dim], or an int
        k.  init = "uniform": k distinct live rows picked with np.random.default_rng(seed); init = "kmeans++": the rows
        kmeans_seed(k, seed) picks — among all live rows, or, where there are more than `sample` of them (None =
        max(64 k, 16 384)), among a seeded uniform subset of that size.  Returns dict(centroids, labels, dist, iters,
        changed, objective); labels / dist are exactly assign(centroids)."""
        if init not in ("uniform", "kmeans++"):
            raise ValueError(f'init = {init!r}: "uniform" or "kmeans++"')
        if isinstance(k_or_centroids, (int, np.integer)) and init == "kmeans++":
            k = int(k_or_centroids)
            sample = max(64 * k, 16384) if sample is None else int(sample)
            base = np.uint64(getattr(self, "_base_id", 0))
            live = np.setdiff1d(np.arange(len(self), dtype=np.uint64) + base, self.deleted())
            among = np.sort(np.random.default_rng(seed).choice(live, size=sample, replace=False)) if live.size > sample else None
            cent = self.kmeans_seed(k, seed, among)["centroids"]
        elif isinstance(k_or_centroids, (int, np.integer)):
            rows = initial_centroid_rows(len(self), self.deleted(), int(k_or_centroids), seed)
            cent = np.concatenate([self.rows(int(r), 1) for r in rows]) if rows.size else np.empty((0, self.dim), np.float32)
        else:
            cent = np.array(k_or_centroids, dtype=np.float32, order="C").reshape(-1, self.dim)
        n = len(self)
        labels, dist = np.empty(n, np.uint32), np.empty(n, np.float32)
        iters, changed, obj = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_double()
        before = int(getattr(self, "_options", {}).get("kmeans_fixed_sum", 0))
        if fixed_sum is not None:
            check(lib().mi_knn_set_option(self._h, b"kmeans_fixed_sum", int(bool(fixed_sum))))
        try:
            check(lib().mi_knn_kmeans(self._h, cent.ctypes.data, cent.shape[0], int(max_iters), labels.ctypes.data, dist.ctypes.data,
                                      ctypes.byref(iters), ctypes.byref(changed), ctypes.byref(obj)))
        finally:
            if fixed_sum is not None:
                check(lib().mi_knn_set_option(self._h, b"kmeans_fixed_sum", before))
        return {"centroids": cent, "labels": labels, "dist": dist, "iters": iters.value, "changed": changed.value,
                "objective": obj.value}

    def summarize(self, labels=None, n_groups: Optional[int] = None) -> dict:
        """What every group looks like (mi_knn_summarize).  labels: one per local row (kmeans / assign labels, dbscan's dense
        labels with -1 for noise, duplicate components, anything; NO_LABEL or any value >= n_groups = belongs to nothing), or
        None: the table's group column, read on the device.  n_groups defaults to the largest label that is not NO_LABEL,
        plus one, or to groups_info()["n_groups"].  A member is a live row with a label < n_groups whose distance to itself
        is a number.  Returns dict(centroids [C, dim] = the mean of x / |x| over the members, summed in kmeans' order and
        bit-identical to its update; count [C]; cover / cover_dist [C] = the member nearest to the centroid (the group's exact
        medoid for unit vectors), NO_ID / +inf for an empty group; odd / odd_dist [C] = the farthest member; measured [C] =
        members with a non-NaN distance; spread [C] = their distances summed as integers of 2^-30; mean_dist [C] float64 =
        spread / measured * 2^-30, NaN where nothing was measured; dist [rows] = a member's distance to its centroid with
        assign's bits, NaN for an unusable row of a group, +inf otherwise; totals {"members", "outside", "unusable",
        "groups"}).  cover and odd are ids; every array indexed by row is indexed by local row."""
        return _summarize_call(lib().mi_knn_summarize, self, labels, n_groups)

    def summarize_stats(self) -> dict:
        """mi_knn_summarize_stats, of the last summarize on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_summarize_stats(self._h, out))
        return {"segments": out[0], "workgroups": out[1], "rows": out[2]}

    def representatives(self, labels=None, n_groups: Optional[int] = None, m: int = 9, min_gap: float = float("-inf"),
                        start="cover") -> dict:
        """m pictures that span every group (mi_knn_representatives): farthest-first traversal of every group at once —
        start at one member, then repeatedly take the member farthest from everything taken so far.  labels / n_groups as
        summarize.  start: "cover" = summarize's cover of every group (one summarize call first), "first" = the member with
        the lowest id, or an array [n_groups] of ids.  A pick is made only while its distance to the nearest earlier pick
        is above min_gap.  Returns dict(rows [C, m] = the picked ids in pick order, NO_ID behind the last; gap [C, m] = a
        pick's distance to the nearest earlier pick, non-increasing from pick 1 on, +inf for pick 0 and the padding;
        n_picked [C]; reach [C] = every measured member lies within this distance of a pick; rep [rows] = the index of the
        pick that stands for a row, NO_LABEL for a row that is no member; rep_dist [rows] = its distance to that pick;
        stands_for [C, m] = how many members a pick stands for (itself included): the "+37 similar" beside a thumbnail;
        totals {"members", "groups", "picks", "rounds"})."""
        n = len(self)
        lab = None
        if labels is not None:
            lab = np.ascontiguousarray(np.asarray(labels).reshape(-1).astype(np.uint32))
            if lab.size != n:
                raise ValueError(f"{lab.size} labels for {n} rows")
            if n_groups is None:
                has = lab[lab != NO_LABEL]
                n_groups = int(has.max()) + 1 if has.size else 1
        elif n_groups is None:
            n_groups = max(int(self.groups_info()["n_groups"]), 1)
        C, m = int(n_groups), int(m)
        first = None
        if isinstance(start, str):
            if start not in ("cover", "first"):
                raise ValueError('start is "cover", "first" or an array of ids')
            if start == "cover" and n and 1 <= C <= 65536:
                first = np.ascontiguousarray(self.summarize(lab, C)["cover"], np.uint64)
        else:
            first = np.ascontiguousarray(np.asarray(start).reshape(-1).astype(np.uint64))
            if first.size != C:
                raise ValueError(f"{first.size} start ids for {C} groups")
        cm = max(C, 0) * max(m, 0)
        rows, gap = np.empty(cm, np.uint64), np.empty(cm, np.float32)
        n_picked, reach = np.empty(max(C, 0), np.uint32), np.empty(max(C, 0), np.float32)
        rep, rep_dist = np.empty(n, np.uint32), np.empty(n, np.float32)
        totals = np.zeros(4, np.uint64)
        check(lib().mi_knn_representatives(self._h, lab.ctypes.data if lab is not None and n else None, C, m, float(min_gap),
                                           first.ctypes.data if first is not None else None, rows.ctypes.data, gap.ctypes.data,
                                           n_picked.ctypes.data, reach.ctypes.data, rep.ctypes.data if n else None,
                                           rep_dist.ctypes.data if n else None, totals.ctypes.data))
        group = lab if lab is not None else (self.groups() if n else np.zeros(0, np.uint32))
        has = rep != NO_LABEL
        stands_for = np.bincount(group[has].astype(np.int64) * m + rep[has].astype(np.int64), minlength=C * m)
        return {"rows": rows.reshape(C, m), "gap": gap.reshape(C, m), "n_picked": n_picked, "reach": reach, "rep": rep,
                "rep_dist": rep_dist, "stands_for": stands_for.astype(np.uint64).reshape(C, m),
                "totals": dict(zip(("members", "groups", "picks", "rounds"), (int(v) for v in totals)))}

    def representatives_of(self, ids, m: int = 9, min_gap: float = float("-inf"), start="cover") -> dict:
        """representatives of ONE group made of the rows `ids` (the highlights of a result list, of a DBSCAN theme, ...):
        the same dict with one group; start as there (an id, not an array, where it is given)."""
        ids = np.asarray(ids).reshape(-1).astype(np.uint64)
        n = len(self)
        local = ids - np.uint64(getattr(self, "_base_id", 0))
        if ids.size and (int(ids.min()) < int(getattr(self, "_base_id", 0)) or int(local.max()) >= n):
            raise ValueError("an id that is not a row of the table")
        labels = np.full(n, NO_LABEL, np.uint32)
        labels[local.astype(np.int64)] = 0
        if not isinstance(start, str):
            start = [int(start)]
        return self.representatives(labels, 1, m, min_gap, start)

    def representatives_stats(self) -> dict:
        """mi_knn_representatives_stats, of the last representatives on this table"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_representatives_stats(self._h, out))
        return {"rounds": out[0], "segments": out[1], "rows_last_round": out[2]}


def _summarize_call(fn, table, labels, n_groups) -> dict:
    """EmbeddingTable.summarize / ShardedTable.summarize: fn = mi_knn_summarize or mi_knn_sharded_summarize"""
    n = len(table)
    lab = None
    if labels is not None:
        lab = np.ascontiguousarray(np.asarray(labels).reshape(-1).astype(np.uint32))
        if lab.size != n:
            raise ValueError(f"{lab.size} labels for {n} rows")
        if n_groups is None:
            has = lab[lab != NO_LABEL]
            n_groups = int(has.max()) + 1 if has.size else 1
    elif n_groups is None:
        n_groups = max(int(table.groups_info()["n_groups"]), 1)
    C = int(n_groups)
    m = max(C, 0)
    cent = np.empty((m, table.dim), np.float32)
    count, cover, odd, measured, spread = (np.empty(m, np.uint64) for _ in range(5))
    cover_dist, odd_dist, dist = np.empty(m, np.float32), np.empty(m, np.float32), np.empty(n, np.float32)
    totals = np.zeros(4, np.uint64)
    check(fn(table._h, lab.ctypes.data if lab is not None and n else None, C, cent.ctypes.data, count.ctypes.data,
             cover.ctypes.data, cover_dist.ctypes.data, odd.ctypes.data, odd_dist.ctypes.data, measured.ctypes.data,
             spread.ctypes.data, dist.ctypes.data if n else None, totals.ctypes.data))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(measured > 0, spread.astype(np.float64) / measured.astype(np.float64) * 2.0 ** -30, np.nan)
    return {"centroids": cent, "count": count, "cover": cover, "cover_dist": cover_dist, "odd": odd, "odd_dist": odd_dist,
            "measured": measured, "spread": spread, "mean_dist": mean, "dist": dist,
            "totals": dict(zip(("members", "outside", "unusable", "groups"), (int(v) for v in totals)))}


def dist_keys(dist) -> np.ndarray:
    """the search's 32-bit order of distances: ascending with the distance, -0 in front of +0, every NaN last"""
    d = np.ascontiguousarray(np.asarray(dist, np.float32).reshape(-1))
    b = d.view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(d)] = np.uint32(0xFFFFFFFF)
    return key


def typical_order(labels, dist, n_groups: Optional[int] = None) -> list:
    """"Most typical first": labels [rows] and the dist [rows] summarize returned -> per group 0 .. C - 1 its members' local rows
    ordered by (distance key, row): the cover first, NaN distances last.  Rows whose dist is +inf (no member: deleted,
    unlabelled) are left out."""
    lab = np.asarray(labels).reshape(-1).astype(np.uint32)
    d = np.asarray(dist, np.float32).reshape(-1)
    if n_groups is None:
        has = lab[lab != NO_LABEL]
        n_groups = int(has.max()) + 1 if has.size else 0
    rows = np.flatnonzero((lab < n_groups) & ~np.isposinf(d))
    order = rows[np.lexsort((rows, dist_keys(d[rows]), lab[rows]))]
    cuts = np.searchsorted(lab[order], np.arange(n_groups + 1))
    return [order[cuts[c]:cuts[c + 1]] for c in range(n_groups)]


def drop_self(idx: np.ndarray, dist: np.ndarray, self_ids) -> tuple:
    """knn_many(rows, k + 1) -> the k nearest OTHER rows: from row i of idx / dist [n, k + 1] the entry whose id is
    self_ids[i] is removed, or, where that is absent (only padding; k + 1 or more exact copies of the row at lower ids),
    the last entry.  Returns (idx [n, k], dist [n, k])."""
    idx = np.asarray(idx, np.uint64)
    dist = np.asarray(dist, np.float32)
    n, m = idx.shape
    own = idx == np.asarray(self_ids, np.uint64).reshape(n, 1)
    drop = np.where(own.any(axis=1), own.argmax(axis=1), m - 1)
    keep = np.arange(m)[None, :] != drop[:, None]
    return idx[keep].reshape(n, m - 1), dist[keep].reshape(n, m - 1)


def rows_of_labels(labels: np.ndarray, C: int) -> list:
    """"Show me everything tagged X": labels [rows, m] (or [rows]) as assign_multi / assign report them -> per label
    0 .. C - 1 the ascending ids (uint64) of the rows that carry it; NO_LABEL entries carry nothing."""
    lab = np.asarray(labels, np.uint32)
    lab = lab.reshape(lab.shape[0], -1) if lab.size else lab.reshape(0, 1)
    if np.any((lab >= C) & (lab != NO_LABEL)):
        raise ValueError(f"a label beyond C = {C}")
    rows = np.repeat(np.arange(lab.shape[0], dtype=np.uint64), lab.shape[1])
    flat = lab.reshape(-1)
    keep = flat != NO_LABEL
    rows, flat = rows[keep], flat[keep]
    order = np.lexsort((rows, flat))
    rows, flat = rows[order], flat[order]
    cuts = np.searchsorted(flat, np.arange(C + 1))
    return [rows[cuts[c]:cuts[c + 1]] for c in range(C)]


def initial_centroid_rows(n_rows: int, deleted, k: int, seed: int = 0) -> np.ndarray:
    """k distinct live rows of a table of n_rows rows, ascending: the seeded choice kmeans(k) starts from"""
    live = np.setdiff1d(np.arange(n_rows, dtype=np.uint64), _ids(deleted), assume_unique=False)
    if not 1 <= k <= live.size:
        raise ValueError(f"k = {k} initial centroids from {live.size} live rows")
    return np.sort(np.random.default_rng(seed).choice(live, size=k, replace=False))


def clusters_of(labels, keys) -> list:
    """labels[i] of keys[i] (NO_LABEL = leave out) -> lists of keys, one per non-empty cluster: the largest first, equal
    sizes by label; inside a list the keys keep their order"""
    by = {}
    for lab, key in zip(labels, keys):
        if int(lab) != int(NO_LABEL):
            by.setdefault(int(lab), []).append(key)
    return [by[lab] for lab in sorted(by, key=lambda c: (-len(by[c]), c))]


def dense_labels(cluster) -> np.ndarray:
    """cluster ids as dbscan reports them (NO_ID: none) -> int64 labels 0 .. C - 1 in the order of the ids, -1 where none"""
    cluster = np.asarray(cluster, np.uint64).reshape(-1)
    labels = np.full(cluster.size, -1, np.int64)
    has = cluster != NO_ID
    labels[has] = np.searchsorted(np.unique(cluster[has]), cluster[has])
    return labels


LEVELS_MAX = 8   # MI_KNN_LEVELS_MAX


def _levels(max_dists) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(max_dists, dtype=np.float32).reshape(-1))


def dbscan_levels_tree(cluster, counts, min_pts: int):
    """The tree between the levels of a dbscan_levels result (mi_dbscan_levels_tree, host only): cluster, counts [L, rows] ->
    (level uint32, child uint64, parent uint64), one entry per cluster of every level l < L - 1, ascending by (level, child
    cluster id); parent = the cluster id at level l + 1 that holds the child's core rows."""
    cluster = np.ascontiguousarray(np.asarray(cluster, np.uint64))
    counts = np.ascontiguousarray(np.asarray(counts, np.uint32))
    if cluster.ndim != 2 or cluster.shape != counts.shape:
        raise ValueError(f"cluster {cluster.shape} and counts {counts.shape} must both be [levels, rows]")
    L, n = cluster.shape
    pad = np.zeros(1, np.uint64)   # (never a null pointer for an empty table)
    pc, pd = (cluster.ctypes.data, counts.ctypes.data) if cluster.size else (pad.ctypes.data, pad.ctypes.data)
    n_edges = ctypes.c_uint64()
    check(lib().mi_dbscan_levels_tree(pc, pd, n, L, int(min_pts), None, None, None, 0, ctypes.byref(n_edges)))
    m = n_edges.value
    level, child, parent = np.empty(m, np.uint32), np.empty(m, np.uint64), np.empty(m, np.uint64)
    if m:
        check(lib().mi_dbscan_levels_tree(pc, pd, n, L, int(min_pts), level.ctypes.data, child.ctypes.data, parent.ctypes.data, m,
                                          ctypes.byref(n_edges)))
    return level, child, parent


def _groups(ids: np.ndarray, starts: np.ndarray) -> list:
    return [ids[int(starts[g]):int(starts[g + 1])] for g in range(len(starts) - 1)]


def pairs_to_groups(a, b) -> list:
    """Pairs -> groups (mi_pairs_to_groups: connected components): arrays of ids, ascending inside a group, the groups
    ordered by their smallest id."""
    a, b = _ids(a), _ids(b)
    if a.size != b.size:
        raise ValueError(f"{a.size} first ids for {b.size} second ids")
    n_ids, n_groups = ctypes.c_uint64(), ctypes.c_uint64()
    pa, pb = (a.ctypes.data, b.ctypes.data) if a.size else (None, None)
    check(lib().mi_pairs_to_groups(pa, pb, a.size, None, 0, None, 0, ctypes.byref(n_ids), ctypes.byref(n_groups)))
    ids, starts = np.empty(n_ids.value, np.uint64), np.empty(n_groups.value + 1, np.uint64)
    check(lib().mi_pairs_to_groups(pa, pb, a.size, ids.ctypes.data if ids.size else None, ids.size, starts.ctypes.data, starts.size,
                                   ctypes.byref(n_ids), ctypes.byref(n_groups)))
    return _groups(ids, starts)


def _ids(ids) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(ids, dtype=np.uint64).reshape(-1))


def _delete(fn, h, ids) -> int:
    a = _ids(ids)
    newly = ctypes.c_uint64()
    check(fn(h, a.ctypes.data if a.size else None, a.size, ctypes.byref(newly)))
    return newly.value


def _deleted(fn, h) -> np.ndarray:
    n = ctypes.c_uint64()
    check(fn(h, None, 0, ctypes.byref(n)))
    out = np.empty(n.value, np.uint64)
    if n.value:
        check(fn(h, out.ctypes.data, n.value, ctypes.byref(n)))
    return out


def _compact(fn, h, rows: int) -> dict:
    new_ids = np.empty(rows, dtype=np.uint64)
    removed = ctypes.c_uint64()
    check(fn(h, new_ids.ctypes.data if rows else None, rows, ctypes.byref(removed)))
    return {"removed": removed.value, "new_ids": new_ids}


class PinnedBuffer:
    """Page-locked host memory (mi_host_alloc) viewed as a numpy array: upload buffers of the
    fused pipeline (asynchronous H2D needs pinned memory)."""

    def __init__(self, shape, dtype=np.float32):
        self.shape = tuple(int(x) for x in shape)
        self.dtype = np.dtype(dtype)
        nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self._p = c_vp()
        check(lib().mi_host_alloc(nbytes, ctypes.byref(self._p)))
        buf = (ctypes.c_char * nbytes).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=self.dtype).reshape(self.shape)

    def close(self):
        if getattr(self, "_p", None) and self._p.value:
            self.array = None
            lib().mi_host_free(self._p)
            self._p = c_vp()

    __del__ = close


class Pipeline:
    """The scan-loop body (clip.rs:107-137) and the query (search.rs:70-86) fused on HIP streams
    (mi_pipeline_*): `ingest` uploads, embeds and inserts a chunk without a readback; `query`
    scans on a second stream under the next chunk's forward; `sync` delivers the results."""

    def __init__(self, model, table):
        """model: one image tower and table: an EmbeddingTable on its GPU — or, for ONE process over several GPUs
        (mi_pipeline_create_sharded), a list of towers, models[s] on the device of shard s of a ShardedTable."""
        self._h = c_vp()
        self.model, self.table = model, table  # borrowed: keep them alive
        self._pending = []
        if isinstance(table, ShardedTable):
            models = list(model) if isinstance(model, (list, tuple)) else [model] * table.info()["shards"]
            arr = (c_vp * len(models))(*[m._h for m in models])
            check(lib().mi_pipeline_create_sharded(arr, len(models), table._h, ctypes.byref(self._h)))
        else:
            check(lib().mi_pipeline_create(model._h, table._h, ctypes.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().mi_pipeline_free(self._h)
            self._h = c_vp()
            self._pending = []

    __del__ = close

    def ingest(self, nchw: np.ndarray) -> int:
        """nchw: [n,3,H,W] f32 (a PinnedBuffer.array makes the upload asynchronous; the array must stay
        untouched until the next ingest / sync returns).  Returns the id of the chunk's first row."""
        x = nchw if (nchw.dtype == np.float32 and nchw.flags.c_contiguous) else np.ascontiguousarray(nchw, np.float32)
        first = ctypes.c_uint64()
        check(lib().mi_pipeline_ingest(self._h, x.ctypes.data, x.shape[0], ctypes.byref(first)))
        return first.value

    def query(self, reference: np.ndarray, k: int = K_REFERENCE):
        """Enqueue `embedding <|k|> $reference`; returns (ids, distances) arrays that are filled by sync()."""
        q = _f32(reference).reshape(-1)
        idx = np.full(k, NO_ID, np.uint64)
        dist = np.full(k, np.inf, np.float32)
        check(lib().mi_pipeline_query(self._h, q.ctypes.data, k, idx.ctypes.data, dist.ctypes.data))
        self._pending.append((idx, dist))  # the library writes into them at sync: keep them alive
        return idx, dist

    def query_device(self, reference: np.ndarray, k: int, d_idx: int, d_dist: int, consumer_stream: int = 0):
        """The same query, its k results left on the device at d_idx [k] uint64 / d_dist [k] f32 (mi_pipeline_query_device);
        `consumer_stream` (a raw hipStream_t) is made to wait for them: the list a sharded search feeds to the all-gather."""
        q = _f32(reference).reshape(-1)
        check(lib().mi_pipeline_query_device(self._h, q.ctypes.data, k, d_idx, d_dist, consumer_stream))

    def sync(self):
        check(lib().mi_pipeline_sync(self._h))
        self._pending = []

    def drain(self, leave_pending: int = 0):
        """Deliver finished queries (oldest first) until at most `leave_pending` remain pending."""
        check(lib().mi_pipeline_drain(self._h, leave_pending))
        if leave_pending == 0:
            self._pending = []
        else:
            self._pending = self._pending[-leave_pending:]

    def stats(self, reset: bool = False):
        """(forwards, ms in forwards, scans, ms in scans) measured by events on the pipeline's streams."""
        out = (ctypes.c_double * 4)()
        check(lib().mi_pipeline_stats(self._h, out, 1 if reset else 0))
        return tuple(out)


def merge_candidates(idx_lists: np.ndarray, dist_lists: np.ndarray, k: int):
    """Global top-k of `lists` per-shard candidate lists (same ordering rule)."""
    i = np.ascontiguousarray(idx_lists, np.uint64).reshape(-1)
    d = np.ascontiguousarray(dist_lists, np.float32).reshape(-1)
    assert i.size == d.size and i.size % k == 0
    idx = np.empty(k, np.uint64)
    dist = np.empty(k, np.float32)
    check(lib().mi_knn_merge(i.ctypes.data, d.ctypes.data, i.size // k, k, idx.ctypes.data, dist.ctypes.data))
    return idx, dist


def merge_candidates_device(device: int, d_idx_in: int, d_dist_in: int, lists: int, nq: int, k: int, d_idx: int, d_dist: int,
                            stream: int = 0):
    """mi_knn_merge_device: the merge of the all-gathered [lists][nq][k] lists on the device, asynchronous on `stream`."""
    check(lib().mi_knn_merge_device(device, d_idx_in, d_dist_in, lists, nq, k, d_idx, d_dist, stream))


class ShardedTable:
    """`image.embedding` row-sharded over the GPUs of one node inside ONE process (mi_knn_sharded_*): the
    reference's one-handle, one-search-at-a-time shape (main.rs:30-35, search.rs:26) for BASELINE config 5.
    Same `insert` / `knn` surface as EmbeddingTable; ids are global insertion ordinals."""

    TRANSPORTS = {0: "single shard", 1: "device copies", 2: "rccl all-gather"}

    def __init__(self, dim: int = 768, devices: Sequence[int] = (0,), block_rows: int = 0):
        self._h = c_vp()
        self.dim = dim
        devs = (ctypes.c_int * len(devices))(*devices)
        check(lib().mi_knn_sharded_create(dim, devs, len(devices), block_rows, ctypes.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().mi_knn_sharded_free(self._h)
            self._h = c_vp()

    __del__ = close

    def info(self):
        rows, n, blk, tr = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
        check(lib().mi_knn_sharded_info(self._h, ctypes.byref(rows), ctypes.byref(n), ctypes.byref(blk), ctypes.byref(tr)))
        return {"rows": rows.value, "shards": n.value, "block_rows": blk.value, "transport": self.TRANSPORTS[tr.value]}

    def stats(self):
        """what the exchange step has executed so far (mi_knn_sharded_stats)"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_sharded_stats(self._h, out))
        return dict(zip(("searches", "collectives", "copies", "merges"), (int(v) for v in out)))

    def __len__(self) -> int:
        return self.info()["rows"]

    def set_option(self, key: str, value: int):
        check(lib().mi_knn_sharded_set_option(self._h, key.encode(), int(value)))

    def reserve(self, rows: int):
        check(lib().mi_knn_sharded_reserve(self._h, rows))

    def insert(self, embeddings: np.ndarray) -> int:
        e = _f32(embeddings).reshape(-1, self.dim)
        first = ctypes.c_uint64()
        check(lib().mi_knn_sharded_append(self._h, e.ctypes.data, e.shape[0], ctypes.byref(first)))
        return first.value

    def insert_synthetic(self, seed: int, first_row: int, n: int):
        check(lib().mi_knn_sharded_append_synthetic(self._h, seed, first_row, n))

    def insert_device(self, d_ptr: int, n: int, src_device: int = 0, stream: int = 0) -> int:
        """rows already in device memory on `src_device`: routed to their shards device to device (mi_knn_sharded_append_device)"""
        first = ctypes.c_uint64()
        check(lib().mi_knn_sharded_append_device(self._h, d_ptr, n, src_device, stream, ctypes.byref(first)))
        return first.value

    def shard_rows(self, s: int) -> int:
        h = lib().mi_knn_sharded_shard(self._h, s)
        n = ctypes.c_uint64()
        check(lib().mi_knn_size(c_vp(h), ctypes.byref(n)))
        return n.value

    def rows(self, first: int, n: int) -> np.ndarray:
        out = np.empty((n, self.dim), np.float32)
        check(lib().mi_knn_sharded_get_rows(self._h, first, n, out.ctypes.data))
        return out

    def knn_async(self, reference: np.ndarray, k: int = K_REFERENCE):
        """mi_knn_sharded_search_async: returns (ids, distances) arrays that are filled by sync()."""
        q = _f32(reference).reshape(-1, self.dim)
        idx = np.full((q.shape[0], k), NO_ID, np.uint64)
        dist = np.full((q.shape[0], k), np.inf, np.float32)
        check(lib().mi_knn_sharded_search_async(self._h, q.ctypes.data, q.shape[0], k, idx.ctypes.data, dist.ctypes.data))
        self._pending = getattr(self, "_pending", []) + [(idx, dist)]
        return idx, dist

    def sync(self):
        check(lib().mi_knn_sharded_sync(self._h))
        self._pending = []

    def rebalance_from(self, src: "ShardedTable"):
        """every row of `src` into this empty table, device to device (mi_knn_sharded_rebalance)"""
        check(lib().mi_knn_sharded_rebalance(self._h, src._h))

    def compact_into(self, dst: "ShardedTable") -> dict:
        """every LIVE row of this table into the empty `dst`, in global order, with its group, tags and stamp
        (mi_knn_sharded_compact_into): the compaction of a sharded table.  This table is unchanged.  Returns {"removed",
        "new_ids"} as EmbeddingTable.compact, new_ids by this table's global row."""
        rows = len(self)
        new_ids = np.empty(rows, dtype=np.uint64)
        removed = ctypes.c_uint64()
        check(lib().mi_knn_sharded_compact_into(dst._h, self._h, new_ids.ctypes.data if rows else None, rows, ctypes.byref(removed)))
        return {"removed": removed.value, "new_ids": new_ids}

    def knn(self, reference: np.ndarray, k: int = K_REFERENCE, within=None):
        """EmbeddingTable.knn over all shards; within: global ids (mi_knn_sharded_search_filtered)"""
        q = _f32(reference)
        single = q.ndim == 1
        q = q.reshape(-1, self.dim)
        idx = np.empty((q.shape[0], k), np.uint64)
        dist = np.empty((q.shape[0], k), np.float32)
        if within is None:
            check(lib().mi_knn_sharded_search(self._h, q.ctypes.data, q.shape[0], k, idx.ctypes.data, dist.ctypes.data))
        else:
            ids = _ids(within)
            check(lib().mi_knn_sharded_search_filtered(self._h, q.ctypes.data, q.shape[0], k, ids.ctypes.data if ids.size else None,
                                                       ids.size, idx.ctypes.data, dist.ctypes.data))
        return (idx[0], dist[0]) if single else (idx, dist)

    def knn_compound(self, terms: np.ndarray, mode: str = "all", without=None, without_within=None, k: int = 10, within=None):
        """EmbeddingTable.knn_compound over all shards (mi_knn_sharded_search_compound): global ids, no per-term distances"""
        pos, code, neg, w, n_neg = _compound_args(self.dim, terms, mode, without, without_within)
        k = int(k)
        idx, dist = np.empty(max(k, 1), np.uint64), np.empty(max(k, 1), np.float32)
        ids, n_ids, _keep = _among(within)
        check(lib().mi_knn_sharded_search_compound(self._h, pos.ctypes.data if pos.size else None, pos.shape[0], code,
                                                   neg.ctypes.data if n_neg else None, w.ctypes.data if n_neg else None, n_neg, k, ids,
                                                   n_ids, idx.ctypes.data, dist.ctypes.data))
        return idx[:k], dist[:k]

    def set_groups(self, groups, ids=None):
        """EmbeddingTable.set_groups on global ids (mi_knn_sharded_set_groups): every shard keeps the column of its own rows"""
        _set_groups(lib().mi_knn_sharded_set_groups, self._h, groups, ids)

    def groups(self, ids=None) -> np.ndarray:
        return _get_groups(lib().mi_knn_sharded_get_groups, self._h, ids, len(self))

    def groups_info(self) -> dict:
        info = (ctypes.c_uint64 * 2)()
        check(lib().mi_knn_sharded_groups_info(self._h, info))
        return {"n_groups": info[0], "rows": info[1]}

    def knn_grouped(self, reference: np.ndarray, k: int = 10, max_dist: float = float("inf"), within=None, facets: bool = False):
        """EmbeddingTable.knn_grouped over all shards (mi_knn_sharded_search_grouped): global ids, a group spread over several
        shards counted once, its members and facets summed"""
        return _grouped_call(lib().mi_knn_sharded_search_grouped, self._h, self.dim, (), reference, k, max_dist,
                             self.groups_info()["n_groups"] if facets else 0, facets, within=within)

    def set_attrs(self, ids, tags=None, stamps=None):
        """EmbeddingTable.set_attrs on global ids (mi_knn_sharded_set_attrs): every shard keeps the columns of its own rows"""
        _set_attrs(lib().mi_knn_sharded_set_attrs, self._h, ids, tags, stamps)

    def get_attrs(self, ids=None):
        return _get_attrs(lib().mi_knn_sharded_get_attrs, self._h, ids, len(self))

    def count_where(self, all_of=0, any_of=0, none_of=0, stamp=(None, None), group=None) -> int:
        """EmbeddingTable.count_where summed over the shards (mi_knn_sharded_count_where)"""
        return _count_where(lib().mi_knn_sharded_count_where, self._h, make_where(all_of, any_of, none_of, stamp, group))

    def rows_where(self, all_of=0, any_of=0, none_of=0, stamp=(None, None), group=None) -> np.ndarray:
        """EmbeddingTable.rows_where on global ids: the shards' lists (mi_knn_rows_where on each shard), merged ascending"""
        w = make_where(all_of, any_of, none_of, stamp, group)
        parts = []
        for s in range(self.info()["shards"]):
            h = c_vp(lib().mi_knn_sharded_shard(self._h, s))
            n = ctypes.c_uint64()
            check(lib().mi_knn_rows_where(h, ctypes.byref(w), None, 0, ctypes.byref(n)))
            ids = np.empty(max(n.value, 1), np.uint64)
            check(lib().mi_knn_rows_where(h, ctypes.byref(w), ids.ctypes.data, n.value, ctypes.byref(n)))
            parts.append(ids[:n.value])
        return np.sort(np.concatenate(parts)) if parts else np.empty(0, np.uint64)

    def knn_where(self, reference: np.ndarray, k: int = 10, all_of=0, any_of=0, none_of=0, stamp=(None, None), group=None):
        """EmbeddingTable.knn_where over all shards (mi_knn_sharded_search_where): every shard builds its own list on its
        device; global ids, the one-table result bit for bit"""
        return _search_where(lib().mi_knn_sharded_search_where, self._h, self.dim, reference, k,
                             make_where(all_of, any_of, none_of, stamp, group))

    def knn_page(self, reference: np.ndarray, k: int = 100, after=None, max_dist: float = float("inf"), within=None):
        """EmbeddingTable.knn_page over all shards (mi_knn_sharded_search_page): global ids, summed counts"""
        return _page_call(lib().mi_knn_sharded_search_page, self._h, self.dim, (), reference, k, after, max_dist, within=within)

    def knn_ordered(self, reference: np.ndarray, k: int = 100, max_dist: float = float("inf"), descending: bool = False, after=None,
                    **predicate):
        """EmbeddingTable.knn_ordered over all shards, global ids, summed counts.  The rows within max_dist of the reference in the order of their stamps (mi_knn_search_ordered): ascending, or newest
        first with descending=True; equal stamps by ascending id.  after: None (from the start) or the (stamp, id) of the
        previous page's last hit — its row may have been deleted since.  predicate: the keyword arguments of make_where (none:
        every live row).  Returns (idx, dist, stamps, counts): the hits in order, NO_ID / +inf / 0 behind them, and counts =
        {"within", "before", "beyond", "nan"} ("101-200 of within").  k <= 4096."""
        return _ordered_call(lib().mi_knn_sharded_search_ordered, self._h, self.dim, (), reference, k, max_dist, descending, after, predicate)

    def timeline(self, reference: np.ndarray, k: int = 100, max_dist: float = float("inf"), descending: bool = False, **predicate):
        """knn_ordered after knn_ordered until one comes back short: yields (idx, dist, stamps, counts) with the padding cut off.
        Rows appended or deleted between two pages are honoured as they stand when each page is asked for."""
        return _timeline(lambda after: self.knn_ordered(reference, k, max_dist, descending, after, **predicate), k)

    def stamp_histogram(self, reference: np.ndarray, edges, max_dist: float = float("inf"), **predicate) -> np.ndarray:
        """The timeline facet (mi_knn_stamp_histogram): hist[b] = the rows within max_dist (and the predicate) with exactly b of
        the strictly ascending edges <= stamp; [len(edges) + 1] uint64, summing to knn_ordered's counts["within"]."""
        return _stamp_histogram(lib().mi_knn_sharded_stamp_histogram, self._h, self.dim, (), reference, edges, max_dist, predicate)

    def near_pairs(self, max_dist: float, first_new: int = 0, cap: int = 1 << 20):
        """EmbeddingTable.near_pairs over all shards (mi_knn_sharded_near_pairs): every pair of live rows a < b (global ids)
        within max_dist whose larger id is >= first_new, pairs that cross shards included; ids and distance bits are those
        of one table holding the same rows."""
        return _pairs_call(lib().mi_knn_sharded_near_pairs, (self._h, float(max_dist), int(first_new)), cap)

    def near_pairs_stats(self):
        """mi_knn_sharded_near_pairs_stats: the last near_pairs, summed over every shard and shard pair"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_sharded_near_pairs_stats(self._h, out))
        return {"candidates": out[0], "pairs": out[1], "launches": out[2], "tiles": out[3]}

    def neighbor_counts(self, max_dist: float) -> np.ndarray:
        """EmbeddingTable.neighbor_counts over all shards (mi_knn_sharded_density): counts [rows] uint32 by global row id, the
        pairs that cross shards counted; no pair list is built."""
        counts = np.empty(len(self), np.uint32)
        check(lib().mi_knn_sharded_density(self._h, float(max_dist), counts.ctypes.data))
        return counts

    def dbscan(self, max_dist: float, min_pts: int = 5) -> dict:
        """EmbeddingTable.dbscan over all shards (mi_knn_sharded_dbscan): the same dict, arrays by global row id — bit for bit
        what one table holding the same rows returns, whatever the shard count, block size or staging.  The pairs never leave
        the devices; labels.astype(np.uint32) fits set_groups."""
        n = len(self)
        cluster, via = np.empty(n, np.uint64), np.empty(n, np.uint64)
        via_dist, counts = np.empty(n, np.float32), np.empty(n, np.uint32)
        summary = np.zeros(4, np.uint64)
        check(lib().mi_knn_sharded_dbscan(self._h, float(max_dist), int(min_pts), cluster.ctypes.data, via.ctypes.data,
                                          via_dist.ctypes.data, counts.ctypes.data, summary.ctypes.data))
        return {"labels": dense_labels(cluster), "cluster": cluster, "via": via, "via_dist": via_dist, "counts": counts,
                "summary": dict(zip(("clusters", "core", "border", "noise"), (int(v) for v in summary)))}

    def dbscan_stats(self) -> dict:
        """mi_knn_sharded_dbscan_stats: the last neighbor_counts / dbscan, summed over every shard and shard pair (unions_merged
        also counts the final merge of the shards' forests)"""
        out = (ctypes.c_uint64 * 8)()
        check(lib().mi_knn_sharded_dbscan_stats(self._h, out))
        return dict(zip(("candidates_pass1", "pairs", "tiles_pass1", "candidates_pass2", "tiles_visited", "tiles_skipped",
                         "unions_merged", "launches"), (int(v) for v in out)))

    def kmeans(self, k_or_centroids, max_iters: int = 20, seed: int = 0, init: str = "uniform") -> dict:
        """EmbeddingTable.kmeans over all shards (mi_knn_sharded_kmeans): the same dict, labels / dist by global row id — bit
        for bit what one table holding the same rows returns with fixed_sum=True, whatever the shard count, block size or
        devices.  An int k starts from the rows EmbeddingTable.kmeans(k, seed) picks over the same data.  Only sums, counts
        and centroids cross between the shards.  (k-means++ seeds: kmeans_seeded.)"""
        if init == "kmeans++":
            raise ValueError('init = "kmeans++" is not offered on a sharded table: the seeding draws every row against the rows '
                             'drawn so far on one device (mi_knn_kmeans_seed) and has no form that runs across shards; seed on '
                             'one table, or pass the centroids')
        if init != "uniform":
            raise ValueError(f'init = {init!r}: "uniform"')
        if isinstance(k_or_centroids, (int, np.integer)):
            rows = initial_centroid_rows(len(self), self.deleted(), int(k_or_centroids), seed)
            cent = np.concatenate([self.rows(int(r), 1) for r in rows]) if rows.size else np.empty((0, self.dim), np.float32)
        else:
            cent = np.array(k_or_centroids, dtype=np.float32, order="C").reshape(-1, self.dim)
        n = len(self)
        labels, dist = np.empty(n, np.uint32), np.empty(n, np.float32)
        iters, changed, obj = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_double()
        check(lib().mi_knn_sharded_kmeans(self._h, cent.ctypes.data, cent.shape[0], int(max_iters), labels.ctypes.data,
                                          dist.ctypes.data, ctypes.byref(iters), ctypes.byref(changed), ctypes.byref(obj)))
        return {"centroids": cent, "labels": labels, "dist": dist, "iters": iters.value, "changed": changed.value,
                "objective": obj.value}

    def kmeans_stats(self) -> dict:
        """mi_knn_sharded_kmeans_stats, of the last kmeans: bytes_exchanged = updates * (shards - 1) * C * (8 dim + 4) inward
        (sums and counts) + updates * (shards - 1) * C * dim * 4 outward (centroids)"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_sharded_kmeans_stats(self._h, out))
        return dict(zip(("updates", "bytes_exchanged", "segments", "merge_launches"), (int(v) for v in out)))

    def kmeans_seed(self, k: int, seed: int = 0, among=None) -> dict:
        """EmbeddingTable.kmeans_seed over all shards (mi_knn_sharded_kmeans_seed): the same dict, rows as global ids — bit for
        bit what one table holding the same rows returns, whatever the shard count, block size or devices.  Per seed only
        per-chunk integer sums, a 16-byte pick word and the chosen row cross between the shards."""
        k = int(k)
        rows, cent = np.empty(max(k, 0), np.uint64), np.empty((max(k, 0), self.dim), np.float32)
        pot = ctypes.c_double()
        ids, n_ids = None, 0
        if among is not None:
            a = _ids(among)
            n_ids = a.size
            if a.size == 0:   # an empty set of candidates, not "every row"
                a = np.zeros(1, np.uint64)
            ids = a.ctypes.data
        check(lib().mi_knn_sharded_kmeans_seed(self._h, k, int(seed), ids, n_ids, rows.ctypes.data if k else None,
                                               cent.ctypes.data if k else None, ctypes.byref(pot)))
        return {"rows": rows, "centroids": cent, "potential": pot.value}

    def kmeans_seed_stats(self) -> dict:
        """mi_knn_sharded_kmeans_seed_stats, of the last kmeans_seed: bytes_exchanged = (k + 1) * 8 * (K + shards - 1) +
        k * (shards - 1) * (32 + 8 dim), K = the chunks (at most 256 candidates of one block) of every shard but the first"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_sharded_kmeans_seed_stats(self._h, out))
        return dict(zip(("candidates", "passes", "fallbacks", "bytes_exchanged"), (int(v) for v in out)))

    def kmeans_seeded(self, k: int, max_iters: int = 20, seed: int = 0, sample: Optional[int] = None) -> dict:
        """kmeans from k-means++ seeds: kmeans_seed(k, seed) among all live rows, or, where there are more than `sample` of
        them (None = max(64 k, 16 384)), among a seeded uniform subset of that size — the rule of
        EmbeddingTable.kmeans(init="kmeans++") — and then kmeans on those centroids.  Equals, bit for bit, one table's
        kmeans(k, init="kmeans++", seed=seed, sample=sample, fixed_sum=True) over the same rows."""
        k = int(k)
        sample = max(64 * k, 16384) if sample is None else int(sample)
        live = np.setdiff1d(np.arange(len(self), dtype=np.uint64), self.deleted())
        among = np.sort(np.random.default_rng(seed).choice(live, size=sample, replace=False)) if live.size > sample else None
        return self.kmeans(self.kmeans_seed(k, seed, among)["centroids"], max_iters)

    def summarize(self, labels=None, n_groups: Optional[int] = None) -> dict:
        """EmbeddingTable.summarize over all shards (mi_knn_sharded_summarize): the same dict with labels and dist by global
        row id and cover / odd as global ids — bit for bit what one table holding the same rows returns with the option
        "kmeans_fixed_sum" on, whatever the shard count, block size or devices; a tie goes to the lowest global id.
        labels=None reads every shard's part of the group column where it lies (set_groups); n_groups defaults as there.
        The step after kmeans / dbscan on a sharded table; typical_order takes the result as it is.  Only sums, counts,
        centroids and 32 bytes per group cross between the shards."""
        return _summarize_call(lib().mi_knn_sharded_summarize, self, labels, n_groups)

    def summarize_stats(self) -> dict:
        """mi_knn_sharded_summarize_stats, of the last summarize: bytes_exchanged = (shards - 1) * C * (8 dim + 4 + 32) inward
        (sums, counts and the per-group words) + (shards - 1) * 4 * C * dim outward (centroids)"""
        out = (ctypes.c_uint64 * 4)()
        check(lib().mi_knn_sharded_summarize_stats(self._h, out))
        return dict(zip(("segments", "bytes_exchanged", "merge_launches", "members"), (int(v) for v in out)))

    def duplicates(self, max_dist: float, first_new: int = 0, cap: int = 1 << 20) -> list:
        """Groups of near-duplicate rows: near_pairs through pairs_to_groups — lists of global ids chained by distances
        <= max_dist, ascending inside a group, the groups by their first id."""
        a, b, _ = self.near_pairs(max_dist, first_new, cap)
        return pairs_to_groups(a, b)

    def assign(self, vectors: np.ndarray):
        """EmbeddingTable.assign over all shards (mi_knn_sharded_assign): labels / dist by global row id"""
        v = _f32(vectors).reshape(-1, self.dim)
        n = len(self)
        labels, dist = np.empty(n, np.uint32), np.empty(n, np.float32)
        check(lib().mi_knn_sharded_assign(self._h, v.ctypes.data, v.shape[0], labels.ctypes.data, dist.ctypes.data))
        return labels, dist

    def assign_multi(self, vectors: np.ndarray, m: int, max_dist: float = float("inf")):
        """EmbeddingTable.assign_multi over all shards (mi_knn_sharded_assign_multi): labels / dist by global row id"""
        v = _f32(vectors).reshape(-1, self.dim)
        n = len(self)
        labels, dist = np.empty((n, int(m)), np.uint32), np.empty((n, int(m)), np.float32)
        check(lib().mi_knn_sharded_assign_multi(self._h, v.ctypes.data, v.shape[0], int(m), float(max_dist), labels.ctypes.data,
                                                dist.ctypes.data))
        return labels, dist

    def knn_many(self, queries: np.ndarray, k: int):
        """EmbeddingTable.knn_many over all shards (mi_knn_sharded_search_many): global ids"""
        q = _f32(queries).reshape(-1, self.dim)
        idx, dist = np.empty((q.shape[0], int(k)), np.uint64), np.empty((q.shape[0], int(k)), np.float32)
        check(lib().mi_knn_sharded_search_many(self._h, q.ctypes.data, q.shape[0], int(k), idx.ctypes.data, dist.ctypes.data))
        return idx, dist

    def knn_many_where(self, queries: np.ndarray, k: int, **predicate):
        """EmbeddingTable.knn_many_where over all shards (mi_knn_sharded_search_many_where): global ids, matched summed"""
        return _many_where(lib().mi_knn_sharded_search_many_where, self._h, self.dim, queries, k, predicate)

    def neighbors(self, k: int, first: int = 0, n: Optional[int] = None):
        """EmbeddingTable.neighbors over all shards, composed on the host: the rows are read back (rows()), searched with
        k + 1 (knn_many) and lose their own entry (drop_self); deleted rows are padded"""
        if n is None:
            n = max(len(self) - int(first), 0)
        if not (0 <= int(first) and int(first) + int(n) <= len(self)):
            raise ValueError(f"rows [{first}, {int(first) + int(n)}) are not rows of this table ({len(self)} rows)")
        if not 1 <= int(k) <= 15:
            raise ValueError("1 <= k <= 15")
        if n == 0:
            return np.empty((0, int(k)), np.uint64), np.empty((0, int(k)), np.float32)
        ids = np.arange(int(first), int(first) + int(n), dtype=np.uint64)
        idx, dist = drop_self(*self.knn_many(self.rows(int(first), int(n)), int(k) + 1), ids)
        gone = np.isin(ids, self.deleted())
        idx[gone], dist[gone] = NO_ID, np.inf
        return idx, dist

    def delete(self, ids) -> int:
        """EmbeddingTable.delete on global ids (mi_knn_sharded_delete)"""
        return _delete(lib().mi_knn_sharded_delete, self._h, ids)

    def deleted(self) -> np.ndarray:
        return _deleted(lib().mi_knn_sharded_deleted, self._h)

    def save(self, prefix: str):
        check(lib().mi_knn_sharded_save(self._h, prefix.encode()))

    def load(self, prefix: str):
        check(lib().mi_knn_sharded_load(self._h, prefix.encode()))


def shard_bounds(n_rows: int, world: int, rank: int):
    """Contiguous row split: rank r owns [r*N/W, (r+1)*N/W)."""
    return (n_rows * rank) // world, (n_rows * (rank + 1)) // world


def gather_and_merge(local_idx: np.ndarray, local_dist: np.ndarray, k: int, group=None):
    """The one exchange step of the sharded search: all-gather every rank's k
    candidates (12*k bytes per rank and query) and merge them identically on
    every rank.  Works on any torch.distributed backend (nccl == RCCL on ROCm,
    gloo on CPU); tensors live where the backend needs them."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    nq = local_idx.shape[0] if local_idx.ndim == 2 else 1
    li = torch.from_numpy(np.ascontiguousarray(local_idx, np.uint64).view(np.int64).reshape(nq, k))
    ld = torch.from_numpy(np.ascontiguousarray(local_dist, np.float32).reshape(nq, k))
    if dist.get_backend(group) == "nccl":
        li, ld = li.cuda(), ld.cuda()
    gi = torch.empty((world * nq, k), dtype=li.dtype, device=li.device)  # rank-major concatenation
    gd = torch.empty((world * nq, k), dtype=ld.dtype, device=ld.device)
    dist.all_gather_into_tensor(gi, li, group=group)
    dist.all_gather_into_tensor(gd, ld, group=group)
    gi = gi.cpu().numpy().view(np.uint64).reshape(world, nq, k)
    gd = gd.cpu().numpy().reshape(world, nq, k)
    out_i = np.empty((nq, k), np.uint64)
    out_d = np.empty((nq, k), np.float32)
    for u in range(nq):
        out_i[u], out_d[u] = merge_candidates(gi[:, u, :], gd[:, u, :], k)
    return out_i, out_d


class ShardExchange:
    """The one exchange step of the row-sharded search, one process per GPU: every rank's k results
    — packed as k uint64 ids followed by k f32 distances, 12 k bytes — all-gathered in ONE collective and merged
    identically on every rank (mi_knn_merge).
      nccl (= RCCL over xGMI): the scan writes its list into a device buffer (Pipeline.query_device), the collective and the
          readback of the gathered lists are enqueued behind it on torch's current stream; the host never touches the
          per-rank list and blocks only in `collect`, for the oldest exchange.
      gloo (CPU rehearsals and tests): the lists come from the host results of Pipeline.query / EmbeddingTable.knn.
    `depth` exchanges may be in flight (a ring of buffers)."""

    def __init__(self, k: int, device=None, group=None, depth: int = 4):
        import torch
        import torch.distributed as dist
        self.k, self.group, self.depth = k, group, depth
        self.world = dist.get_world_size(group)
        self.on_device = dist.get_backend(group) == "nccl"
        self.nbytes = 12 * k
        dev = (device if device is not None else torch.device("cuda", torch.cuda.current_device())) if self.on_device else "cpu"
        self.ring = []
        for _ in range(depth):
            slot = {"loc": torch.empty((1, self.nbytes), dtype=torch.uint8, device=dev),
                    "all": torch.empty((self.world, self.nbytes), dtype=torch.uint8, device=dev), "busy": False}
            if self.on_device:
                slot["host"] = torch.empty((self.world, self.nbytes), dtype=torch.uint8).pin_memory()
                slot["ev"] = torch.cuda.Event()
            self.ring.append(slot)
        self.n = 0
        self.pending = []

    def _slot(self):
        slot = self.ring[self.n % self.depth]
        self.n += 1
        if slot["busy"]:
            raise RuntimeError(f"more than {self.depth} exchanges in flight: collect() first")
        slot["busy"] = True
        self.pending.append(slot)
        return slot

    def _gather(self, slot):
        import torch.distributed as dist
        dist.all_gather_into_tensor(slot["all"], slot["loc"], group=self.group)

    def query(self, pipeline: "Pipeline", reference: np.ndarray):
        """nccl only: enqueue the scan on the pipeline's search stream, the all-gather and the readback behind it."""
        import torch
        assert self.on_device, "ShardExchange.query needs the nccl backend; use submit() with host lists on gloo"
        slot = self._slot()
        p = slot["loc"].data_ptr()
        pipeline.query_device(reference, self.k, p, p + 8 * self.k, torch.cuda.current_stream().cuda_stream)
        self._gather(slot)
        slot["host"].copy_(slot["all"], non_blocking=True)
        slot["ev"].record()

    def submit(self, local_idx: np.ndarray, local_dist: np.ndarray):
        """A rank's list already on the host (gloo; or nccl after a host search): pack, all-gather."""
        import torch
        slot = self._slot()
        packed = np.concatenate([np.ascontiguousarray(local_idx, np.uint64).reshape(self.k).view(np.uint8),
                                 np.ascontiguousarray(local_dist, np.float32).reshape(self.k).view(np.uint8)])
        slot["loc"].copy_(torch.from_numpy(packed).reshape(1, -1))
        self._gather(slot)
        if self.on_device:
            slot["host"].copy_(slot["all"], non_blocking=True)
            slot["ev"].record()

    def collect(self):
        """Oldest exchange in flight -> (ids [k], distances [k]) of the whole table; blocks for that one only."""
        slot = self.pending.pop(0)
        if self.on_device:
            slot["ev"].synchronize()
            h = slot["host"].numpy()
        else:
            h = slot["all"].numpy()
        gi = np.ascontiguousarray(h[:, :8 * self.k]).view(np.uint64)
        gd = np.ascontiguousarray(h[:, 8 * self.k:]).view(np.float32)
        slot["busy"] = False
        return merge_candidates(gi, gd, self.k)

    def in_flight(self) -> int:
        return len(self.pending)


def _cstrs(strings):
    arr = (ctypes.c_char_p * max(len(strings), 1))()
    for i, p in enumerate(strings):
        arr[i] = p.encode()
    return arr


class ImageIndex:
    """Table `image` {id, image_path, embedding} (search.rs:13-18; rows inserted at clip.rs:125-137): the C ABI's
    mi_index_* — one HBM shard plus the image_path column, both inside the library.  Row id = insertion ordinal.
      `SELECT image_path FROM image WHERE image_path IN $paths`              -> existing()
      `db.insert("image").content(rows)`                                     -> insert()
      `SELECT id, image_path, embedding FROM image WHERE image_path IN $p`   -> embeddings_of()
      `SELECT id, image_path, knn() FROM image WHERE embedding <|K|> $ref`   -> web_search_text()
      `DELETE FROM image WHERE image_path IN $paths`                         -> remove()
    kept across restarts by save / load (what the database did for the reference)."""

    def __init__(self, dim: int = 768, device: int = 0, media_dir: str = ""):
        self._h = c_vp()
        self.dim, self.device, self.media_dir = dim, device, media_dir
        check(lib().mi_index_create(dim, device, media_dir.encode(), ctypes.byref(self._h)))
        self.table = EmbeddingTable.__new__(EmbeddingTable)          # the shard inside the index, borrowed
        self.table._h, self.table.dim, self.table.device = c_vp(lib().mi_index_table(self._h)), dim, device
        self.table.close = lambda: None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.table._h = c_vp()
            lib().mi_index_free(self._h)
            self._h = c_vp()

    __del__ = close

    def __len__(self) -> int:
        n = ctypes.c_uint64()
        check(lib().mi_index_size(self._h, ctypes.byref(n)))
        return n.value

    def path(self, row: int, web: bool = False) -> str:
        need = ctypes.c_size_t()
        check(lib().mi_index_path(self._h, row, int(web), None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        check(lib().mi_index_path(self._h, row, int(web), buf, need.value, None))
        return buf.value.decode()

    @property
    def paths(self) -> list:
        """image_path by row id; None for a removed row"""
        gone = set(int(i) for i in self.table.deleted())
        return [None if i in gone else self.path(i) for i in range(len(self))]

    def existing(self, paths: Sequence[str]) -> set:
        """clip.rs:74-83: which of `paths` already have a row."""
        paths = list(paths)
        flags = (ctypes.c_uint8 * max(len(paths), 1))()
        check(lib().mi_index_existing(self._h, _cstrs(paths), len(paths), flags))
        return {p for p, f in zip(paths, flags) if f}

    def insert(self, paths: Sequence[str], embeddings: np.ndarray) -> int:
        """clip.rs:125-137: one row per (image_path, embedding) pair, ids in insertion order.  Like the
        reference's table there is no uniqueness constraint; the scan loop filters first."""
        paths = list(paths)
        e = _f32(embeddings).reshape(-1, self.dim)
        if e.shape[0] != len(paths):
            raise ValueError(f"{len(paths)} paths for {e.shape[0]} embeddings")
        first = ctypes.c_uint64()
        check(lib().mi_index_insert(self._h, _cstrs(paths), e.ctypes.data, len(paths), ctypes.byref(first)))
        return first.value

    def remove(self, paths: Sequence[str]) -> int:
        """`DELETE FROM image WHERE image_path IN $paths` (mi_index_remove): every row of each path; paths without rows
        are ignored.  Returns the rows removed."""
        paths = list(paths)
        n = ctypes.c_uint64()
        check(lib().mi_index_remove(self._h, _cstrs(paths), len(paths), ctypes.byref(n)))
        return n.value

    def compact(self) -> dict:
        """The removed rows leave the table and the path column (mi_index_compact); every lookup and search names the same
        paths as before, row ids change.  Returns {"removed", "new_ids"} as EmbeddingTable.compact."""
        return _compact(lib().mi_index_compact, self._h, len(self.table))

    def live_paths(self) -> set:
        """the image_path of every row that has not been removed (mi_index_live_paths: one call)"""
        need = ctypes.c_size_t()
        check(lib().mi_index_live_paths(self._h, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(max(need.value, 1))
        check(lib().mi_index_live_paths(self._h, buf, need.value, ctypes.byref(need)))
        return {p.decode() for p in buf.raw[:need.value].split(b"\0") if p}

    def adopt(self, paths: Sequence[str]):
        """Paths for rows the fused pipeline has just written into `self.table` (mi_index_adopt)."""
        paths = list(paths)
        check(lib().mi_index_adopt(self._h, _cstrs(paths), len(paths)))

    def embeddings_of(self, paths: Sequence[str]):
        """search.rs:43-58.  Rows come back in table (id) order, whatever the request order — the
        order matters: average_slices adds in input order (search.rs:139-143)."""
        rows = self.rows_of(paths)
        return rows, [self.table.rows(r, 1)[0] for r in rows]

    def rows_of(self, paths: Sequence[str]) -> list:
        """the ids of the rows stored under `paths` (mi_index_rows_of), ascending, each once"""
        paths = list(paths)
        cnt = ctypes.c_size_t()
        check(lib().mi_index_rows_of(self._h, _cstrs(paths), len(paths), None, 0, ctypes.byref(cnt)))
        ids = np.empty(cnt.value, np.uint64)
        check(lib().mi_index_rows_of(self._h, _cstrs(paths), len(paths), ids.ctypes.data, cnt.value, ctypes.byref(cnt)))
        return [int(i) for i in ids]

    def web_search_text(self, text_embedding: np.ndarray, referenced_images: Sequence[str] = (), k: int = K_REFERENCE,
                        folders: Optional[Sequence[str]] = None):
        """search.rs:20-110 after the text tower: refine with the marked images that are in the
        table, K nearest by cosine distance, paths mapped back under `media/`.
        Returns [(id, image_path, similarity)] with similarity = vector::distance::knn().
        folders: client names ("media/2024/trip"; "media/" = everything): the K nearest among the
        images under them, whole path components (mi_index_search_within)."""
        q = _f32(text_embedding).reshape(-1)
        refs = list(referenced_images)
        idx = np.empty(k, np.uint64)
        dist = np.empty(k, np.float32)
        n = ctypes.c_uint32()
        if folders is None:
            check(lib().mi_index_search(self._h, q.ctypes.data, _cstrs(refs), len(refs), k, idx.ctypes.data, dist.ctypes.data,
                                        ctypes.byref(n)))
        else:
            fs = list(folders)
            check(lib().mi_index_search_within(self._h, q.ctypes.data, _cstrs(refs), len(refs), _cstrs(fs), len(fs), k,
                                               idx.ctypes.data, dist.ctypes.data, ctypes.byref(n)))
        return [(int(idx[i]), self.path(int(idx[i]), web=True), float(dist[i])) for i in range(n.value)]

    def web_search_diverse(self, text_embedding: np.ndarray, referenced_images: Sequence[str] = (), k: int = 100,
                           min_gap: float = 0.05, pool: Optional[int] = None, folders: Sequence[str] = (), web: bool = False):
        """web_search_text with near-duplicates collapsed (mi_index_search_diverse): the k best distinct images, each with
        the number of look-alikes (cosine distance <= min_gap to it) hidden behind it.  Returns [(id, image_path,
        similarity, hidden)].  pool: how many results of the plain search are looked at, None = min(4096, max(4 * k, 64));
        folders: as web_search_text, () = everything; web: paths as sent to the client."""
        q = _f32(text_embedding).reshape(-1)
        refs, fs = list(referenced_images), list(folders)
        k = int(k)
        pool = min(4096, max(4 * k, 64)) if pool is None else int(pool)
        idx, dist, hidden = np.empty(max(k, 1), np.uint64), np.empty(max(k, 1), np.float32), np.empty(max(k, 1), np.uint32)
        n = ctypes.c_uint32()
        check(lib().mi_index_search_diverse(self._h, q.ctypes.data, _cstrs(refs), len(refs), _cstrs(fs), len(fs), k, pool,
                                            float(min_gap), idx.ctypes.data, dist.ctypes.data, hidden.ctypes.data, ctypes.byref(n)))
        return [(int(idx[i]), self.path(int(idx[i]), web=web), float(dist[i]), int(hidden[i])) for i in range(n.value)]

    def web_search_compound(self, terms: np.ndarray, mode: str = "all", without=None, without_within=None, k: int = 100,
                            folders: Sequence[str] = (), term_dist: bool = False, web: bool = False):
        """and / or / not over text (or image) embeddings (mi_index_search_compound): EmbeddingTable.knn_compound over the
        images under `folders` (() = everything); removed paths never appear.  No refinement happens here: pass a term through
        refine_query first if it should be refined.  Returns [(id, image_path, score)], with term_dist=True [(id, image_path,
        score, [distance to every term, positives first])] — which term held a picture back."""
        pos, code, neg, w, n_neg = _compound_args(self.dim, terms, mode, without, without_within)
        fs = list(folders)
        k = int(k)
        T = pos.shape[0] + n_neg
        idx, dist = np.empty(max(k, 1), np.uint64), np.empty(max(k, 1), np.float32)
        td = np.empty((max(k, 1), max(T, 1)), np.float32) if term_dist else None
        n = ctypes.c_uint32()
        check(lib().mi_index_search_compound(self._h, pos.ctypes.data if pos.size else None, pos.shape[0], code,
                                             neg.ctypes.data if n_neg else None, w.ctypes.data if n_neg else None, n_neg, _cstrs(fs),
                                             len(fs), k, idx.ctypes.data, dist.ctypes.data, td.ctypes.data if term_dist else None,
                                             ctypes.byref(n)))
        hits = [(int(idx[i]), self.path(int(idx[i]), web=web), float(dist[i])) for i in range(n.value)]
        return [h + ([float(v) for v in td[i, :T]],) for i, h in enumerate(hits)] if term_dist else hits

    def web_search_page(self, text_embedding: np.ndarray, referenced_images: Sequence[str] = (), k: int = 100, after=None,
                        max_dist: float = float("inf"), folders: Sequence[str] = (), web: bool = True):
        """One page of web_search_text (mi_index_search_page): the query refined with the marked images, the images under
        `folders` (() = everything), then the k nearest after the cursor `after` and within max_dist; removed paths never
        appear.  Returns ([(id, image_path, similarity)], counts, next): counts = {"before", "window", "beyond", "nan"} ("101-200
        of before + window"), next = the cursor for the following page (None: this was the last)."""
        refs, fs = list(referenced_images), list(folders)
        n = ctypes.c_uint32()
        lead = (_cstrs(refs), len(refs), _cstrs(fs), len(fs))
        idx, dist, counts, nxt = _page_call(lib().mi_index_search_page, self._h, self.dim, lead, text_embedding, k, after, max_dist,
                                            tail_ptr=ctypes.byref(n))
        return [(int(idx[i]), self.path(int(idx[i]), web=web), float(dist[i])) for i in range(n.value)], counts, nxt

    def group_name(self, group: int, web: bool = True) -> str:
        """the directory behind a group id of web_search_grouped (mi_index_group_name), with its trailing '/'"""
        need = ctypes.c_size_t()
        check(lib().mi_index_group_name(self._h, int(group), int(web), None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        check(lib().mi_index_group_name(self._h, int(group), int(web), buf, need.value, None))
        return buf.value.decode()

    def group_count(self) -> int:
        n = ctypes.c_uint32()
        check(lib().mi_index_group_count(self._h, ctypes.byref(n)))
        return n.value

    def web_search_grouped(self, text_embedding: np.ndarray, referenced_images: Sequence[str] = (), k: int = 10,
                           max_dist: float = float("inf"), folders: Sequence[str] = (), by="folder", facets: bool = False,
                           web: bool = True):
        """The best picture of every folder (mi_index_search_grouped): the query refined with the marked images, the images
        under `folders` (() = everything), one hit per group within max_dist, the k nearest of those.  by="folder": a group is
        the image's directory.  by = an integer array, one label per row (k-means labels, duplicate components; NO_GROUP = the
        row stands for itself): those are the groups — the array goes into the table's column, and the next by="folder" call
        puts the folders back.  Returns ([(id, image_path, distance, group name or label, members)], totals) with totals =
        {"groups", "window", "beyond", "nan"}; a hit without a group has the name None.  facets=True appends {name or label:
        count} for the groups with at least one image within max_dist."""
        refs, fs = list(referenced_images), list(folders)
        if isinstance(by, str):
            if by != "folder":
                raise ValueError(f"by: 'folder' or an integer array, not {by!r}")
            n = ctypes.c_uint32()
            lead = (_cstrs(refs), len(refs), _cstrs(fs), len(fs))
            out = _grouped_call(lib().mi_index_search_grouped, self._h, self.dim, lead, text_embedding, k, max_dist,
                                self.group_count() if facets else 0, facets, tail_ptr=ctypes.byref(n))
            n_hits, name = n.value, (lambda g: self.group_name(g, web=web))
        else:
            labels = np.asarray(by)
            if labels.size != len(self):
                raise ValueError(f"{labels.size} labels for {len(self)} rows")
            self.table.set_groups(labels)
            within = None
            if fs:   # the live rows under the folders, whole path components, as mi_index_search_within finds them
                under = [self.media_dir + f[len("media/"):] for f in fs if f.startswith("media/")]
                under = [d if d == self.media_dir or d.endswith("/") else d + "/" for d in under]
                within = self.rows_of(sorted(p for p in self.live_paths() if any(p.startswith(d) for d in under)))
            q = text_embedding
            marked = self.embeddings_of([self.media_dir + r[len("media/"):] for r in refs if r.startswith("media/")])[1] if refs else []
            if len(marked):
                q = refine_query(text_embedding, marked)
            out = self.table.knn_grouped(q, k, max_dist, within=within, facets=facets)
            n_hits, name = int((out[0] != NO_ID).sum()), int
        idx, dist, group, members, totals = out[:5]
        hits = [(int(idx[i]), self.path(int(idx[i]), web=web), float(dist[i]), None if group[i] == NO_GROUP else name(int(group[i])),
                 int(members[i])) for i in range(n_hits)]
        if not facets:
            return hits, totals
        return hits, totals, {name(g): int(c) for g, c in enumerate(out[5]) if c}

    def group_of(self, folder: str) -> int:
        """the group id of a directory as the client names it, "media/a/b" (mi_index_group_of): web_search_where's `group`"""
        g = ctypes.c_uint32()
        check(lib().mi_index_group_of(self._h, folder.encode(), ctypes.byref(g)))
        return g.value

    def set_attrs(self, paths: Sequence[str], tags=None, stamps=None):
        """EmbeddingTable.set_attrs by stored path (mi_index_set_attrs): tags[i] / stamps[i] go to every row of paths[i]; an
        unknown path raises and writes nothing"""
        paths = list(paths)
        tg = None if tags is None else np.ascontiguousarray(np.asarray(tags, dtype=np.uint64).reshape(-1))
        st = None if stamps is None else np.ascontiguousarray(np.asarray(stamps, dtype=np.int64).reshape(-1))
        for name, col in (("tags", tg), ("stamps", st)):
            if col is not None and col.size != len(paths):
                raise ValueError(f"{col.size} {name} for {len(paths)} paths")
        check(lib().mi_index_set_attrs(self._h, _cstrs(paths), len(paths), tg.ctypes.data if tg is not None and tg.size else None,
                                       st.ctypes.data if st is not None and st.size else None))

    def web_search_where(self, text_embedding: np.ndarray, referenced_images: Sequence[str] = (), k: int = 10, all_of=0, any_of=0,
                         none_of=0, stamp=(None, None), folder: Optional[str] = None, group=None, web: bool = True):
        """web_search_text among the images a predicate keeps (mi_index_search_where): the query refined with the marked
        images, then tags / stamp as EmbeddingTable.knn_where takes them.  folder="media/a/b": only the images directly in that
        directory (its group id, group_of; or pass `group`) — no id list is built.  Returns ([(id, image_path, distance)],
        matched)."""
        refs = list(referenced_images)
        if folder is not None:
            group = self.group_of(folder)
        w = make_where(all_of, any_of, none_of, stamp, group)
        q = _f32(text_embedding).reshape(-1)
        if q.size != self.dim:
            raise ValueError(f"a query of {q.size} floats for dim {self.dim}")
        k = int(k)
        idx, dist = np.empty(max(k, 1), np.uint64), np.empty(max(k, 1), np.float32)
        n, matched = ctypes.c_uint32(), ctypes.c_uint64()
        check(lib().mi_index_search_where(self._h, q.ctypes.data, _cstrs(refs), len(refs), k, ctypes.byref(w), idx.ctypes.data,
                                          dist.ctypes.data, ctypes.byref(n), ctypes.byref(matched)))
        return [(int(idx[i]), self.path(int(idx[i]), web=web), float(dist[i])) for i in range(n.value)], matched.value

    def web_search_ordered(self, text_embedding: np.ndarray, referenced_images: Sequence[str] = (), k: int = 100,
                           max_dist: float = float("inf"), descending: bool = True, after=None, folder: Optional[str] = None,
                           web: bool = True, **predicate):
        """web_search_text as a timeline (mi_index_search_ordered): the query refined with the marked images, the images within
        max_dist in the order of their stamps (newest first by default), a page of k after the (stamp, id) cursor.  predicate:
        the keyword arguments of make_where; folder="media/a/b": only the images directly in that directory.  Returns ([(id,
        image_path, distance, stamp)], counts, next) — next = the cursor for the following page, None when this was the last."""
        refs = list(referenced_images)
        if folder is not None:
            predicate["group"] = self.group_of(folder)
        idx, dist, stamps, counts = _ordered_call(lib().mi_index_search_ordered, self._h, self.dim, (_cstrs(refs), len(refs)),
                                                  text_embedding, k, max_dist, descending, after, predicate, n_found=True)
        n = int((idx != NO_ID).sum())
        nxt = (int(stamps[n - 1]), int(idx[n - 1])) if n and n == int(k) else None
        return [(int(idx[i]), self.path(int(idx[i]), web=web), float(dist[i]), int(stamps[i])) for i in range(n)], counts, nxt

    def web_timeline_histogram(self, text_embedding: np.ndarray, edges, referenced_images: Sequence[str] = (),
                               max_dist: float = float("inf"), folder: Optional[str] = None, **predicate) -> np.ndarray:
        """The "matches per month" strip above web_search_ordered (mi_index_stamp_histogram): EmbeddingTable.stamp_histogram
        behind the refined query; edges are the month starts."""
        refs = list(referenced_images)
        if folder is not None:
            predicate["group"] = self.group_of(folder)
        return _stamp_histogram(lib().mi_index_stamp_histogram, self._h, self.dim, (_cstrs(refs), len(refs)), text_embedding, edges,
                                max_dist, predicate)

    def duplicates(self, max_dist: float, first_new: int = 0, web: bool = False, max_pairs: int = 1 << 20) -> list:
        """Groups of near-duplicate images (mi_index_duplicates): lists of paths whose embeddings are chained by cosine
        distances <= max_dist, ordered by row id inside a group and by their first row between groups; removed paths
        never appear.  first_new: only what the rows from that id on duplicate.  web: names as sent to the client."""
        return self._pair_groups(lib().mi_index_duplicates, (self._h, float(max_dist), int(first_new), max_pairs), web)

    def _pair_groups(self, fn, lead, web: bool) -> list:
        """fn(*lead, ids, cap_ids, group_start, cap_groups, &n_ids, &n_groups) of duplicates / bursts -> lists of paths"""
        n_ids, n_groups = ctypes.c_uint64(), ctypes.c_uint64()
        check(fn(*lead, None, 0, None, 0, ctypes.byref(n_ids), ctypes.byref(n_groups)))
        ids, starts = np.empty(n_ids.value, np.uint64), np.empty(n_groups.value + 1, np.uint64)
        check(fn(*lead, ids.ctypes.data if ids.size else None, ids.size, starts.ctypes.data, starts.size, ctypes.byref(n_ids),
                 ctypes.byref(n_groups)))
        return [[self.path(int(i), web=web) for i in g] for g in _groups(ids, starts)]

    def bursts(self, max_dist: float, window: int, web: bool = False, max_pairs: int = 1 << 20) -> list:
        """Bursts (mi_index_bursts): duplicates' groups over the pairs that look alike AND were taken within `window` of each
        other (the stamps set_attrs set; EmbeddingTable.near_pairs_window through pairs_to_groups) — "the twelve shots of that
        jump", not every beach picture of ten years."""
        return self._pair_groups(lib().mi_index_bursts, (self._h, float(max_dist), int(window), 0, max_pairs), web)

    def matches(self, other: "ImageIndex", max_dist: float, web: bool = False, max_pairs: int = 1 << 20) -> list:
        """"Skip what I already have" (mi_index_matches): (path here, path in `other`, distance) for every pair of images
        within max_dist, ordered by this index's row id, then the other's; removed paths never appear."""
        a, b, d = _pairs_call(lib().mi_index_matches, (self._h, other._h, float(max_dist)), max_pairs)
        return [(self.path(int(x), web=web), other.path(int(y), web=web), float(z)) for x, y, z in zip(a, b, d)]

    def themes(self, max_dist: float, min_pts: int = 5, web: bool = False):
        """The events / themes that are really there, however many, and the odd pictures (mi_index_themes: EmbeddingTable.dbscan
        on the index's table): (lists of paths, the largest cluster first, equal sizes by their first row, paths ordered by
        row id inside a list; the paths of the noise rows).  Removed paths are in neither."""
        return self._clusters(lib().mi_index_themes, (self._h, float(max_dist), int(min_pts)), web)

    def events(self, max_dist: float, window: int, min_pts: int = 5, web: bool = False):
        """Events (mi_index_events): themes() whose neighbourhood is "within max_dist and within `window` in time"
        (EmbeddingTable.dbscan_window on the index's table): a theme photographed in two far-apart periods is two events.
        Same output shape as themes()."""
        return self._clusters(lib().mi_index_events, (self._h, float(max_dist), int(window), int(min_pts)), web)

    def _clusters(self, fn, lead, web: bool):
        """fn(*lead, ids, cap_ids, group_start, cap_groups, &n_ids, &n_groups, &n_noise) of themes / events -> (lists, noise)"""
        n_ids, n_groups, n_noise = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        n = len(self.table)
        ids, starts = np.empty(n, np.uint64), np.empty(n + 1, np.uint64)
        check(fn(*lead, ids.ctypes.data if n else None, n, starts.ctypes.data, starts.size, ctypes.byref(n_ids), ctypes.byref(n_groups),
                 ctypes.byref(n_noise)))
        ids, starts = ids[:n_ids.value], starts[:n_groups.value + 1]
        groups = sorted(_groups(ids, starts), key=lambda g: (-len(g), int(g[0])))
        out = set(int(i) for i in ids) | set(int(i) for i in self.table.deleted())
        noise = [r for r in range(n) if r not in out]   # n_noise.value of them
        return [[self.path(int(i), web=web) for i in g] for g in groups], [self.path(r, web=web) for r in noise]

    def theme_tree(self, max_dists, min_pts: int = 5, web: bool = False):
        """Themes inside themes (EmbeddingTable.dbscan_levels on the index's table): (themes, noise).  themes = the clusters
        of the loosest distance max_dists[-1], the largest first, equal sizes by their first row; each a dict {"level",
        "max_dist", "paths" (ordered by row id), "children"}, children = the clusters of the level below whose core rows lie in
        it, ordered the same way, down to level 0.  noise = the paths of the top level's noise rows.  Removed paths are in
        neither.  (A child's border path may be missing from its parent's paths: the tree goes through core rows.)"""
        d = _levels(max_dists)
        res = self.table.dbscan_levels(d, min_pts)
        labels, L = res["labels"], d.size
        paths = {}

        def path(r):
            if r not in paths:
                paths[r] = self.path(r, web=web)
            return paths[r]

        def nodes(l, which):
            rows = {c: np.flatnonzero(labels[l] == c) for c in which}
            out = []
            for c in sorted(which, key=lambda c: (-rows[c].size, int(rows[c][0]))):
                kids = [int(k) for k in np.flatnonzero(res["tree"][l - 1] == c)] if l > 0 else []
                out.append({"level": l, "max_dist": float(d[l]), "paths": [path(int(r)) for r in rows[c]],
                            "children": nodes(l - 1, kids) if l > 0 else []})
            return out

        top = labels[L - 1]
        themes = nodes(L - 1, list(range(int(top.max()) + 1 if top.size else 0)))
        deleted = set(int(r) for r in self.table.deleted())
        noise = [path(r) for r in range(top.size) if top[r] < 0 and r not in deleted]
        return themes, noise

    def label(self, vectors: np.ndarray, names: Optional[Sequence[str]] = None, web: bool = False) -> dict:
        """"Tag my library" (EmbeddingTable.assign): {path: (label, distance)} for every path that has not been removed;
        label = the index of the nearest of `vectors` (text embeddings of the tags), or names[index].  A path with several
        rows reports its last row."""
        labels, dist = self.table.assign(vectors)
        out = {}
        for r in range(labels.size):
            if labels[r] != NO_LABEL:
                lab = int(labels[r])
                out[self.path(r, web=web)] = (names[lab] if names is not None else lab, float(dist[r]))
        return out

    def tags(self, vectors: np.ndarray, names: Optional[Sequence[str]] = None, m: int = 5, max_dist: float = float("inf"),
             web: bool = False) -> dict:
        """Several tags per image, none where nothing matches (EmbeddingTable.assign_multi): {path: [(label, distance), ...]}
        for every path that has not been removed, nearest first, at most m of them and only those within max_dist — an
        untagged image has an empty list.  label = the index into `vectors` (text embeddings of the tags), or names[index].
        A path with several rows reports its last row."""
        labels, dist = self.table.assign_multi(vectors, m, max_dist)
        deleted = set(int(r) for r in self.table.deleted())
        out = {}
        for r in range(labels.shape[0]):
            if r in deleted:
                continue
            hits = [(int(l), float(d)) for l, d in zip(labels[r], dist[r]) if l != NO_LABEL]
            out[self.path(r, web=web)] = [(names[l] if names is not None else l, d) for l, d in hits]
        return out

    def related(self, k: int = 10, web: bool = False) -> dict:
        """"More like this" for every image (EmbeddingTable.neighbors): {path: [(path, distance), ...]} over the paths that
        have not been removed, nearest first, at most k other images each.  A path with several rows reports its last row."""
        idx, dist = self.table.neighbors(k)
        deleted = set(int(r) for r in self.table.deleted())
        names = {}

        def name(r):
            if r not in names:
                names[r] = self.path(r, web=web)
            return names[r]

        out = {}
        for r in range(idx.shape[0]):
            if r not in deleted:
                out[name(r)] = [(name(int(i)), float(d)) for i, d in zip(idx[r], dist[r]) if i != NO_ID]
        return out

    def best_per_label(self, vectors: np.ndarray, names: Optional[Sequence[str]] = None, k: int = 10, web: bool = False) -> dict:
        """"The best k images for each of my tags" (EmbeddingTable.knn_many): {label: [(path, distance), ...]}, nearest
        first; label = the index into `vectors` (text embeddings of the tags), or names[index].  Removed paths never
        appear."""
        idx, dist = self.table.knn_many(vectors, k)
        return {(names[c] if names is not None else c): [(self.path(int(i), web=web), float(d)) for i, d in zip(idx[c], dist[c]) if i != NO_ID]
                for c in range(idx.shape[0])}

    def best_per_label_where(self, vectors: np.ndarray, names: Optional[Sequence[str]] = None, k: int = 10, web: bool = False,
                             **predicate) -> dict:
        """best_per_label among the images a predicate keeps (EmbeddingTable.knn_many_where): "the best k for each of my
        tags among my favourites, 2019-2021"; with none_of = the hidden flag a hidden picture shows up under no tag."""
        idx, dist, _matched = self.table.knn_many_where(vectors, k, **predicate)
        return {(names[c] if names is not None else c): [(self.path(int(i), web=web), float(d)) for i, d in zip(idx[c], dist[c]) if i != NO_ID]
                for c in range(idx.shape[0])}

    def related_where(self, k: int = 10, web: bool = False, **predicate) -> dict:
        """related with the answers narrowed (EmbeddingTable.neighbors_where): every image that has not been removed is
        listed, only the images the predicate keeps stand beside it."""
        idx, dist = self.table.neighbors_where(k, **predicate)
        deleted = set(int(r) for r in self.table.deleted())
        names = {}

        def name(r):
            if r not in names:
                names[r] = self.path(r, web=web)
            return names[r]

        return {name(r): [(name(int(i)), float(d)) for i, d in zip(idx[r], dist[r]) if i != NO_ID]
                for r in range(idx.shape[0]) if r not in deleted}

    def suggest_folders(self, inbox: str, k: int = 10, max_dist: float = float("inf"), min_votes: int = 1, web: bool = False,
                        **voters_predicate) -> dict:
        """"File my inbox" (EmbeddingTable.propose_groups): the images directly in the directory `inbox` ("media/inbox", as
        group_of takes it) ask, the images of every other folder vote (narrowed by make_where's keywords: hidden pictures do
        not vote).  {path: (folder name, votes, heard, distance)} for the inbox images whose winning folder got at least
        min_votes; nothing is moved."""
        ask = self.group_of(inbox)
        # the table's group column holds the directories once a call under the group flag has run: one row of the inbox
        unit = np.zeros(self.dim, np.float32)
        unit[0] = 1.0
        self.web_search_where(unit, k=1, group=ask)
        res = self.table.propose_groups(k, max_dist, ask, **voters_predicate)
        out = {}
        for r in np.nonzero((res["group"] != NO_GROUP) & (res["votes"] >= int(min_votes)))[0]:
            out[self.path(int(r), web=web)] = (self.group_name(int(res["group"][r]), web=web), int(res["votes"][r]),
                                               int(res["heard"][r]), float(res["dist"][r]))
        return out

    def clusters(self, k: int, max_iters: int = 20, seed: int = 0, web: bool = False, init: str = "uniform",
                 sample: Optional[int] = None) -> list:
        """"Group my library into k themes" (EmbeddingTable.kmeans): lists of paths, the largest cluster first; removed
        paths never appear, empty clusters are left out.  init / sample: the seeding, as EmbeddingTable.kmeans."""
        res = self.table.kmeans(int(k), max_iters=max_iters, seed=seed, init=init, sample=sample)
        rows = [r for r in range(res["labels"].size) if res["labels"][r] != NO_LABEL]
        return clusters_of(res["labels"][rows], [self.path(r, web=web) for r in rows])

    def _overview(self, res: dict, names, web: bool) -> list:
        out = []
        for g in sorted(range(len(names)), key=lambda c: (-int(res["count"][c]), c)):
            if int(res["count"][g]) == 0:
                continue
            cover, odd = int(res["cover"][g]), int(res["odd"][g])
            mean = float(res["mean_dist"][g])
            out.append({"group": names[g], "images": int(res["count"][g]), "cover": self.path(cover, web=web),
                        "cover_dist": float(res["cover_dist"][g]), "odd_one_out": None if odd == int(NO_ID) else self.path(odd, web=web),
                        "odd_dist": float(res["odd_dist"][g]), "mean_dist": mean})
        return out

    def folder_overview(self, web: bool = False) -> list:
        """The folders at a glance (mi_index_folder_overview): per directory that holds an image {folder, images, cover,
        cover_dist, odd_one_out, odd_dist, mean_dist}, the largest first, equal sizes by directory id.  cover = the image
        nearest to the folder's centroid (its medoid), odd_one_out = the farthest; removed paths count nowhere."""
        C = self.group_count()
        n = ctypes.c_uint32()
        count, cover, odd, measured, spread = (np.empty(C, np.uint64) for _ in range(5))
        cover_dist, odd_dist = np.empty(C, np.float32), np.empty(C, np.float32)
        check(lib().mi_index_folder_overview(self._h, C, count.ctypes.data, cover.ctypes.data, cover_dist.ctypes.data, odd.ctypes.data,
                                             odd_dist.ctypes.data, measured.ctypes.data, spread.ctypes.data, ctypes.byref(n)))
        C = min(C, n.value)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(measured > 0, spread.astype(np.float64) / measured.astype(np.float64) * 2.0 ** -30, np.nan)
        res = {"count": count[:C], "cover": cover, "cover_dist": cover_dist, "odd": odd, "odd_dist": odd_dist, "mean_dist": mean}
        out = self._overview(res, [self.group_name(g, web=web) for g in range(C)], web)
        for o in out:
            o["folder"] = o.pop("group")
        return out

    def folder_highlights(self, m: int = 9, min_gap: float = float("-inf"), web: bool = False) -> list:
        """Up to m pictures that tell what is in each folder (mi_index_folder_highlights: farthest-first picks started at
        the folder's cover): per directory that holds an image {folder, highlights = paths in pick order, gaps = a pick's
        distance to the nearest earlier pick (+inf for the cover)}, in directory order.  A pick is made only while that
        distance is above min_gap; removed paths are never picked."""
        C, m = self.group_count(), int(m)
        n = ctypes.c_uint32()
        picks, gap, n_picked = np.empty(C * max(m, 0), np.uint64), np.empty(C * max(m, 0), np.float32), np.empty(C, np.uint32)
        check(lib().mi_index_folder_highlights(self._h, C, m, float(min_gap), picks.ctypes.data, gap.ctypes.data, n_picked.ctypes.data,
                                               ctypes.byref(n)))
        C = min(C, n.value)
        picks, gap = picks.reshape(-1, m), gap.reshape(-1, m)
        out = []
        for g in range(C):
            k = int(n_picked[g])
            if k:
                out.append({"folder": self.group_name(g, web=web), "highlights": [self.path(int(r), web=web) for r in picks[g, :k]],
                            "gaps": [float(v) for v in gap[g, :k]]})
        return out

    def highlights(self, paths: Sequence[str], m: int = 9, min_gap: float = float("-inf"), web: bool = False) -> list:
        """Up to m of `paths` that span them all (EmbeddingTable.representatives_of over their rows, started at their cover):
        the highlights of a result list or of a theme, as paths in pick order."""
        ids = self.rows_of(paths)
        if not ids:
            return []
        res = self.table.representatives_of(ids, m, min_gap)
        return [self.path(int(r), web=web) for r in res["rows"][0, :int(res["n_picked"][0])]]

    def cluster_overview(self, k: int, max_iters: int = 20, seed: int = 0, web: bool = False, init: str = "uniform",
                         sample: Optional[int] = None) -> list:
        """"Group my library into k themes and show me each": EmbeddingTable.kmeans, then summarize over its labels — per
        non-empty cluster {group (the label), images, cover, cover_dist, odd_one_out, odd_dist, mean_dist}, largest first."""
        res = self.table.kmeans(int(k), max_iters=max_iters, seed=seed, init=init, sample=sample)
        C = res["centroids"].shape[0]
        return self._overview(self.table.summarize(res["labels"], C), list(range(C)), web)

    def theme_overview(self, max_dist: float, min_pts: int = 5, web: bool = False) -> list:
        """The themes that are really there, each with its cover (EmbeddingTable.dbscan, its dense labels, then summarize):
        per theme {group (the dense label), images, cover, cover_dist, odd_one_out, odd_dist, mean_dist}, largest first.
        Noise belongs to no theme."""
        labels = self.table.dbscan(max_dist, min_pts)["labels"]
        C = int(labels.max()) + 1 if labels.size and labels.max() >= 0 else 0
        if C == 0:
            return []
        return self._overview(self.table.summarize(labels.astype(np.uint32), C), list(range(C)), web)

    def save(self, directory: str):
        check(lib().mi_index_save(self._h, directory.encode()))

    @classmethod
    def load(cls, directory: str, device: int = 0, dim: int = 768) -> "ImageIndex":
        ix = cls(dim, device, "")
        check(lib().mi_index_load(ix._h, directory.encode()))
        need = ctypes.c_size_t()
        check(lib().mi_index_media_dir(ix._h, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        check(lib().mi_index_media_dir(ix._h, buf, need.value, None))
        ix.media_dir = buf.value.decode()
        return ix


def decode_rgb8(path: str) -> np.ndarray:
    """`image::open(path)...to_rgb8()` with Pillow as the decoder: RGB8 [H,W,3].  High-bit-depth images (16-bit PNG /
    TIFF, modes I;16 / I / F) are SCALED to 8 bits the way the image crate converts sample types (>> 8), not clipped at
    255 as Pillow's convert("RGB") does — those photos would otherwise embed as almost white."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode in ("I;16", "I;16B", "I;16L", "I"):
            a = np.asarray(im).astype(np.uint32)
            a = (a >> 8).clip(0, 255).astype(np.uint8) if a.max(initial=0) > 255 else a.astype(np.uint8)
            return np.repeat(a[..., None], 3, axis=2)
        if im.mode == "F":
            a = np.asarray(im, np.float32)
            return np.repeat((np.clip(a, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)[..., None], 3, axis=2)
        return np.asarray(im.convert("RGB"), np.uint8)


def _image_files(media_dir: str, errors=None) -> list:
    """the scan's walk (clip.rs:42-60): every allow-listed file under media_dir, following links, each directory once.
    errors (a list, optional) collects what the walk could not look into — an unreadable directory, a link whose target is
    gone (an unmounted folder looks just like that) — so that a prune does not take what it could not see for deleted."""
    import os
    from .clip import is_image_path
    paths = []
    seen_dirs = set()
    note = errors.append if errors is not None else (lambda e: None)
    for root, dirs, files in os.walk(media_dir, followlinks=True, onerror=note):
        # WalkDir::follow_links detects cycles; os.walk does not: never descend into a directory twice
        st = os.stat(root)
        seen_dirs.add((st.st_dev, st.st_ino))
        keep = []
        for d in dirs:
            try:
                sd = os.stat(os.path.join(root, d))
            except OSError as err:
                note(err)
                continue
            if (sd.st_dev, sd.st_ino) not in seen_dirs:
                seen_dirs.add((sd.st_dev, sd.st_ino))
                keep.append(d)
        dirs[:] = keep
        for name in files:
            p = os.path.join(root, name)
            if os.path.islink(p) and not os.path.exists(p):
                note(OSError(f"dangling link {p}"))
            elif os.path.isfile(p) and is_image_path(p):
                paths.append(p)
    return paths


def prune_missing_images(index, media_dir: str, found=None) -> int:
    """Remove (ImageIndex.remove) the rows whose stored path lies under `media_dir` and is no longer an allow-listed
    file there: deleted photos, and the old paths of moved or renamed folders.  `found`: the walk's paths if the caller
    has them (embed_all_images_in_dir), else the directory is walked here.  Rows of paths outside media_dir are kept.
    A walk that could not see everything (an unreadable directory, a dangling link: _image_files) removes nothing and
    raises OSError — a folder that is briefly unmounted must not lose its rows.  Returns the rows removed."""
    if found is None:
        errors = []
        found = _image_files(media_dir, errors)
        if errors:
            raise OSError(f"the walk of {media_dir} was incomplete ({errors[0]}); nothing was removed")
    found = set(found)
    prefix = media_dir.rstrip("/") + "/"
    stale = sorted(p for p in index.live_paths() if p.startswith(prefix) and p not in found)
    return index.remove(stale) if stale else 0


def embed_all_images_in_dir(model, index: ImageIndex, media_dir: str, image_chunk_size: int = 500, decode=None,
                            shuffle_seed=None, prune: bool = False, compact_above: Optional[float] = None) -> int:
    """clip.rs:42-151: walk `media_dir` (following links), keep the allow-listed extensions, shuffle,
    and per chunk: skip paths that already have a row, decode, embed (resize + normalise + tower on
    the device: Model.forward_images), insert.  A crash loses at most one chunk; a rerun resumes.
    `decode(path) -> RGB8 [H,W,3]` defaults to Pillow; files that fail to decode are logged and
    skipped TOGETHER WITH their path (the reference zips the unfiltered path list with the
    surviving embeddings, clip.rs:125-134, which shifts paths after a failure).  prune=True first removes the rows of
    files that are gone from media_dir (prune_missing_images; the reference only ever adds); compact_above: after such a
    prune, when deleted rows / rows exceeds this fraction the index is compacted (ImageIndex.compact: row ids change,
    paths do not); None = never.  Returns rows added."""
    import logging
    import random
    if decode is None:
        decode = decode_rgb8
    errors = []
    paths = _image_files(media_dir, errors)
    if prune:
        if errors:  # what the walk could not see is not gone: no prune this time
            logging.getLogger(__name__).error("walk of %s incomplete (%s): rows not pruned", media_dir, errors[0])
        else:
            prune_missing_images(index, media_dir, paths)
            if compact_above is not None:
                rows = len(index.table)
                if rows and len(index.table.deleted()) / rows > compact_above:
                    index.compact()
    random.Random(shuffle_seed).shuffle(paths)
    added = 0
    for c0 in range(0, len(paths), image_chunk_size):
        chunk = paths[c0:c0 + image_chunk_size]
        have = index.existing(chunk)
        new_paths, images = [], []
        for p in chunk:
            if p in have:
                continue
            try:
                images.append(decode(p))
                new_paths.append(p)
            except Exception as err:  # noqa: BLE001 — mirrors `Failed to open image` (clip.rs:98-101)
                logging.getLogger(__name__).error("Failed to open image %s: %s", p, err)
        if new_paths:
            index.insert(new_paths, model.forward_images(images))
            added += len(new_paths)
    return added
