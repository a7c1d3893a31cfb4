"""What the narrowed many-query calls cost: --rows synthetic rows at dim 768, 1 000 Gaussian queries, k = 10.

    python tools/measure_many_where.py [--rows 1000000] [--parent-lib PATH] [--out profiles/many_where_profile.json]

  (a) mi_knn_search_many — on this library and, with --parent-lib (a libmi355clip.so built from the parent commit), on that
      one too: both loaded into this process, each with a table of its own over the same rows, timed alternately.
      And on this library over a table with one deleted row (stage 1 reads a bitmap, as under every mask).
  (b) mi_knn_search_many_where under an all-pass predicate.
  (c) the same with 10 % and with 1 % of the rows passing, with the stage-1 candidate counts.
  (d) mi_knn_propose_groups, k = 10: 10 % of the rows hold one of ten groups and vote, the rest ask.
  (e) the mask alone: a predicate that no row meets ends the call behind many_mask_kernel and the 8-byte read of its count.
  (f) the one-residue mask (rows with index % 16 == 0) at k = 16: no threshold forms, every passing row is a candidate of
      every query and stage 1's buffer overflows into pieces (the known cost).
Host clock around calls that wait for their results; one warm-up per variant, then --reps rounds that visit the variants in
turn; medians.  ctypes only: the parent's library lacks the new symbols, so image_search_amd._lib cannot bind it.
"""
import argparse
import ctypes
import datetime
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM, NQ, K = 768, 1000, 10
NO_GROUP = 0xFFFFFFFF
TEN, ONE, SIXTEENTH, NOBODY = 1 << 0, 1 << 1, 1 << 2, 1 << 40
vp, u32, u64, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float


class Where(ctypes.Structure):
    _fields_ = [("all_of", u64), ("any_of", u64), ("none_of", u64), ("stamp_lo", ctypes.c_int64), ("stamp_hi", ctypes.c_int64),
                ("group", u32), ("flags", u32)]


def where(all_of=0):
    return Where(all_of, 0, 0, -(1 << 63), (1 << 63) - 1, 0, 0)


def load(path, new_symbols):
    try:
        import torch  # noqa: F401  (one HIP runtime per process: image_search_amd/_lib.py)
    except ImportError:
        pass
    l = ctypes.CDLL(path)
    sig = {"mi_knn_create": [u32, ctypes.c_int, ctypes.POINTER(vp)], "mi_knn_free": [vp],
           "mi_knn_append_synthetic": [vp, u64, u64, u64], "mi_knn_search_many": [vp, vp, u32, u32, vp, vp],
           "mi_knn_search_many_stats": [vp, ctypes.POINTER(u64)], "mi_knn_set_attrs": [vp, vp, u64, vp, vp],
           "mi_knn_set_groups": [vp, vp, u64, vp], "mi_knn_delete": [vp, vp, u64, ctypes.POINTER(u64)]}
    if new_symbols:
        sig.update({"mi_knn_search_many_where": [vp, vp, u32, u32, ctypes.POINTER(Where), vp, vp, ctypes.POINTER(u64)],
                    "mi_knn_propose_groups": [vp, u32, f32, u32, ctypes.POINTER(Where), vp, vp, vp, vp, ctypes.POINTER(u64)],
                    "mi_knn_propose_groups_stats": [vp, ctypes.POINTER(u64)]})
    for name, args in sig.items():
        fn = getattr(l, name)
        fn.argtypes = args
        fn.restype = None if name == "mi_knn_free" else ctypes.c_int
    l.mi_last_error.restype = ctypes.c_char_p
    return l


def ok(l, rc):
    if rc != 0:
        sys.exit(f"a call failed with {rc}: {l.mi_last_error().decode(errors='replace')}")


def table(l, rows):
    h = vp()
    ok(l, l.mi_knn_create(DIM, 0, ctypes.byref(h)))
    ok(l, l.mi_knn_append_synthetic(h, 11, 0, rows))
    return h


def stats(l, h, fn="mi_knn_search_many_stats"):
    out = (u64 * 4)()
    ok(l, getattr(l, fn)(h, out))
    return list(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lib", default=os.path.join(ROOT, "image_search_amd", "libmi355clip.so"))
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "many_where_profile.json"))
    a = ap.parse_args()
    n = a.rows
    rng = np.random.default_rng(5)
    q = np.ascontiguousarray(rng.standard_normal((NQ, DIM)).astype(np.float32))
    new = load(a.lib, True)
    t = table(new, n)
    ids = np.arange(n, dtype=np.uint64)
    u = rng.random(n)
    tags = (np.where(u < 0.1, TEN, 0) | np.where(u < 0.01, ONE, 0) | np.where(ids % 16 == 0, SIXTEENTH, 0)).astype(np.uint64)
    ok(new, new.mi_knn_set_attrs(t, ids.ctypes.data, n, tags.ctypes.data, None))
    groups = np.where(u < 0.1, rng.integers(0, 10, n), NO_GROUP).astype(np.uint32)
    ok(new, new.mi_knn_set_groups(t, ids.ctypes.data, n, groups.ctypes.data))

    idx, dist = np.empty((NQ, 16), np.uint64), np.empty((NQ, 16), np.float32)
    matched = u64()

    def many(l, h):
        ok(l, l.mi_knn_search_many(h, q.ctypes.data, NQ, K, idx.ctypes.data, dist.ctypes.data))
        return stats(l, h)

    def many_where(all_of, k=K):
        w = where(all_of)
        ok(new, new.mi_knn_search_many_where(t, q.ctypes.data, NQ, k, ctypes.byref(w), idx.ctypes.data, dist.ctypes.data,
                                             ctypes.byref(matched)))
        return stats(new, t) + [matched.value]

    # (a) again on a table with ONE deleted row: stage 1 then reads a bitmap for the columns, as it does under every mask
    t_del = table(new, n)
    gone = np.array([n - 1], np.uint64)
    ok(new, new.mi_knn_delete(t_del, gone.ctypes.data, 1, None))
    variants = {"a_search_many": lambda: many(new, t), "a_search_many_one_deleted": lambda: many(new, t_del)}
    if a.parent_lib:
        old = load(a.parent_lib, False)
        t_old = table(old, n)
        variants["a_search_many_parent"] = lambda: many(old, t_old)
    variants.update({"b_all_pass": lambda: many_where(0), "c_ten_percent": lambda: many_where(TEN),
                     "c_one_percent": lambda: many_where(ONE), "e_mask_alone": lambda: many_where(NOBODY)})

    res = {"box": socket.gethostname(), "date": datetime.date.today().isoformat(), "rows": n, "queries": NQ, "k": K, "reps": a.reps,
           "clock": "host clock around calls that wait for their results; median"}
    runs, last = {name: [] for name in variants}, {}
    for name, f in variants.items():   # warm-up: code objects, the first allocations
        f()
    answers = {}
    for rep in range(a.reps):
        for name, f in variants.items():
            t0 = time.perf_counter()
            last[name] = f()
            runs[name].append(time.perf_counter() - t0)
            if name in ("a_search_many", "a_search_many_parent", "b_all_pass"):   # the same answers, bit for bit
                answers[name] = (idx.reshape(-1)[:NQ * K].copy(), dist.reshape(-1)[:NQ * K].copy().view(np.uint32))   # written [NQ][K]
    ref = answers["a_search_many"]
    for name, got in answers.items():
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), name
    for name in variants:
        st = last[name]
        res[name] = {"host_s_median": statistics.median(runs[name]), "host_s": runs[name], "candidates": st[0], "hits": st[1],
                     "launches": st[2], "tiles": st[3], "candidates_per_query": st[0] / NQ}
        if len(st) > 4:
            res[name]["matched"] = st[4]
        print(name, json.dumps(res[name]), flush=True)
    res["b_bound_s"] = res["a_search_many"]["host_s_median"] * 1.025 + res["e_mask_alone"]["host_s_median"]
    print("b <= a x 1.025 + e:", res["b_all_pass"]["host_s_median"], "<=", res["b_bound_s"], flush=True)

    # (f) and (d): long calls, one warm-up and three runs each
    for name, f in (("f_one_residue_k16", lambda: many_where(SIXTEENTH, 16)), ("d_propose_groups", None)):
        if f is None:
            g, v, h = (np.empty(n, np.uint32) for _ in range(3))
            dd = np.empty(n, np.float32)
            tot = (u64 * 4)()

            def f():
                ok(new, new.mi_knn_propose_groups(t, K, np.inf, NO_GROUP, None, g.ctypes.data, v.ctypes.data, h.ctypes.data,
                                                  dd.ctypes.data, tot))
                return stats(new, t, "mi_knn_propose_groups_stats") + list(tot)
        f()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            st = f()
            times.append(time.perf_counter() - t0)
        res[name] = {"host_s_median": statistics.median(times), "host_s": times, "stats": st[:4], "rest": st[4:]}
        print(name, json.dumps(res[name]), flush=True)
    new.mi_knn_free(t)
    new.mi_knn_free(t_del)
    if a.parent_lib:
        old.mi_knn_free(t_old)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
