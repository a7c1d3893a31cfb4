"""What the ordered search costs on top of the distance scan: 10 M synthetic rows of dim 768, k = 100, each case
measured against mi_knn_search_page at the same k and bound on the same table — that call runs the same scan and then selects
on the distance alone, so the ratio is the price of selecting on the stamp.  Cases: mi_knn_search_ordered at a bound that keeps
about 1 % of the rows and at one that keeps all of them (every stamp distinct: random 64-bit values), the same over a column
drawn from 8 distinct values (the position digits decide), and mi_knn_stamp_histogram with 120 edges.  The calls alternate in
one process, warm, median and min of --iters runs each.  Both calls are synchronous and run on the table's own stream, which a
caller cannot put events on: a figure is the host clock around the call (the upload of the query, the kernels, the wait, the
copy of one record) — an upper bound of its device time, the same for both sides of a ratio.  Writes
profiles/ordered_profile.json.

    python tools/knn_ordered_profile.py [--rows 10000000] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from image_search_amd import synth
    from image_search_amd.search import EmbeddingTable

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ordered_profile.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    ids = np.arange(a.rows, dtype=np.uint64)
    columns = {"distinct": rng.integers(-(1 << 63), (1 << 63) - 1, a.rows, dtype=np.int64, endpoint=True),
               "eight": rng.choice(np.array([-(1 << 62), -(1 << 40), -1, 0, 1, 1 << 20, 1 << 41, 1 << 62], np.int64), a.rows)}
    tables = {}
    for name, col in columns.items():
        t = EmbeddingTable(768, 0)
        t.insert_synthetic(3, 0, a.rows)
        t.set_attrs(ids, None, col)
        tables[name] = t
    q = synth.corpus_rows(1003, 0, 1)[0]
    inf = float("inf")

    # the bound that keeps about 1 % of the rows: bisection on the paged search's window count
    t = tables["distinct"]
    lo, hi = 0.0, 2.0
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        if t.knn_page(q, 1, None, mid)[2]["window"] < a.rows // 100:
            lo = mid
        else:
            hi = mid
    one_pct = float(np.float32(hi))
    kept = {"one_pct": int(t.knn_page(q, 1, None, one_pct)[2]["window"]), "all": int(t.knn_page(q, 1, None, inf)[2]["window"])}
    edges = np.linspace(-(2.0 ** 62), 2.0 ** 62, 120).astype(np.int64)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    cases = {
        "ordered_1pct": ("distinct", one_pct, lambda t, b: t.knn_ordered(q, a.k, b, True)),
        "ordered_100pct": ("distinct", inf, lambda t, b: t.knn_ordered(q, a.k, b, True)),
        "ordered_ties8_100pct": ("eight", inf, lambda t, b: t.knn_ordered(q, a.k, b, True)),
        "histogram_120_edges_100pct": ("distinct", inf, lambda t, b: t.stamp_histogram(q, edges, b)),
    }
    ms = {c: {"call": [], "page": []} for c in cases}
    for rep in range(3 + a.iters):   # three warm rounds (workspaces are allocated by the first call)
        for name, (table, bound, fn) in cases.items():   # alternate: drifts of the clock hit every case and both sides alike
            t = tables[table]
            page = clock(lambda: t.knn_page(q, a.k, None, bound))
            call = clock(lambda: fn(t, bound))
            if rep >= 3:
                ms[name]["page"].append(page)
                ms[name]["call"].append(call)
    out = {"rows": a.rows, "k": a.k, "iters": a.iters, "device": torch.cuda.get_device_name(0), "clock": "host, around the call",
           "max_dist_1pct": one_pct, "rows_within": kept, "cases": {}}
    for name in cases:
        call, page = np.array(ms[name]["call"]), np.array(ms[name]["page"])
        out["cases"][name] = {"ms_median": float(np.median(call)), "ms_min": float(call.min()),
                              "page_ms_median": float(np.median(page)), "page_ms_min": float(page.min()),
                              "ratio_to_page": float(np.median(call) / np.median(page))}
    for t in tables.values():
        t.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
