"""What mi_knn_sharded_summarize costs beside the single table's call: --rows rows of 20 planted themes, dim
768 (the corpus of tools/knn_summary_profile.py).

    python tools/knn_sharded_summary_profile.py [--rows 1000000]      # host clocks -> profiles/sharded_summary_profile.json

One process.  EmbeddingTable.summarize with "kmeans_fixed_sum" = 1 alternating with ShardedTable.summarize as 2 / 4 / 8 shards
on ONE device (blocks of 4 096 rows), medians of 5 after one warm-up each, on the host clock, for two labelings: "themes" =
the 20 planted themes, "kmeans" = the labels of kmeans(1 000, 2 iterations).  Every sharded result is compared with the single
table's for equality.  Shards on one device share it: the ratio is what the decomposition, the exchange and the host's dealing
and scatter cost, not what several GPUs gain.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from knn_summary_profile import BLOCK, DIM, THEMES, build_table   # noqa: E402

OUT = os.path.join(ROOT, "profiles", "sharded_summary_profile.json")
SHARDS = (2, 4, 8)
BLOCK_ROWS, REPEATS = 4096, 5
ARRAYS = ("centroids", "count", "cover", "cover_dist", "odd", "odd_dist", "measured", "spread", "dist")


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def same(x, y):
    return all(np.array_equal(x[k].view(np.uint32) if x[k].dtype == np.float32 else x[k],
                              y[k].view(np.uint32) if y[k].dtype == np.float32 else y[k]) for k in ARRAYS) and x["totals"] == y["totals"]


def host_clocks(n):
    from image_search_amd.search import ShardedTable
    one, _, own = build_table(n)
    one.set_option("kmeans_fixed_sum", 1)
    labelings = {"themes": (own, THEMES), "kmeans": (one.kmeans(1000, max_iters=2, seed=0)["labels"], 1000)}
    want = {name: one.summarize(labels, C) for name, (labels, C) in labelings.items()}      # (the single table's warm-up too)
    res = {"rows": n, "dim": DIM, "block_rows": BLOCK_ROWS, "repeats": REPEATS, "shards": {}}
    for shards in SHARDS:
        t = ShardedTable(DIM, [0] * shards, BLOCK_ROWS)
        for first in range(0, n, BLOCK):
            t.insert(one.rows(first, min(BLOCK, n - first)))
        res["shards"][str(shards)] = {}
        for name, (labels, C) in labelings.items():
            equal = same(t.summarize(labels, C), want[name])                                # the warm-up
            sharded, single = [], []
            for _ in range(REPEATS):
                s, got = clock(lambda: t.summarize(labels, C))
                sharded.append(s)
                equal = equal and same(got, want[name])
                single.append(clock(lambda: one.summarize(labels, C))[0])
            res["shards"][str(shards)][name] = {"C": C, "equal_to_single_fixed": bool(equal), "host_s": sharded, "single_fixed_host_s": single,
                                                "ratio_sharded_over_single_fixed": statistics.median(sharded) / statistics.median(single),
                                                "ratio_fastest_sharded_over_single_fixed": min(sharded) / min(single),
                                                "stats": t.summarize_stats(), "single_stats": one.summarize_stats()}
            print(shards, name, json.dumps(res["shards"][str(shards)][name]), flush=True)
        t.close()
    one.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    a = ap.parse_args()
    res = json.load(open(OUT)) if os.path.exists(OUT) else {}
    res[str(a.rows)] = host_clocks(a.rows)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)
    if not all(v["equal_to_single_fixed"] for per in res[str(a.rows)]["shards"].values() for v in per.values()):
        sys.exit("a sharded result differs from the single table's")
