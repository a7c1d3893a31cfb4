"""What DBSCAN costs on a sharded table beside the single table's: --rows synthetic rows + 20 planted clusters
of 500 adjacent rows each (tools/knn_density_profile.py's corpus), max_dist 0.1, min_pts 5.

    python tools/knn_sharded_density_profile.py [--rows 1000000]      # host clocks -> profiles/sharded_density_profile.json

EmbeddingTable.dbscan against ShardedTable.dbscan as 2 / 4 / 8 shards on ONE device, the calls alternating in one process,
medians of 5 after one warm-up each, on the host clock; every sharded result is compared with the single table's for equality.
The single table's dbscan is the yardstick.  Shards on one device share it: the figure is what the decomposition into
S self pieces and S (S - 1) / 2 shard pairs, the second forest pass and the host's scatter cost — not what several GPUs gain.
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

from knn_density_profile import CLUSTERS, DIM, MAX_DIST, MIN_PTS, PER, make_table   # noqa: E402

OUT = os.path.join(ROOT, "profiles", "sharded_density_profile.json")
SHARDS = (2, 4, 8)


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def same(x, y):
    return (all(np.array_equal(x[k], y[k]) for k in ("labels", "cluster", "via", "counts"))
            and np.array_equal(x["via_dist"].view(np.uint32), y["via_dist"].view(np.uint32)) and x["summary"] == y["summary"])


def host_clocks(n):
    from image_search_amd.search import ShardedTable
    one = make_table(n)
    total = n + CLUSTERS * PER
    planted = one.rows(n, CLUSTERS * PER)
    _, want = clock(lambda: one.dbscan(MAX_DIST, MIN_PTS))     # the warm-up
    res = {"rows": total, "max_dist": MAX_DIST, "min_pts": MIN_PTS, "summary": want["summary"], "single_stats": one.dbscan_stats(),
           "shards": {}}
    for shards in SHARDS:
        t = ShardedTable(DIM, [0] * shards)
        t.insert_synthetic(11, 0, n)
        t.insert(planted)
        _, got = clock(lambda: t.dbscan(MAX_DIST, MIN_PTS))    # the warm-up
        equal = same(got, want)
        single_s, sharded_s = [], []
        for _ in range(5):
            s, _ = clock(lambda: one.dbscan(MAX_DIST, MIN_PTS))
            single_s.append(s)
            s, got = clock(lambda: t.dbscan(MAX_DIST, MIN_PTS))
            sharded_s.append(s)
            equal = equal and same(got, want)
        res["shards"][str(shards)] = {"block_rows": t.info()["block_rows"], "equal_to_single": bool(equal),
                                      "single_host_s_median": statistics.median(single_s), "single_host_s": single_s,
                                      "sharded_host_s_median": statistics.median(sharded_s), "sharded_host_s": sharded_s,
                                      "ratio_sharded_over_single": statistics.median(sharded_s) / statistics.median(single_s),
                                      "stats": t.dbscan_stats()}
        t.close()
        print(shards, json.dumps(res["shards"][str(shards)]), flush=True)
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
    print(json.dumps(res[str(a.rows)]))
    if not all(v["equal_to_single"] for v in res[str(a.rows)]["shards"].values()):
        sys.exit("a sharded result differs from the single table's")
