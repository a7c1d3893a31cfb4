"""What DBSCAN on the join's tiles costs beside the join itself: --rows synthetic rows + 20 planted clusters of
500 adjacent rows each (a burst's rows are adjacent), max_dist 0.1, min_pts 5.

    python tools/knn_density_profile.py [--rows 1000000]              # host clocks -> profiles/density_profile.json

dbscan against near_pairs at the same max_dist on the same table, the calls alternating in one process, median of 5 after
one warm-up each, on the host clock.  The derived expectation is two tile passes — about twice near_pairs' time — less
whatever pass 2 skips; the ratio and the skipped share of pass 2's tiles are what 5.27 quotes.  neighbor_counts (pass 1
alone) is timed the same way.
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

DIM, CLUSTERS, PER, MAX_DIST, MIN_PTS = 768, 20, 500, 0.1, 5
OUT = os.path.join(ROOT, "profiles", "density_profile.json")


def make_table(n):
    from image_search_amd.search import EmbeddingTable
    t = EmbeddingTable(DIM, 0)
    t.insert_synthetic(11, 0, n)
    rng = np.random.default_rng(11)
    src = np.sort(rng.choice(n, CLUSTERS, replace=False))
    for r in src:
        c = t.rows(int(r), 1)[0]
        sigma = 0.25 * np.sqrt(np.mean(c * c))            # member to member about 0.06
        t.insert(((c + sigma * rng.standard_normal((PER, DIM))) * rng.uniform(0.1, 10.0, (PER, 1))).astype(np.float32))
    return t


def host_clocks(n):
    t = make_table(n)
    total = n + CLUSTERS * PER

    def clock(f):
        t0 = time.perf_counter()
        out = f()
        return time.perf_counter() - t0, out

    cap = 1 << 22
    clock(lambda: t.near_pairs(MAX_DIST, cap=cap))
    clock(lambda: t.dbscan(MAX_DIST, MIN_PTS))
    clock(lambda: t.neighbor_counts(MAX_DIST))
    join_s, dbscan_s, density_s = [], [], []
    for _ in range(5):
        s, pairs = clock(lambda: t.near_pairs(MAX_DIST, cap=cap))
        join_s.append(s)
        s, res = clock(lambda: t.dbscan(MAX_DIST, MIN_PTS))
        dbscan_s.append(s)
        stats = t.dbscan_stats()
        s, _ = clock(lambda: t.neighbor_counts(MAX_DIST))
        density_s.append(s)
    t.close()
    tiles2 = stats["tiles_visited"] + stats["tiles_skipped"]
    return {"rows": total, "max_dist": MAX_DIST, "min_pts": MIN_PTS, "pairs": int(pairs[0].size), "summary": res["summary"],
            "near_pairs_host_s_median": statistics.median(join_s), "near_pairs_host_s": join_s,
            "dbscan_host_s_median": statistics.median(dbscan_s), "dbscan_host_s": dbscan_s,
            "neighbor_counts_host_s_median": statistics.median(density_s), "neighbor_counts_host_s": density_s,
            "ratio_dbscan_over_near_pairs": statistics.median(dbscan_s) / statistics.median(join_s),
            "ratio_neighbor_counts_over_near_pairs": statistics.median(density_s) / statistics.median(join_s),
            "pass2_tiles_skipped_share": stats["tiles_skipped"] / tiles2 if tiles2 else None, "stats": stats}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    a = ap.parse_args()
    res = json.load(open(OUT)) if os.path.exists(OUT) else {}
    res[str(a.rows)] = host_clocks(a.rows)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)
    print(json.dumps(res[str(a.rows)]))
