"""What DBSCAN at several distances in one pass costs beside the separate calls: --rows synthetic rows + 20
planted clusters of 500 adjacent rows each (tools/knn_density_profile.py's table), max_dists 0.05 / 0.1 / 0.15 / 0.2, min_pts 5.

    python tools/knn_density_levels_profile.py [--rows 1000000]      # host clocks -> profiles/density_levels_profile.json

dbscan_levels against the four separate dbscan calls and against the one dbscan at the top distance, all on the same table,
the calls alternating in one process, median of 5 after one warm-up each, on the host clock around the synchronous calls.
The derived expectation is about one dbscan at the top distance plus the extra stage-2 link work; the call must come out
below the sum of the separate calls to be worth having.  Every level is compared with its separate call for equality on the
way, so the times are those of the same answer.
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

from tools.knn_density_profile import CLUSTERS, PER, make_table  # noqa: E402

MAX_DISTS, MIN_PTS = (0.05, 0.1, 0.15, 0.2), 5
OUT = os.path.join(ROOT, "profiles", "density_levels_profile.json")


def host_clocks(n):
    t = make_table(n)
    total = n + CLUSTERS * PER

    def clock(f):
        t0 = time.perf_counter()
        out = f()
        return time.perf_counter() - t0, out

    clock(lambda: t.dbscan_levels(MAX_DISTS, MIN_PTS))
    for md in MAX_DISTS:
        clock(lambda: t.dbscan(md, MIN_PTS))
    levels_s, top_s, separate_s = [], [], [[] for _ in MAX_DISTS]
    same = True
    for _ in range(5):
        s, res = clock(lambda: t.dbscan_levels(MAX_DISTS, MIN_PTS))
        levels_s.append(s)
        stats = t.dbscan_stats()
        for l, md in enumerate(MAX_DISTS):
            s, one = clock(lambda: t.dbscan(md, MIN_PTS))
            separate_s[l].append(s)
            same = same and all(res[k][l].tobytes() == one[k].tobytes() for k in ("cluster", "via", "via_dist", "counts"))
            same = same and res["summary"][l] == one["summary"]
        top_stats = t.dbscan_stats()
        s, _ = clock(lambda: t.dbscan(MAX_DISTS[-1], MIN_PTS))
        top_s.append(s)
    t.close()
    separate_medians = [statistics.median(v) for v in separate_s]
    return {"rows": total, "max_dists": list(MAX_DISTS), "min_pts": MIN_PTS, "summary": res["summary"],
            "tree": [v.tolist() for v in res["tree"]], "levels_equal_the_separate_calls": bool(same),
            "dbscan_levels_host_s_median": statistics.median(levels_s), "dbscan_levels_host_s": levels_s,
            "dbscan_separate_host_s_median": separate_medians, "dbscan_separate_host_s": separate_s,
            "dbscan_separate_sum_host_s": sum(separate_medians),
            "dbscan_top_host_s_median": statistics.median(top_s), "dbscan_top_host_s": top_s,
            "ratio_levels_over_sum_of_separate": statistics.median(levels_s) / sum(separate_medians),
            "ratio_levels_over_top": statistics.median(levels_s) / statistics.median(top_s),
            "stats_levels": stats, "stats_top": top_stats}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    a = ap.parse_args()
    res = json.load(open(OUT)) if os.path.exists(OUT) else {}
    res[str(a.rows)] = host_clocks(a.rows)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)
    print(json.dumps(res[str(a.rows)]))
