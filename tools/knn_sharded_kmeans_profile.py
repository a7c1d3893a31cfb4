"""What k-means costs on the fixed-point sum and on a sharded table beside the single table's float sum:
--rows synthetic rows + 20 planted themes of 500 rows each (tools/knn_density_profile.py's corpus), C = 40 start rows picked
from a seed, 10 iterations.

    python tools/knn_sharded_kmeans_profile.py [--rows 1000000]      # host clocks -> profiles/sharded_kmeans_profile.json
    rocprofv3 --kernel-trace --stats -d DIR -o km -- python tools/knn_sharded_kmeans_profile.py --kernels
                                                                     # device time per kernel, in a run of its own

(a) EmbeddingTable.kmeans on the float sum, (b) the same table with "kmeans_fixed_sum" = 1, (c) ShardedTable.kmeans as
2 / 4 / 8 shards on ONE device — the calls alternating in one process, medians of 15 after one warm-up each, on the host
clock (a call lasts 30 .. 50 ms and other work shares the host: the fastest call is kept beside the median).
ms per iteration = (a call of 10 iterations - a call of 0 iterations) / 10: one assign and one update, without the mirror, the
norms and the download, which both calls pay once.  The update's share, for the single table: 1 - assign / iteration, the assign
clocked as EmbeddingTable.assign with the table's mirror kept ("prefilter" = 1), which still pays the download of labels and
dist — an upper bound of the assign, so a lower bound of the update.  Every fixed-sum result is compared with (b) for equality.
Shards on one device share it: (c) / (b) is what the decomposition, the exchange and the host's scatter cost, not what several
GPUs gain.
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

from knn_density_profile import CLUSTERS, DIM, PER, make_table   # noqa: E402

OUT = os.path.join(ROOT, "profiles", "sharded_kmeans_profile.json")
SHARDS = (2, 4, 8)
C, ITERS, REPEATS = 40, 10, 15


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def same(x, y):
    return (np.array_equal(x["centroids"].view(np.uint32), y["centroids"].view(np.uint32)) and np.array_equal(x["labels"], y["labels"])
            and np.array_equal(x["dist"].view(np.uint32), y["dist"].view(np.uint32)) and x["iters"] == y["iters"]
            and x["changed"] == y["changed"] and x["objective"] == y["objective"])


def per_iteration(full, zero, iters):
    return (statistics.median(full) - statistics.median(zero)) / max(iters, 1) * 1e3


def kernels(n):
    """the single table's two updates once each behind a warm-up, for a kernel trace: 2 x ITERS launches of km_sum_kernel and
    of km_sum_fixed_kernel and 2 x (ITERS + 1) assigns in both"""
    from image_search_amd.search import initial_centroid_rows
    one = make_table(n)
    c0 = np.concatenate([one.rows(int(r), 1) for r in initial_centroid_rows(n + CLUSTERS * PER, np.empty(0, np.uint64), C, 5)])
    for _ in range(2):
        for fixed in (False, True):
            print(fixed, one.kmeans(c0, max_iters=ITERS, fixed_sum=fixed)["iters"], flush=True)
    one.close()


def host_clocks(n):
    from image_search_amd.search import ShardedTable, initial_centroid_rows
    one = make_table(n)
    one.set_option("prefilter", 1)       # the mirror is kept: a call of 0 iterations is one assign and the download
    total = n + CLUSTERS * PER
    planted = one.rows(n, CLUSTERS * PER)
    c0 = np.concatenate([one.rows(int(r), 1) for r in initial_centroid_rows(total, np.empty(0, np.uint64), C, 5)])
    runs = {"float": lambda it: one.kmeans(c0, max_iters=it, fixed_sum=False), "fixed": lambda it: one.kmeans(c0, max_iters=it, fixed_sum=True)}
    want = {}
    for name, f in runs.items():         # the warm-ups
        f(0)
        want[name] = f(ITERS)
    one.assign(c0)
    clocks = {k: [] for k in ("float", "float0", "fixed", "fixed0", "assign")}
    for _ in range(REPEATS):
        for name, f in runs.items():
            clocks[name + "0"].append(clock(lambda: f(0))[0])
            clocks[name].append(clock(lambda: f(ITERS))[0])
        clocks["assign"].append(clock(lambda: one.assign(c0))[0])
    res = {"rows": total, "C": C, "max_iters": ITERS, "single": {}, "shards": {}}
    assign_ms = statistics.median(clocks["assign"]) * 1e3
    for name in runs:
        it_ms = per_iteration(clocks[name], clocks[name + "0"], want[name]["iters"])
        res["single"][name] = {"iters": want[name]["iters"], "changed": want[name]["changed"], "objective": want[name]["objective"],
                               "host_s": clocks[name], "host_s_zero_iters": clocks[name + "0"], "ms_per_iteration": it_ms,
                               "assign_ms_upper_bound": assign_ms, "update_ms_lower_bound": it_ms - assign_ms,
                               "update_share_lower_bound": (it_ms - assign_ms) / it_ms}
    res["single"]["update_fixed_over_float"] = (res["single"]["fixed"]["update_ms_lower_bound"]
                                                / res["single"]["float"]["update_ms_lower_bound"])
    res["single"]["largest_centroid_difference_fixed_vs_float"] = float(np.max(np.abs(want["fixed"]["centroids"] - want["float"]["centroids"])))
    print("single", json.dumps(res["single"]), flush=True)
    for shards in SHARDS:
        t = ShardedTable(DIM, [0] * shards)
        t.insert_synthetic(11, 0, n)
        t.insert(planted)
        t.kmeans(c0, max_iters=0)
        equal = same(t.kmeans(c0, max_iters=ITERS), want["fixed"])
        full, zero, single = [], [], []
        for _ in range(REPEATS):
            zero.append(clock(lambda: t.kmeans(c0, max_iters=0))[0])
            s, got = clock(lambda: t.kmeans(c0, max_iters=ITERS))
            full.append(s)
            equal = equal and same(got, want["fixed"])
            single.append(clock(lambda: runs["fixed"](ITERS))[0])
        it_ms = per_iteration(full, zero, want["fixed"]["iters"])
        res["shards"][str(shards)] = {"block_rows": t.info()["block_rows"], "equal_to_single_fixed": bool(equal), "host_s": full,
                                      "host_s_zero_iters": zero, "single_fixed_host_s": single, "ms_per_iteration": it_ms,
                                      "ratio_call_sharded_over_single_fixed": statistics.median(full) / statistics.median(single),
                                      "ratio_fastest_call_sharded_over_single_fixed": min(full) / min(single),
                                      "ratio_iteration_sharded_over_single_fixed": it_ms / res["single"]["fixed"]["ms_per_iteration"],
                                      "stats": t.kmeans_stats()}
        t.close()
        print(shards, json.dumps(res["shards"][str(shards)]), flush=True)
    one.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--kernels", action="store_true", help="only the single table's float and fixed k-means, for a kernel trace")
    a = ap.parse_args()
    if a.kernels:
        kernels(a.rows)
        sys.exit(0)
    res = json.load(open(OUT)) if os.path.exists(OUT) else {}
    res[str(a.rows)] = host_clocks(a.rows)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)
    print(json.dumps(res[str(a.rows)]))
    if not all(v["equal_to_single_fixed"] for v in res[str(a.rows)]["shards"].values()):
        sys.exit("a sharded result differs from the single table's")
