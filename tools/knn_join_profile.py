"""What the threshold self-join costs: --rows synthetic rows + 1 000 planted copies-with-noise, max_dist 0.05.

    python tools/knn_join_profile.py [--rows 1000000]                 # host clocks -> profiles/join_profile.json
    rocprofv3 --kernel-trace --stats -f csv -d TRACE -- python tools/knn_join_profile.py --workload
    python tools/knn_join_profile.py --trace TRACE                    # adds device time per kernel and stage 1's rate

Host clock of the join: median of 5 calls after 1 warm-up.  Baseline, the only route to the same information before the
join existed: groups of 16 rows as queries through mi_knn_search_batched_device ("prefilter" = 2, k = 64), timed over 64
groups in the same process, alternating with the join, scaled by N / 16 / 64.  --workload runs one warm-up and one join for
the trace; stage 1's rate = N (N - 1) / 2 * 2 * dim flop over the summed time of join_tiles_kernel, as a fraction of the
2.5 PFLOP/s bf16 peak the README uses.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, PLANTED, MAX_DIST, PEAK = 768, 1000, 0.05, 2.5e15
OUT = os.path.join(ROOT, "profiles", "join_profile.json")


def make_table(n):
    from image_search_amd.search import EmbeddingTable
    t = EmbeddingTable(DIM, 0)
    t.insert_synthetic(11, 0, n)
    rng = np.random.default_rng(11)
    src = np.sort(rng.choice(n, PLANTED, replace=False))
    base = np.stack([t.rows(int(r), 1)[0] for r in src])
    sigma = np.linspace(0.0, 0.4, PLANTED)[:, None] * np.abs(base).mean()
    t.insert(((base + sigma * rng.standard_normal((PLANTED, DIM))) * rng.uniform(0.1, 10.0, (PLANTED, 1))).astype(np.float32))
    return t


def host_clocks(n):
    import torch
    t = make_table(n)
    total = n + PLANTED
    t.set_option("prefilter", 2)
    q = torch.from_numpy(t.rows(0, 16 * 64)).cuda().reshape(64, 16, DIM)
    idx = torch.zeros((16, 64), dtype=torch.int64, device="cuda")
    dist = torch.zeros((16, 64), dtype=torch.float32, device="cuda")

    def groups(first, count):
        t0 = time.perf_counter()
        for g in range(first, first + count):
            t.knn_device(q[g].data_ptr(), 16, 64, idx.data_ptr(), dist.data_ptr(), 0, batched=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    groups(0, 4)
    t.near_pairs(MAX_DIST)   # warm-up (builds the join's own mirror once more per call: "prefilter" = 2 keeps bytes)
    join_s, base_s = [], 0.0
    for it in range(5):
        t0 = time.perf_counter()
        a, b, d = t.near_pairs(MAX_DIST)
        join_s.append(time.perf_counter() - t0)
        base_s += groups(it * 12, 12 if it < 4 else 16)   # 64 groups in all, alternating with the join
    stats = t.near_pairs_stats()
    baseline_scaled = base_s / 64 * (total / 16)
    t.close()
    return {"rows": total, "max_dist": MAX_DIST, "join_host_s_median": statistics.median(join_s), "join_host_s": join_s,
            "baseline_s_per_group_of_16": base_s / 64, "baseline_scaled_s": baseline_scaled,
            "ratio_baseline_over_join": baseline_scaled / statistics.median(join_s), "pairs": int(a.size), "stats": stats}


def workload(n):
    t = make_table(n)
    t.near_pairs(MAX_DIST)
    t.near_pairs(MAX_DIST)
    print(t.near_pairs_stats())
    t.close()


def read_trace(directory, n):
    per = {}
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"].split("(")[0]
            per[name] = per.get(name, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9
    tiles = sum(v for k, v in per.items() if "join_tiles_kernel" in k) / 2   # the workload runs the join twice
    total = n + PLANTED
    flop = total * (total - 1) / 2 * 2 * DIM
    return {"kernel_seconds_two_joins": {k: v for k, v in sorted(per.items(), key=lambda kv: -kv[1]) if "join_" in k or "mirror" in k},
            "stage1_s_per_join": tiles, "stage1_fraction_of_peak": flop / tiles / PEAK if tiles else None}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--trace")
    a = ap.parse_args()
    if a.workload:
        workload(a.rows)
        sys.exit(0)
    res = json.load(open(OUT)) if os.path.exists(OUT) else {}
    key = str(a.rows)
    res.setdefault(key, {})
    if a.trace:
        res[key]["device"] = read_trace(a.trace, a.rows)
    else:
        res[key].update(host_clocks(a.rows))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(res, open(OUT, "w"), indent=1)
    print(json.dumps(res[key]))
