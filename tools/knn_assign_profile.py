"""What mi_knn_assign and mi_knn_kmeans cost: --rows synthetic rows against C Gaussian vectors.

    python tools/knn_assign_profile.py [--rows 1000000] [--out profiles/assign_profile.json]     # host clocks
    rocprofv3 --kernel-trace --stats -f csv -d TRACE -- python tools/knn_assign_profile.py --workload --c 1024
    python tools/knn_assign_profile.py --trace TRACE --c 1024          # adds device time per kernel and stage 1's rates

Host clock of an assign: median of 5 calls after 1 warm-up, per C in 16, 256, 1 024, 4 096, "prefilter" = 1 (the table keeps
the bf16 mirror, so no call builds one).  Baseline, the only route to the same labels before the assign existed: a table of
the C vectors searched with groups of 16 table rows through mi_knn_search_batched_device (k = 1), timed over 64 groups in
the same process, alternating with the assign, scaled by N / 16 (the row copies the route also needs are not charged).
k-means: one run of 10 iterations at C = 256, and the same call with max_iters = 0 (one assign) to split assign from update.
--workload runs one warm-up and two assigns for the trace; stage 1's rates = 2 N C dim flop against the 2.5 PFLOP/s bf16
peak and the mirror's N dim 2 bytes against the 8 TB/s HBM peak, over the summed time of assign_tiles_kernel.
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

DIM, PEAK_FLOPS, PEAK_HBM = 768, 2.5e15, 8e12
CS = (16, 256, 1024, 4096)


def vectors(C):
    return np.random.default_rng(C).standard_normal((C, DIM)).astype(np.float32)


def make_table(n):
    from image_search_amd.search import EmbeddingTable
    t = EmbeddingTable(DIM, 0)
    t.insert_synthetic(11, 0, n)
    t.set_option("prefilter", 1)
    return t


def host_clocks(n, cs, kmeans):
    import torch
    from image_search_amd.search import EmbeddingTable
    t = make_table(n)
    q = torch.from_numpy(t.rows(0, 16 * 64)).cuda().reshape(64, 16, DIM)
    idx = torch.zeros((16, 1), dtype=torch.int64, device="cuda")
    dist = torch.zeros((16, 1), dtype=torch.float32, device="cuda")
    res = {"rows": n}
    for C in cs:
        v = vectors(C)
        tv = EmbeddingTable(DIM, 0)
        tv.insert(v)

        def groups(first, count):
            t0 = time.perf_counter()
            for g in range(first, first + count):
                tv.knn_device(q[g].data_ptr(), 16, 1, idx.data_ptr(), dist.data_ptr(), 0, batched=True)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        groups(0, 4)
        t.assign(v)   # warm-up (the first one also builds the table's mirror)
        asg, base_s = [], 0.0
        for it in range(5):
            t0 = time.perf_counter()
            t.assign(v)
            asg.append(time.perf_counter() - t0)
            base_s += groups(it * 12, 12 if it < 4 else 16)   # 64 groups in all, alternating with the assign
        st = t.assign_stats()
        med = statistics.median(asg)
        res[f"C{C}"] = {"assign_host_s_median": med, "assign_host_s": asg, "candidates_per_row": st["candidates"] / n,
                        "launches": st["launches"], "baseline_s_per_group_of_16": base_s / 64,
                        "baseline_scaled_s": base_s / 64 * (n / 16), "ratio_baseline_over_assign": base_s / 64 * (n / 16) / med}
        tv.close()
    if kmeans:
        c0 = t.rows(0, 256)
        t.kmeans(c0, max_iters=1)
        t0 = time.perf_counter()
        one = t.kmeans(c0, max_iters=0)
        t1 = time.perf_counter()
        run = t.kmeans(c0, max_iters=10)
        t2 = time.perf_counter()
        # a run of i iterations = i + 1 assigns and i updates, plus the setup both calls share
        per_assign = t1 - t0
        res["kmeans_C256"] = {"iters": run["iters"], "run_s": t2 - t1, "one_assign_call_s": per_assign,
                              "update_s_per_iter": ((t2 - t1) - (run["iters"] + 1) * per_assign) / max(run["iters"], 1),
                              "objective_first_last": [one["objective"], run["objective"]], "changed_last": run["changed"]}
    t.close()
    return res


def workload(n, C):
    t = make_table(n)
    v = vectors(C)
    for _ in range(3):
        t.assign(v)
    print(t.assign_stats())
    t.close()


def read_trace(directory, n, C):
    per = {}
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"].split("(")[0]
            per[name] = per.get(name, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9
    tiles = sum(v for k, v in per.items() if "assign_tiles_kernel" in k) / 3   # the workload runs the assign three times
    return {"kernel_seconds_three_assigns": {k: v for k, v in sorted(per.items(), key=lambda kv: -kv[1]) if "assign_" in k or "mirror" in k},
            "stage1_s_per_assign": tiles, "stage1_fraction_of_bf16_peak": 2.0 * n * C * DIM / tiles / PEAK_FLOPS if tiles else None,
            "stage1_fraction_of_hbm_peak": 2.0 * n * DIM / tiles / PEAK_HBM if tiles else None}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--c", type=int, default=0, help="one C only (default: 16, 256, 1024, 4096)")
    ap.add_argument("--no-kmeans", action="store_true")
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_profile.json"))
    a = ap.parse_args()
    if a.workload:
        workload(a.rows, a.c or 1024)
        sys.exit(0)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    key = str(a.rows)
    res.setdefault(key, {})
    if a.trace:
        res[key][f"device_C{a.c or 1024}"] = read_trace(a.trace, a.rows, a.c or 1024)
    else:
        res[key].update(host_clocks(a.rows, (a.c,) if a.c else CS, not a.no_kmeans))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res[key]))
