"""What mi_knn_search_grouped costs against the page call it shares its scan and its select with: --rows
synthetic rows of dim 768, k = 100, five groupings.

    python tools/knn_grouped_profile.py [--rows 10000000] [--calls 20] [--out profiles/grouped_profile.json]

Two child processes, each under its own time limit (--limit seconds):
  --measure   in ONE process, per grouping, yardstick and new calls alternating, medians of --calls timings.  Every call is
              synchronous on the handle's own stream (upload, kernels, readback, wait), so a call is timed on the host around
              that one call, the same on both sides; the kernels alone come from the trace below.
                page            mi_knn_search_page(k, no cursor) with "prefilter" 0 — the yardstick: the same scan, the same select
                grouped         mi_knn_search_grouped(k)
                grouped_facets  ... with the facets asked for (one more copy of 4 n_groups bytes)
                grouped_global  ... with "group_lds_max" = 0 where the default takes the LDS form (the other reduce form)
              and once, on a 2-shard table on one device holding the same rows: page against grouped.
  --workload  the same calls once more under `rocprofv3 --kernel-trace`: per kernel name and grouping, the durations.
No threshold is asserted here; the numbers go to --out and into DESIGN.md 5.24.  The expectation to hold them against: the
grouped call moves 12 B per row more than the scan's 3 072 B, so time above the page call by more than 10 % is not bytes.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, K = 768, 100
NO_GROUP = 0xFFFFFFFF


def groupings(rows):
    """name -> the column, one id per row"""
    rng = np.random.default_rng(1)
    heavy = rng.integers(1, 16, rows, dtype=np.uint32)
    heavy[rng.random(rows) < 0.82] = 0
    return [("16_uniform", rng.integers(0, 16, rows, dtype=np.uint32)),
            ("1000_uniform", rng.integers(0, 1000, rows, dtype=np.uint32)),
            ("1e6_uniform", rng.integers(0, 1_000_000, rows, dtype=np.uint32)),
            ("all_singletons", np.full(rows, NO_GROUP, np.uint32)),
            ("16_one_heavy", heavy)]


def setup(rows, sharded=False):
    from image_search_amd.search import EmbeddingTable, ShardedTable
    t = ShardedTable(DIM, devices=(0, 0)) if sharded else EmbeddingTable(DIM, 0)
    t.reserve(rows)
    t.insert_synthetic(21, 0, rows)
    t.set_option("prefilter", 0)
    rng = np.random.default_rng(0)
    q = t.rows(int(rng.integers(0, rows)), 1)[0] + 0.5 * rng.standard_normal(DIM)
    return t, q.astype(np.float32)


def forms(t, q, lds_form):
    calls = [("page", lambda: t.knn_page(q, K)),
             ("grouped", lambda: t.knn_grouped(q, K)),
             ("grouped_facets", lambda: t.knn_grouped(q, K, facets=True))]
    if lds_form:
        def other():
            t.set_option("group_lds_max", 0)
            try:
                return t.knn_grouped(q, K)
            finally:
                t.set_option("group_lds_max", 4096)
        calls.append(("grouped_global", other))
    return calls


def timed(calls, n):
    walls = {name: [] for name, _ in calls}
    for it in range(2 + n):                    # alternating: page, grouped, ..., page, ...
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            if it >= 2:
                walls[name].append(time.perf_counter() - t0)
    case = {}
    for name, w in walls.items():
        case[name + "_ms_median"] = 1e3 * statistics.median(w)
        case[name + "_ms_min"] = 1e3 * min(w)
        case[name + "_ms_max"] = 1e3 * max(w)
    for name in walls:
        if name != "page":
            case[name + "_over_page"] = case[name + "_ms_median"] / case["page_ms_median"]
    return case


def measure(a):
    t, q = setup(a.rows)
    cols = groupings(a.rows)
    for name, col in cols:
        t.set_groups(col)
        n_groups = int(col[col != NO_GROUP].max()) + 1 if np.any(col != NO_GROUP) else 0
        case = {"grouping": name, "n_groups": n_groups, "k": K}
        case.update(timed(forms(t, q, 0 < n_groups <= 4096), a.calls))
        idx, dist, group, members, totals = t.knn_grouped(q, K)
        case["totals"] = totals
        case["hits"] = int((idx != np.uint64(0xFFFFFFFFFFFFFFFF)).sum())
        print(json.dumps(case), flush=True)
    t.close()
    if not a.no_sharded:
        t, q = setup(a.rows, sharded=True)
        t.set_groups(cols[1][1])
        case = {"grouping": "1000_uniform", "shards": 2, "k": K}
        case.update(timed([("page", lambda: t.knn_page(q, K)), ("grouped", lambda: t.knn_grouped(q, K)),
                           ("grouped_facets", lambda: t.knn_grouped(q, K, facets=True))], a.calls))
        print(json.dumps(case), flush=True)
        t.close()


def workload(a):
    """for the trace: per grouping, 3 rounds of the calls"""
    t, q = setup(a.rows)
    for name, col in groupings(a.rows):
        t.set_groups(col)
        n_groups = int(col[col != NO_GROUP].max()) + 1 if np.any(col != NO_GROUP) else 0
        for _ in range(3):
            for _, fn in forms(t, q, 0 < n_groups <= 4096):
                fn()
    t.close()


WATCH = ("knn_page_scan_kernel", "group_reduce_kernel", "group_mark_kernel", "group_finish_kernel", "knn_select", "knn_merge",
         "knn_page_finish_kernel")


def kernels(trace_dir):
    """rocprofv3 kernel trace -> {kernel name: [ms] in launch order} of the kernels the two calls are made of"""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name", "")
            if any(w in name for w in WATCH):
                rows.append((int(r["Start_Timestamp"]), name.split("(")[0], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    by_name = {}
    for _, n, ms in sorted(rows):
        by_name.setdefault(n, []).append(round(ms, 4))
    return by_name


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--limit", type=int, default=420, help="seconds each GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_profile.json"))
    ap.add_argument("--no-sharded", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--workload", action="store_true")
    a = ap.parse_args()
    if a.measure:
        measure(a)
        sys.exit(0)
    if a.workload:
        workload(a)
        sys.exit(0)
    me = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--calls", str(a.calls)] + (["--no-sharded"] if a.no_sharded else [])
    res = {"rows": a.rows, "dim": DIM, "calls": a.calls, "cases": [], "kernels_ms": None}
    p = subprocess.run(["timeout", "-k", "10", str(a.limit)] + me + ["--measure"], stdout=subprocess.PIPE, text=True)
    res["cases"] = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)   # the call times are kept whatever becomes of the trace
    if p.returncode != 0:
        raise SystemExit(f"the measuring step ended with {p.returncode}")   # nothing more is started on the GPU
    prof = shutil.which("rocprofv3")
    if prof and not a.no_trace:
        trace = os.path.join(os.path.dirname(os.path.abspath(a.out)) or ".", "grouped_trace")
        shutil.rmtree(trace, ignore_errors=True)
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), prof, "--kernel-trace", "--output-format", "csv", "-d", trace, "--"] + me + ["--workload"])
        if p.returncode != 0:
            raise SystemExit(f"the traced step ended with {p.returncode}")
        res["kernels_ms"] = kernels(trace)
        shutil.rmtree(trace, ignore_errors=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))
