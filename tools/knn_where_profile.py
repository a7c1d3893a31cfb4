"""What mi_knn_search_where costs against the filtered call over the same ids: --rows synthetic rows of dim
768, k = 10, predicates that keep 0.1 / 1 / 10 / 100 % of the rows.

    python tools/knn_where_profile.py [--rows 10000000] [--calls 20] [--out profiles/where_profile.json]

Two child processes, each under its own time limit (--limit seconds):
  --measure   in ONE process, per selectivity, yardstick and new call alternating, medians of --calls timings.  Every call is
              synchronous on the handle's own stream (upload, kernels, readback, wait), so a call is timed on the host around
              that one call, the same on both sides; the kernels alone come from the trace below.
                filtered   mi_knn_search_filtered(k, ids = the qualifying rows, an array the caller already holds) — the
                           yardstick: the host checks and orders the ids, uploads the list, runs the gathered search
                where      mi_knn_search_where(k, the predicate): the list is built on the device, the same gathered search
              Both answers are compared for equality before anything is timed.
  --workload  the same calls once more under `rocprofv3 --kernel-trace`: per kernel name, the durations.
No threshold is asserted here; the numbers go to --out and into DESIGN.md 5.25.  The expectation to hold them against: the two
predicate passes read about 2 x 17-21 B per row (0.4 GB at 10 M rows: some tens of microseconds), the gathered kernels are the
filtered call's own, so the new call should undercut the filtered call at every selectivity, at 100 % by the 24 ms of host
preparation and upload DESIGN.md 5.14 reports.
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

DIM, K = 768, 10
# the stamp column holds row % 1000: a range of m stamps keeps m / 1000 of the rows, spread over the whole table
CASES = [("0.1%", (0, 0)), ("1%", (0, 9)), ("10%", (0, 99)), ("100%", (None, None))]


def setup(rows):
    from image_search_amd.search import EmbeddingTable
    t = EmbeddingTable(DIM, 0)
    t.reserve(rows)
    t.insert_synthetic(21, 0, rows)
    t.set_option("prefilter", 0)
    ids = np.arange(rows, dtype=np.uint64)
    t.set_attrs(ids, tags=np.ones(rows, np.uint64), stamps=(ids % 1000).astype(np.int64))
    rng = np.random.default_rng(0)
    q = t.rows(int(rng.integers(0, rows)), 1)[0] + 0.5 * rng.standard_normal(DIM)
    return t, q.astype(np.float32)


def timed(calls, n):
    walls = {name: [] for name, _ in calls}
    for it in range(2 + n):                    # alternating: filtered, where, filtered, ...
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
    case["where_over_filtered"] = case["where_ms_median"] / case["filtered_ms_median"]
    return case


def measure(a):
    t, q = setup(a.rows)
    for name, stamp in CASES:
        ids = t.rows_where(all_of=1, stamp=stamp)
        f = t.knn(q, K, within=ids)
        w = t.knn_where(q, K, all_of=1, stamp=stamp)
        same = bool(np.array_equal(f[0], w[0]) and np.array_equal(f[1].view(np.uint32), w[1].view(np.uint32)))
        case = {"keeps": name, "matched": int(w[2]), "k": K, "same_as_filtered": same}
        case.update(timed([("filtered", lambda: t.knn(q, K, within=ids)), ("where", lambda: t.knn_where(q, K, all_of=1, stamp=stamp))],
                          a.calls))
        print(json.dumps(case), flush=True)
    t.close()


def workload(a):
    """for the trace: per selectivity, 3 rounds of the two calls"""
    t, q = setup(a.rows)
    for name, stamp in CASES:
        ids = t.rows_where(all_of=1, stamp=stamp)
        for _ in range(3):
            t.knn(q, K, within=ids)
            t.knn_where(q, K, all_of=1, stamp=stamp)
    t.close()


WATCH = ("where_count_kernel", "where_offsets_kernel", "where_emit_kernel", "knn_scan_gather", "knn_select", "knn_merge", "knn_finalize")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "where_profile.json"))
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
    me = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--calls", str(a.calls)]
    res = {"rows": a.rows, "dim": DIM, "calls": a.calls, "cases": [], "kernels_ms": None}
    p = subprocess.run(["timeout", "-k", "10", str(a.limit)] + me + ["--measure"], stdout=subprocess.PIPE, text=True)
    res["cases"] = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)   # the call times are kept whatever becomes of the trace
    if p.returncode != 0:
        raise SystemExit(f"the measuring step ended with {p.returncode}")   # nothing more is started on the GPU
    prof = shutil.which("rocprofv3")
    if prof and not a.no_trace:
        trace = os.path.join(os.path.dirname(os.path.abspath(a.out)) or ".", "where_trace")
        shutil.rmtree(trace, ignore_errors=True)
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), prof, "--kernel-trace", "--output-format", "csv", "-d", trace, "--"] + me + ["--workload"])
        if p.returncode != 0:
            raise SystemExit(f"the traced step ended with {p.returncode}")
        res["kernels_ms"] = kernels(trace)
        shutil.rmtree(trace, ignore_errors=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))
