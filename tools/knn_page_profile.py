"""What mi_knn_search_page costs against the single pass it is built like: --rows synthetic rows of dim 768,
k in {10, 64, 100, 1000}.

    python tools/knn_page_profile.py [--rows 10000000] [--calls 10] [--out profiles/page_profile.json]

Two child processes, each under its own time limit (--limit seconds):
  --measure   in ONE process, per k, old and new calls alternating, medians of --calls host wall times (upload, readback and
              the wait included on both sides): mi_knn_search with "prefilter" 0 — the yardstick: the page scan issues that
              pass's loads and FMAs per row — against mi_knn_search_page for page 1, for the page behind it (a cursor), and
              for a page with a distance bound.
  --workload  the same calls once more under `rocprofv3 --kernel-trace`: the scan kernels alone (knn_page_scan_kernel against
              knn_scan_kernel), per dispatch, in launch order.
No threshold is asserted here; the numbers go to --out and into DESIGN.md 5.23.  The expectation to hold them against: the page
is not slower than the single pass by more than the +- 2.5 % two machines of one pool differ by.
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

DIM = 768
KS = (10, 64, 100, 1000)


def setup(rows):
    from image_search_amd.search import EmbeddingTable
    t = EmbeddingTable(DIM, 0)
    t.reserve(rows)
    t.insert_synthetic(21, 0, rows)
    t.set_option("prefilter", 0)
    rng = np.random.default_rng(0)
    q = t.rows(int(rng.integers(0, rows)), 1)[0] + 0.5 * rng.standard_normal(DIM)
    return t, q.astype(np.float32)


def forms(t, q, k):
    """name -> call, the yardstick first; the cursor is page 1's last hit, the bound the distance of its middle hit"""
    idx, dist, counts, nxt = t.knn_page(q, k)
    bound = float(dist[k // 2])
    return [("search", lambda: t.knn(q, k)),
            ("page_1", lambda: t.knn_page(q, k)),
            ("page_2", lambda: t.knn_page(q, k, after=nxt)),
            ("page_bound", lambda: t.knn_page(q, k, max_dist=bound))]


def measure(a):
    t, q = setup(a.rows)
    for k in KS:
        calls = forms(t, q, k)
        walls = {name: [] for name, _ in calls}
        for it in range(2 + a.calls):          # alternating: search, page, page, page, search, ...
            for name, fn in calls:
                t0 = time.perf_counter()
                fn()
                if it >= 2:
                    walls[name].append(time.perf_counter() - t0)
        case = {"k": k}
        for name, w in walls.items():
            case[name + "_ms_median"] = 1e3 * statistics.median(w)
            case[name + "_ms_min"] = 1e3 * min(w)
            case[name + "_ms_max"] = 1e3 * max(w)
        case["page_1_over_search"] = case["page_1_ms_median"] / case["search_ms_median"]
        case["page_2_over_search"] = case["page_2_ms_median"] / case["search_ms_median"]
        # the results the timed calls gave: page 1 is the search's list
        s_idx, s_dist = t.knn(q, k)
        p_idx, p_dist, counts, _ = t.knn_page(q, k)
        case["page_1_equals_search"] = bool(np.array_equal(s_idx, p_idx) and np.array_equal(s_dist.view(np.uint32), p_dist.view(np.uint32)))
        case["counts"] = counts
        print(json.dumps(case), flush=True)
    t.close()


def workload(a):
    """for the trace: per k, 3 rounds of the four calls"""
    t, q = setup(a.rows)
    for k in KS:
        calls = forms(t, q, k)
        for _ in range(3):
            for _, fn in calls:
                fn()
    t.close()


def scan_kernels(trace_dir):
    """rocprofv3 kernel trace -> [(kernel name, ms)] of the scan kernels in launch order"""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name", "")
            if "knn_page_scan_kernel" in name or "knn_scan_kernel" in name:
                rows.append((int(r["Start_Timestamp"]), name.split("(")[0], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    return [(n, ms) for _, n, ms in sorted(rows)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--limit", type=int, default=420, help="seconds each GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "page_profile.json"))
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
    res = {"rows": a.rows, "dim": DIM, "calls": a.calls, "cases": [], "scan_kernels_ms": None}
    p = subprocess.run(["timeout", "-k", "10", str(a.limit)] + me + ["--measure"], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise SystemExit(f"the measuring step ended with {p.returncode}")
    res["cases"] = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)   # the call times are kept whatever becomes of the trace
    prof = shutil.which("rocprofv3")
    if prof:
        trace = os.path.join(os.path.dirname(os.path.abspath(a.out)) or ".", "page_trace")
        shutil.rmtree(trace, ignore_errors=True)
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), prof, "--kernel-trace", "--output-format", "csv", "-d", trace, "--"] + me + ["--workload"])
        if p.returncode != 0:
            raise SystemExit(f"the traced step ended with {p.returncode}")
        by_name = {}
        for name, ms in scan_kernels(trace):
            by_name.setdefault(name, []).append(round(ms, 4))
        res["scan_kernels_ms"] = by_name
        shutil.rmtree(trace, ignore_errors=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({"cases": res["cases"], "scan_kernels_ms": res["scan_kernels_ms"]}, indent=1))
