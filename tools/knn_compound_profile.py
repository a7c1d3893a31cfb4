"""What mi_knn_search_compound costs against the passes it is built like: --rows synthetic rows of dim 768,
T in {2, 4, 8} terms (one of them negative from T = 4 on) at k = 10 and k = 1000.

    python tools/knn_compound_profile.py [--rows 10000000] [--calls 10] [--out profiles/compound_profile.json]

Two child processes, each under its own time limit (--limit seconds):
  --measure   in ONE process, per (T, k), medians of --calls: the call (host wall time, upload and readback included); the
              yardsticks on the device clock (events around --calls launches): mi_knn_search_device for one query and
              mi_knn_search_batched_device with "prefilter" 0 for a group of T queries — the same loads and FMAs per row.
  --workload  the same calls once more under `rocprofv3 --kernel-trace`: the scan kernels alone (knn_compound_scan_kernel against
              knn_scan_batched_kernel / knn_scan_kernel), per dispatch, in launch order.
No threshold is asserted here; the numbers go to --out and into DESIGN.md 5.22.
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
CASES = [(T, k) for k in (10, 1000) for T in (2, 4, 8)]


def setup(rows):
    from image_search_amd.search import EmbeddingTable
    t = EmbeddingTable(DIM, 0)
    t.reserve(rows)
    t.insert_synthetic(21, 0, rows)
    t.set_option("prefilter", 0)
    rng = np.random.default_rng(0)
    terms = np.stack([t.rows(int(r), 1)[0] for r in rng.integers(0, rows, 8)]) + 0.5 * rng.standard_normal((8, DIM))
    return t, terms.astype(np.float32)


def compound(t, terms, T, k):
    """T terms: all positive up to 2, the last one negative (threshold 0.9: excludes a few rows of unrelated vectors) from 4 on"""
    if T <= 2:
        return t.knn_compound(terms[:T], "all", k=k)
    return t.knn_compound(terms[:T - 1], "all", terms[T - 1:T], [0.9], k=k)


def measure(a):
    import torch
    t, terms = setup(a.rows)
    d_q = torch.from_numpy(terms).cuda()
    st = torch.cuda.Stream()
    out = []
    for T, k in CASES:
        walls = []
        for it in range(2 + a.calls):
            t0 = time.perf_counter()
            compound(t, terms, T, k)
            if it >= 2:
                walls.append(time.perf_counter() - t0)
        case = {"terms": T, "k": k, "call_ms_median": 1e3 * statistics.median(walls), "call_ms_min": 1e3 * min(walls),
                "call_ms_max": 1e3 * max(walls), "stats": t.knn_compound_stats()}
        for name, nq, batched in (("search_1_query", 1, False), (f"batched_{T}_queries", T, True)):
            di = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            dd = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            for _ in range(2):
                t.knn_device(d_q.data_ptr(), nq, k, di.data_ptr(), dd.data_ptr(), st.cuda_stream, batched=batched)
            st.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.calls):
                t.knn_device(d_q.data_ptr(), nq, k, di.data_ptr(), dd.data_ptr(), st.cuda_stream, batched=batched)
            e1.record(st)
            st.synchronize()
            case[f"yardstick_{name}_ms"] = e0.elapsed_time(e1) / a.calls
        print(json.dumps(case), flush=True)
        out.append(case)
    t.close()
    return out


def workload(a):
    """for the trace: per case 3 compound calls, then 3 batched passes of T queries and 3 single searches"""
    import torch
    t, terms = setup(a.rows)
    d_q = torch.from_numpy(terms).cuda()
    st = torch.cuda.Stream()
    for T, k in CASES:
        for _ in range(3):
            compound(t, terms, T, k)
        di = torch.empty((T, k), dtype=torch.int64, device="cuda")
        dd = torch.empty((T, k), dtype=torch.float32, device="cuda")
        for nq, batched in ((T, True), (1, False)):
            for _ in range(3):
                t.knn_device(d_q.data_ptr(), nq, k, di.data_ptr(), dd.data_ptr(), st.cuda_stream, batched=batched)
            st.synchronize()
    t.close()


def scan_kernels(trace_dir):
    """rocprofv3 kernel trace -> [(kernel name, ms)] of the scan kernels in launch order"""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name", "")
            if "knn_compound_scan_kernel" in name or "knn_scan_batched_kernel" in name or "knn_scan_kernel" in name:
                rows.append((int(r["Start_Timestamp"]), name.split("(")[0], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    return [(n, ms) for _, n, ms in sorted(rows)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--limit", type=int, default=420, help="seconds each GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compound_profile.json"))
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
    prof = shutil.which("rocprofv3")
    if prof:
        trace = os.path.join(os.path.dirname(os.path.abspath(a.out)) or ".", "compound_trace")
        shutil.rmtree(trace, ignore_errors=True)
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), prof, "--kernel-trace", "--output-format", "csv", "-d", trace, "--"] + me + ["--workload"])
        if p.returncode != 0:
            raise SystemExit(f"the traced step ended with {p.returncode}")
        by_name = {}
        for name, ms in scan_kernels(trace):
            by_name.setdefault(name, []).append(round(ms, 4))
        res["scan_kernels_ms"] = by_name
        shutil.rmtree(trace, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res["scan_kernels_ms"], indent=1))
