"""What a filtered search costs: 10 M synthetic rows, k = 10 and k = 1000, filters of 100 / 10 / 1 / 0.1 %
of the rows (10 / 1 / 0.1 % as scattered ids and as one contiguous run; 100 % is one list either way), against the unfiltered
single pass.

mi_knn_search_filtered runs on the table's own stream and waits for its results, so a caller cannot put device events
around it.  Device time comes from a kernel and memory-copy trace of a fixed workload instead:

    rocprofv3 --kernel-trace --memory-copy-trace -f csv -d TRACE -- python tools/knn_filter_profile.py --workload
    python tools/knn_filter_profile.py --trace TRACE            # host clocks, then the trace -> profiles/filter_profile.json

--workload runs every case (3 warm-up calls, then --iters calls of one query each) between two marker kernels of torch
(a fill before, a multiply after), so the trace splits into cases; every search ends with knn_finalize_kernel, so a case
splits into calls.  Per call: `kernels` = the summed durations of its kernels, the runtime's memset / copy kernels included
(the device's work; the single pass's figure is the same sum over its own kernels); `h2d` = its host-to-device copies in
the copy trace (for a filtered call the list, 4 bytes per row, from pinned memory).  Medians and mins over the calls.
Host clocks (no trace): `prep` = a filtered call with no query (the host's id preparation alone); `call` = one query, start to
results.  Then the host time of folder resolution at 1 M paths (mi_index_search_within against mi_knn_search_filtered over the
same rows).

    python tools/knn_filter_profile.py [--rows 10000000] [--iters 20] [--workload | --trace DIR]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


CASES_K = (10, 1000)


def make_filters(n):
    rng = np.random.default_rng(1)
    filters = {"all_1.0": rng.permutation(n).astype(np.uint64)}
    for f in (0.1, 0.01, 0.001):
        m = int(n * f)
        filters[f"scattered_{f}"] = rng.permutation(n)[:m].astype(np.uint64)
        start = (n - m) // 2
        filters[f"contiguous_{f}"] = np.arange(start, start + m, dtype=np.uint64)
    return filters


def plan(filters):
    """the cases of --workload, in order: (k, name); name "single" = the unfiltered search"""
    return [(k, name) for k in CASES_K for name in ["single"] + list(filters)]


def read_trace(d):
    """rocprofv3 csv output -> kernels [(start, end, name)], host-to-device copies [(start, end)], both by start"""
    kf = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    mf = glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True)
    if not kf:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    kern = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for f in kf for r in csv.DictReader(open(f)))
    h2d = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for f in mf for r in csv.DictReader(open(f))
                 if any("HOST_TO_DEVICE" in str(v) for v in r.values()))
    return kern, h2d


def split_trace(kern, h2d, cases):
    """per case: per call {kernels, h2d} in ms, from the marker kernels around each case's timed calls"""
    out, i, c = {}, 0, 0
    while i < len(kern) and c < len(cases):
        if "FillFunctor" not in kern[i][2]:   # (the runtime's own fill and copy kernels belong to the calls)
            i += 1
            continue
        j = i + 1   # the case's calls run until the multiply marker
        while j < len(kern) and "at::native" not in kern[j][2]:
            j += 1
        calls, cur = [], []
        for s, e, name in kern[i + 1:j]:
            cur.append((s, e))
            if "knn_finalize_kernel" in name:
                t1 = cur[-1][1]
                # the call's copies: from the previous call's end (or the marker) to its finalize
                lo = calls[-1]["_end"] if calls else kern[i][1]
                cp = sum(ce - cs for cs, ce in h2d if lo <= cs < t1)
                calls.append({"kernels": sum(b - a for a, b in cur) * 1e-6, "h2d": cp * 1e-6, "_end": t1})
                cur = []
        out[cases[c]] = calls
        c += 1
        i = j + 1
    return out


def med_min(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min())}


def main():
    import torch

    from image_search_amd import synth
    from image_search_amd.search import EmbeddingTable, ImageIndex

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--paths", type=int, default=1_000_000)
    ap.add_argument("--workload", action="store_true", help="the traced workload only (run it under rocprofv3)")
    ap.add_argument("--trace", default=None, help="rocprofv3 output directory of a --workload run: device times from it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_profile.json"))
    a = ap.parse_args()
    n = a.rows
    t = EmbeddingTable(768, 0)
    t.insert_synthetic(3, 0, n)
    q = synth.corpus_rows(1003, 0, 1)
    none = np.zeros((0, 768), np.float32)
    filters = make_filters(n)
    cases = plan(filters)

    def search(k, name):
        return t.knn(q, k) if name == "single" else t.knn(q, k, within=filters[name])

    if a.workload:
        m = torch.empty(1, device="cuda")   # (empty: no kernel before the first marker)
        for k, name in cases:
            for _ in range(3):   # warm-up: code objects, workspaces
                search(k, name)
            torch.cuda.synchronize()
            m.fill_(1.0)         # marker: the case starts
            torch.cuda.synchronize()
            for _ in range(a.iters):
                search(k, name)
            m.mul_(2.0)          # marker: the case ends
            torch.cuda.synchronize()
        t.close()
        return

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    out = {"rows": n, "iters": a.iters, "device": torch.cuda.get_device_name(0), "ms": {}}
    for k in CASES_K:
        for _ in range(3):
            for name in ["single"] + list(filters):
                search(k, name)
        res = {name: {"call": [], "prep": []} for name in ["single"] + list(filters)}
        for _ in range(a.iters):  # alternate: drifts of the clock hit every case alike
            for name in res:
                res[name]["call"].append(wall(lambda: search(k, name)))
                if name != "single":
                    res[name]["prep"].append(wall(lambda: t.knn(none, k, within=filters[name])))
        out["ms"][f"k{k}"] = {name: {"rows": n if name == "single" else int(filters[name].size), "host_call": med_min(r["call"]),
                                     **({"host_prep": med_min(r["prep"])} if r["prep"] else {})} for name, r in res.items()}
    t.close()
    if a.trace:
        kern, h2d = read_trace(a.trace)
        per_case = split_trace(kern, h2d, cases)
        out["trace"] = "rocprofv3 --kernel-trace --memory-copy-trace of --workload"
        for (k, name), calls in per_case.items():
            cur = out["ms"][f"k{k}"][name]
            for key in ("kernels", "h2d"):
                cur["device_" + key] = med_min([c[key] for c in calls])
            cur["device_calls"] = len(calls)
            kt = cur["device_kernels"]["median"]
            cur["rows_read_TBps"] = cur["rows"] * 768 * 4 / (kt * 1e-3) / 1e12
        for k in CASES_K:
            base = out["ms"][f"k{k}"]["single"]
            for name, cur in out["ms"][f"k{k}"].items():
                if name != "single" and "device_kernels" in cur:
                    cur["kernels_vs_single"] = cur["device_kernels"]["median"] / base["device_kernels"]["median"] - 1.0

    # folder resolution at 1 M paths: 1000 folders of 1000 images each; a folder = 0.1 % of the rows
    ix = ImageIndex(768, 0, "/m/")
    ix.table.insert_synthetic(4, 0, a.paths)
    per = 1000
    ix.adopt([f"/m/f{j // per:04d}/img{j % per}.jpg" for j in range(a.paths)])
    ids = np.arange(500 * per, 501 * per, dtype=np.uint64)
    for _ in range(3):
        ix.web_search_text(q[0], (), 10, folders=["media/f0500"])
        ix.table.knn(q[0], 10, within=ids)
    w_f, w_i = [], []
    for _ in range(a.iters):
        w_f.append(wall(lambda: ix.web_search_text(q[0], (), 10, folders=["media/f0500"])))
        w_i.append(wall(lambda: ix.table.knn(q[0], 10, within=ids)))
    out["folders_1M_paths"] = {"paths": a.paths, "rows_in_folder": per,
                               "search_within_ms_median": float(np.median(w_f)), "search_within_ms_min": float(min(w_f)),
                               "filtered_ids_ms_median": float(np.median(w_i)), "filtered_ids_ms_min": float(min(w_i)),
                               "resolution_ms": float(np.median(w_f) - np.median(w_i))}
    ix.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
