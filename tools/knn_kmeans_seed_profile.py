"""What mi_knn_kmeans_seed costs and what it buys: --rows synthetic rows, dim 768.

    python tools/knn_kmeans_seed_profile.py [--rows 1000000] [--out profiles/kmeans_seed_profile.json]

Cases (C, sample): (64, 16 384), (1 024, 65 536), (1 024, all rows), (4 096, 262 144); `sample` rows are a seeded uniform
subset, as EmbeddingTable.kmeans(init="kmeans++") draws it.  Every case runs in a child process of its own under a time
limit; a case that fails ends the run.  Per case: the host clock of a seeding (median of 3 after 1 warm-up), the time per
pass against the bytes a pass reads (S x dim x 4; as a fraction of the 8 TB/s HBM peak where those bytes exceed the 256 MB
Infinity Cache), one Lloyd iteration's time beside it, and — with --objective, for the first two cases — the objective
after 20 iterations from init = "uniform" and from init = "kmeans++" for seeds 0 .. 4.
Baseline, at (1 024, 65 536): the host route the call replaces — mi_knn_get_rows of the sample and the numpy form of the
same rule with one float32 matrix-vector product per centre, on 16 threads.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "16")
os.environ.setdefault("MKL_NUM_THREADS", "16")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM = 768
CASES = {"a": (64, 16384), "b": (1024, 65536), "c": (1024, 0), "d": (4096, 262144)}   # sample 0 = all rows
HBM_PEAK, CACHE = 8.0e12, 256 << 20


def splitmix64(seed, n):
    out, state, mask = [], seed, (1 << 64) - 1
    for _ in range(n):
        state = (state + 0x9E3779B97F4A7C15) & mask
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        out.append(z ^ (z >> 31))
    return out


def host_route(t, among, C, seed):
    """the replaced route: fetch the sample's rows (the table in blocks of 65 536 rows, the sample's rows kept: cheaper than
    one mi_knn_get_rows per id), then C dependent passes in numpy (one float32 matrix-vector product per centre)"""
    t0 = time.perf_counter()
    n, parts = len(t), []
    for first in range(0, n, 65536):
        block = t.rows(first, min(65536, n - first))
        parts.append(block if among is None else block[(among[(among >= first) & (among < first + 65536)] - np.uint64(first)).astype(np.int64)])
    x = np.concatenate(parts)
    fetch = time.perf_counter() - t0
    inv = 1.0 / np.sqrt(np.einsum("ij,ij->i", x, x))
    z = splitmix64(seed, C)
    D = np.full(x.shape[0], np.inf, np.float32)
    w = np.ones(x.shape[0], np.uint64)
    picks = []
    for j in range(C):
        prefix = np.cumsum(w)
        p = int(np.searchsorted(prefix, np.uint64((z[j] * int(prefix[-1])) >> 64), side="right"))
        picks.append(p)
        D = np.minimum(D, 1.0 - (x @ x[p]) * inv * inv[p])
        w = np.floor(np.clip(D, 0.0, 2.0) * np.float32(2.0 ** 30)).astype(np.uint64)
        w[picks] = 0
    return fetch, time.perf_counter() - t0


def run_case(case, n, objective):
    from image_search_amd.search import EmbeddingTable
    C, sample = CASES[case]
    t = EmbeddingTable(DIM, 0)
    t.insert_synthetic(11, 0, n)
    S = n if sample == 0 or sample >= n else sample
    among = None if S == n else np.sort(np.random.default_rng(0).choice(np.arange(n, dtype=np.uint64), size=S, replace=False))
    t.kmeans_seed(C, 0, among)   # warm-up
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = t.kmeans_seed(C, 0, among)
        runs.append(time.perf_counter() - t0)
    med = statistics.median(runs)
    bytes_per_pass = S * DIM * 4
    per_pass = med / (C + 1)
    res = {"rows": n, "C": C, "candidates": S, "seed_s_median": med, "seed_s": runs, "s_per_pass": per_pass,
           "bytes_per_pass": bytes_per_pass, "stats": t.kmeans_seed_stats(), "potential": got["potential"],
           "hbm_fraction": bytes_per_pass / per_pass / HBM_PEAK if bytes_per_pass > CACHE else None}
    t0 = time.perf_counter()
    t.kmeans(got["centroids"], max_iters=1)
    res["one_lloyd_iteration_s"] = time.perf_counter() - t0
    if case == "b":
        fetch, total = host_route(t, among, C, 0)
        res["baseline_host_route"] = {"get_rows_s": fetch, "total_s": total, "ratio_baseline_over_new": total / med}
    if objective:
        res["objective_after_20"] = {init: [t.kmeans(C, max_iters=20, seed=s, init=init, sample=sample or None)["objective"] for s in range(5)]
                                     for init in ("uniform", "kmeans++")}
    t.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--case", default="", help="a .. d: run that case in this process and print its JSON (what the parent starts)")
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--objective", default="ab", help="cases that also run the 2 x 5 k-means of 20 iterations")
    ap.add_argument("--limit", type=int, default=280, help="seconds a case may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_seed_profile.json"))
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, a.rows, a.case in a.objective)))
        sys.exit(0)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for case in a.cases:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--case", case, "--objective", a.objective],
                           timeout=a.limit, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.exit(f"case {case} ended with status {p.returncode}: nothing more is started")
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        res.setdefault(str(a.rows), {})[f"case_{case}"] = json.loads(line[len("RESULT "):])
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
