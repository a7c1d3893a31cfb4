"""What mi_knn_summarize costs: --rows rows of 20 planted themes, dim 768.

    python tools/knn_summary_profile.py [--rows 1000000] [--out profiles/summary_profile.json]

Two steps, each in a child process of its own under a time limit; a step that fails ends the run.
  measure   the table is built once.  (a) the host clock of summarize (median of 5 after 1 warm-up) for three labelings:
            "themes" = the 20 planted themes, "kmeans" = the labels of kmeans(1 000, 2 iterations), "singletons" = 65 536
            random labels (15 members each: the unfavourable case).  (b) one single-pass fp32 knn(q, 10) over the same table
            (median of 5).  The call reads the member rows twice (the sum, then the distances), so (a) / (b) is the figure
            to read; 2 is what two passes at the search's speed would give.
  baseline  (c) the route without the call, once, on the "themes" labeling: rows(0, n) in blocks of 65 536 and numpy —
            unit rows, per-group sums, distances to the centroids, cover and odd one out by sorting.
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

DIM, THEMES, BLOCK = 768, 20, 65536


def build_table(n):
    """n rows = theme[r % 20] + 0.5 x noise under row scales 0.1 .. 10, generated and inserted block by block"""
    from image_search_amd.search import EmbeddingTable
    rng = np.random.default_rng(7)
    themes = rng.standard_normal((THEMES, DIM)).astype(np.float32)
    t = EmbeddingTable(DIM, 0)
    t.reserve(n)
    for first in range(0, n, BLOCK):
        m = min(BLOCK, n - first)
        own = (np.arange(first, first + m) % THEMES)
        x = themes[own] + np.float32(0.5) * rng.standard_normal((m, DIM), dtype=np.float32)
        x *= rng.uniform(0.1, 10.0, (m, 1)).astype(np.float32)
        t.insert(x)
    return t, themes, (np.arange(n) % THEMES).astype(np.uint32)


def timed(f, runs=5):
    f()   # warm-up
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        out.append(time.perf_counter() - t0)
    return out


def measure(n, only=""):
    """only: one labeling's name — that labeling alone (what a run under a profiler wants: its kernels are then the call's)"""
    t, themes, own = build_table(n)
    res = {"rows": n, "dim": DIM}
    q = themes[3] + np.float32(0.5) * np.random.default_rng(8).standard_normal(DIM).astype(np.float32)
    runs = timed(lambda: t.knn(q, 10))
    res["search_single_pass_s"] = {"median": statistics.median(runs), "runs": runs}
    labelings = {"themes": (own, THEMES), "kmeans": (None, 1000),
                 "singletons": (np.random.default_rng(9).integers(0, 65536, n).astype(np.uint32), 65536)}
    for name, (labels, C) in labelings.items():
        if only and name != only:
            continue
        if labels is None:
            t0 = time.perf_counter()
            labels = t.kmeans(C, max_iters=2, seed=0)["labels"]
            res["kmeans_1000_two_iterations_s"] = time.perf_counter() - t0
        runs = timed(lambda: t.summarize(labels, C))
        s = t.summarize(labels, C)
        med = statistics.median(runs)
        res[name] = {"C": C, "summarize_s": {"median": med, "runs": runs}, "ratio_to_one_search_pass": med / res["search_single_pass_s"]["median"],
                     "member_bytes_read_twice": 2 * s["totals"]["members"] * DIM * 4, "totals": s["totals"], "stats": t.summarize_stats(),
                     "largest_group": int(s["count"].max()), "mean_dist_median": float(np.nanmedian(s["mean_dist"]))}
        print(name, res[name], flush=True)
    t.close()
    return res


def baseline(n):
    """(c): every row over the bus, then numpy"""
    t, themes, own = build_table(n)
    t0 = time.perf_counter()
    x = np.concatenate([t.rows(first, min(BLOCK, n - first)) for first in range(0, n, BLOCK)])
    fetch = time.perf_counter() - t0
    unit = x / np.sqrt(np.einsum("ij,ij->i", x, x))[:, None]
    order = np.argsort(own, kind="stable")
    cuts = np.searchsorted(own[order], np.arange(THEMES + 1))
    cent = np.stack([unit[order[cuts[c]:cuts[c + 1]]].sum(axis=0) / max(cuts[c + 1] - cuts[c], 1) for c in range(THEMES)])
    cn = cent / np.linalg.norm(cent, axis=1, keepdims=True)
    dist = 1.0 - np.einsum("ij,ij->i", unit, cn[own])
    by = np.lexsort((dist, own))
    cover, odd = by[cuts[:-1]], by[cuts[1:] - 1]
    total = time.perf_counter() - t0
    t.close()
    return {"rows": n, "get_rows_s": fetch, "total_s": total, "cover_0": int(cover[0]), "odd_0": int(odd[0])}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--step", default="", help="measure | baseline: run that step in this process and print its JSON (what the parent starts)")
    ap.add_argument("--only", default="", help="with --step measure: themes | kmeans | singletons alone")
    ap.add_argument("--steps", default="measure,baseline")
    ap.add_argument("--limit", type=int, default=280, help="seconds a step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_profile.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(measure(a.rows, a.only) if a.step == "measure" else baseline(a.rows)))
        sys.exit(0)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for step in a.steps.split(","):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--step", step], timeout=a.limit,
                           stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.exit(f"step {step} ended with status {p.returncode}: nothing more is started")
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        res.setdefault(str(a.rows), {})[step] = json.loads(line[len("RESULT "):])
        if step == "baseline" and "measure" in res[str(a.rows)]:
            res[str(a.rows)]["baseline"]["ratio_baseline_over_call"] = (res[str(a.rows)]["baseline"]["total_s"]
                                                                        / res[str(a.rows)]["measure"]["themes"]["summarize_s"]["median"])
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
