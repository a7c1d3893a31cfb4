"""What mi_knn_search_diverse costs on top of a search, against the route it replaces: --rows synthetic
rows of dim 768, (pool, k) in (256, 64), (1 000, 250), (4 096, 1 000).

    python tools/knn_diverse_profile.py [--rows 1000000] [--calls 20] [--out profiles/diverse_profile.json]

Per case, in ONE process, the three routes interleaved call by call after 3 warm-up rounds, medians of --calls calls:
  (a) mi_knn_search with k = pool alone;
  (b) mi_knn_search_diverse(k, pool, min_gap);
  (c) what a user had before: (a), mi_knn_get_rows of the pool's rows, a numpy float32 pair matrix and the walk in python,
      on 16 threads.
min_gap is found per case by bisection over route (c)'s own pair matrix so that the walk hides 5 .. 20 % of the pool
(synthetic rows are unrelated: their pair distances lie in a narrow band below 1, so the gap is large; what is timed does
not depend on its value).  Reported: the medians, (b) - (a) against (c) - (a), and (b) / (a).
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "16")
os.environ.setdefault("MKL_NUM_THREADS", "16")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM = 768
CASES = [(256, 64), (1000, 250), (4096, 1000)]


def walk(G, k, gap):
    """the greedy walk over a pair matrix in rank coordinates -> (kept ranks, entries hidden)"""
    kept, hidden = [], 0
    for r in range(G.shape[0]):
        if kept and np.any(G[r, kept] <= gap):
            hidden += 1
        elif len(kept) < k:
            kept.append(r)
    return kept, hidden


def pair_matrix(t, idx):
    rows = np.stack([t.rows(int(i), 1)[0] for i in idx])          # mi_knn_get_rows, one call per pool entry
    unit = rows / np.sqrt(np.einsum("ij,ij->i", rows, rows))[:, None]
    return (np.float32(1.0) - unit @ unit.T).astype(np.float32)


def host_route(t, q, pool, k, gap):
    idx, dist = t.knn(q, pool)
    idx = idx[idx != np.uint64(0xFFFFFFFFFFFFFFFF)]
    return walk(pair_matrix(t, idx), k, gap)


def find_gap(t, q, pool, k):
    idx, _ = t.knn(q, pool)
    G = pair_matrix(t, idx)
    lo, hi = float(G[np.triu_indices(pool, 1)].min()), float(np.median(G))
    for _ in range(20):
        gap = 0.5 * (lo + hi)
        frac = walk(G, k, np.float32(gap))[1] / pool
        if 0.05 <= frac <= 0.20:
            return gap, frac
        lo, hi = (gap, hi) if frac < 0.05 else (lo, gap)
    raise SystemExit(f"no min_gap hides 5 .. 20 % of a pool of {pool}")


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diverse_profile.json"))
    a = ap.parse_args()
    from image_search_amd.search import EmbeddingTable
    t = EmbeddingTable(DIM, 0)
    t.insert_synthetic(21, 0, a.rows)
    q = (t.rows(a.rows // 2, 1)[0] + 0.5 * np.random.default_rng(0).standard_normal(DIM)).astype(np.float32)
    res = {"rows": a.rows, "dim": DIM, "calls": a.calls, "cases": []}
    for pool, k in CASES:
        gap, frac = find_gap(t, q, pool, k)
        routes = {"a": lambda: t.knn(q, pool), "b": lambda: t.knn_diverse(q, k, gap, pool=pool),
                  "c": lambda: host_route(t, q, pool, k, np.float32(gap))}
        times = {name: [] for name in routes}
        for it in range(3 + a.calls):
            for name, f in routes.items():
                s = timed(f)
                if it >= 3:
                    times[name].append(s)
        med = {name: statistics.median(v) for name, v in times.items()}
        case = {"pool": pool, "k": k, "min_gap": gap, "hidden_fraction_host_walk": frac, "stats": t.knn_diverse_stats(),
                "median_s": med, "min_s": {n: min(v) for n, v in times.items()}, "max_s": {n: max(v) for n, v in times.items()},
                "b_minus_a_s": med["b"] - med["a"], "c_minus_a_s": med["c"] - med["a"],
                "b_minus_a_over_c_minus_a": (med["b"] - med["a"]) / (med["c"] - med["a"]), "b_over_a": med["b"] / med["a"]}
        print(json.dumps(case))
        res["cases"].append(case)
    t.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
