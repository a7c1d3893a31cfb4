"""What mi_knn_representatives costs: --rows rows of 20 planted themes, dim 768, m = 9.

    python tools/measure_representatives.py [--rows 1000000] [--out profiles/representatives_profile.json]

One step in a child process of its own under a time limit.  The table is built once (tools/knn_summary_profile.py's).  For
two labelings — "themes" = the 20 planted themes, "kmeans" = the labels of kmeans(1 000, 2 iterations) — three things are
timed on the host clock, ALTERNATING inside one loop (7 rounds after 1 warm-up, medians): a single-pass fp32 knn(q, 10) over
the same table, representatives(m = 1) and representatives(m = 9), both started at the first member.  The search is also
timed once more at once, and five times back to back in front of the loop: a search that comes right behind a call which
freed its device buffers has been seen to take many times a search that comes behind a search, so both are recorded.  A round
reads the member rows once, as that search reads every row once, so the search is the yardstick:
    per_round_s = (call(m = 9) - call(m = 1)) / 8,   ratio_round_to_search[_back_to_back] = per_round_s / search
The whole call (with start = "cover", one summarize in front) is timed the same way.  Not measured here: device time per
kernel, and other dims.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

from knn_summary_profile import DIM, THEMES, build_table

M = 9


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def measure(n):
    t, themes, own = build_table(n)
    res = {"rows": n, "dim": DIM, "m": M}
    q = themes[3] + np.float32(0.5) * np.random.default_rng(8).standard_normal(DIM).astype(np.float32)
    for name, C in (("themes", THEMES), ("kmeans", 1000)):
        labels = own if name == "themes" else t.kmeans(C, max_iters=2, seed=0)["labels"]
        runs = {"search": [], "search_again": [], "m1": [], "m9": [], "cover_m9": []}
        last = None
        before = [clock(lambda: t.knn(q, 10))[0] for _ in range(6)][1:]      # back to back, nothing in between
        for i in range(8):          # the first round is the warm-up
            a, _ = clock(lambda: t.knn(q, 10))
            a2, _ = clock(lambda: t.knn(q, 10))                              # ... and once more at once: what the first one paid for coming behind a call
            b, _ = clock(lambda: t.representatives(labels, C, 1, start="first"))
            c, last = clock(lambda: t.representatives(labels, C, M, start="first"))
            stats = t.representatives_stats()
            d, _ = clock(lambda: t.representatives(labels, C, M))
            if i:
                for k, v in zip(("search", "search_again", "m1", "m9", "cover_m9"), (a, a2, b, c, d)):
                    runs[k].append(v)
        med = {k: statistics.median(v) for k, v in runs.items()}
        per_round = (med["m9"] - med["m1"]) / (M - 1)
        res[name] = {"C": C, "search_single_pass_s": med["search"], "search_repeated_at_once_s": med["search_again"],
                     "search_back_to_back_s": statistics.median(before),
                     "ratio_round_to_search_back_to_back": per_round / statistics.median(before), "call_m1_s": med["m1"], "call_m9_s": med["m9"],
                     "call_m9_from_cover_s": med["cover_m9"], "per_round_s": per_round,
                     "ratio_round_to_search": per_round / med["search"], "rounds_launched": stats["rounds"], "stats": stats,
                     "totals": last["totals"], "member_bytes_per_round": last["totals"]["members"] * DIM * 4,
                     "reach_median": float(np.median(last["reach"][np.isfinite(last["reach"])])),
                     "gap_last_median": float(np.median(last["gap"][:, M - 1][np.isfinite(last["gap"][:, M - 1])])), "runs": runs}
        print(name, {k: v for k, v in res[name].items() if k != "runs"}, flush=True)
    t.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--step", default="", help="measure: run in this process and print the JSON (what the parent starts)")
    ap.add_argument("--limit", type=int, default=400, help="seconds the step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "representatives_profile.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(measure(a.rows)))
        sys.exit(0)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--step", "measure"], timeout=a.limit,
                       stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        sys.exit(f"the measurement ended with status {p.returncode}")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res[str(a.rows)] = json.loads(line[len("RESULT "):])
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
