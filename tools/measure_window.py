"""What the stamp window does to the pair calls: --rows synthetic rows with the 20 planted themes of
tools/knn_density_profile.py (500 members each, max_dist 0.1, min_pts 5), but every theme spread over the whole table — its
members are appended in 100 instalments between the synthetic rows — and stamps that ascend in append order over ten years.

    python tools/measure_window.py [--rows 1000000] [--out profiles/window_profile.json]

near_pairs_window and dbscan_window at windows of one hour, one day and 2^64 - 1 against near_pairs and dbscan themselves at
the same distance on the same table (the yardsticks): all eight calls alternate in one loop, medians of 7 after one warm-up
round, on the host clock.  Recorded per call: the times, mi_knn_window_stats' words and the ratio to its yardstick.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, CLUSTERS, PER, PARTS, MAX_DIST, MIN_PTS = 768, 20, 500, 100, 0.1, 5
TEN_YEARS = 10 * 365 * 86_400
WINDOWS = {"hour": 3_600, "day": 86_400, "u64_max": 2 ** 64 - 1}
ROUNDS = 7


def make_table(n):
    from image_search_amd.search import EmbeddingTable
    t = EmbeddingTable(DIM, 0)
    rng = np.random.default_rng(11)
    seg = n // PARTS
    centres = sigma = None
    for p in range(PARTS):
        t.insert_synthetic(11, p * seg, seg if p < PARTS - 1 else n - seg * (PARTS - 1))
        if centres is None:
            centres = np.stack([t.rows(int(r), 1)[0] for r in np.sort(rng.choice(seg, CLUSTERS, replace=False))])
            sigma = 0.25 * np.sqrt(np.mean(centres * centres, axis=1))            # member to member about 0.06
        k = PER // PARTS
        members = centres[:, None, :] + sigma[:, None, None] * rng.standard_normal((CLUSTERS, k, DIM))
        members *= rng.uniform(0.1, 10.0, (CLUSTERS, k, 1))
        t.insert(members.reshape(-1, DIM).astype(np.float32))
    total = len(t)
    stamps = 1_400_000_000 + (np.arange(total, dtype=np.int64) * TEN_YEARS) // total
    t.set_attrs(np.arange(total, dtype=np.uint64), stamps=stamps)
    return t


def measure(n):
    t = make_table(n)
    cap = 1 << 22
    calls = {"near_pairs": lambda: t.near_pairs(MAX_DIST, cap=cap), "dbscan": lambda: t.dbscan(MAX_DIST, MIN_PTS)}
    for name, w in WINDOWS.items():
        calls["near_pairs_window_" + name] = lambda w=w: t.near_pairs_window(MAX_DIST, w, cap=cap)
        calls["dbscan_window_" + name] = lambda w=w: t.dbscan_window(MAX_DIST, w, MIN_PTS)
    times = {k: [] for k in calls}
    stats, result = {}, {}
    for rnd in range(ROUNDS + 1):
        for name, f in calls.items():
            t0 = time.perf_counter()
            out = f()
            dt = time.perf_counter() - t0
            if rnd == 0:
                result[name] = int(out[0].size) if isinstance(out, tuple) else out["summary"]
                stats[name] = (t.window_stats() if "window" in name else
                               t.near_pairs_stats() if name == "near_pairs" else t.dbscan_stats())
            else:
                times[name].append(dt)
    rows = len(t)
    t.close()
    res = {"rows": rows, "max_dist": MAX_DIST, "min_pts": MIN_PTS, "themes": CLUSTERS, "members": PER, "instalments": PARTS,
           "span_s": TEN_YEARS, "rounds": ROUNDS, "calls": {}}
    for name in calls:
        yard = "near_pairs" if name.startswith("near_pairs") else "dbscan"
        med = statistics.median(times[name])
        res["calls"][name] = {"host_s_median": med, "host_s": times[name], "ratio_to_" + yard: med / statistics.median(times[yard]),
                              "result": result[name], "stats": stats[name]}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_profile.json"))
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res[str(a.rows)] = measure(a.rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res[str(a.rows)]))
