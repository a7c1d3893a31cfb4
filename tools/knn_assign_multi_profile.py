"""What mi_knn_assign_multi costs: --rows synthetic rows against C = 1 024 Gaussian vectors.

    python tools/knn_assign_multi_profile.py [--rows 1000000] [--out profiles/assign_multi_profile.json]

Host clock of a call: median of 5 after 1 warm-up, per m in 1, 4, 16 and max_dist in +inf, 0.9, "prefilter" = 1 (the table
keeps the bf16 mirror, so no call builds one), with the candidates per row stage 1 handed over.  Baseline, the only other
route to the same labels: a table of the C vectors searched with groups of 16 table rows through
mi_knn_search_batched_device (k = m), timed over 64 groups in the same process, alternating with the calls, scaled by
N / 16 (the row copies and the threshold pass the route also needs are not charged).  At m = 1, max_dist = +inf
mi_knn_assign is timed beside it the same way.
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

DIM, C = 768, 1024
MS = (1, 4, 16)
MAX_DISTS = (float("inf"), 0.9)


def host_clocks(n, ms):
    import torch
    from image_search_amd.search import EmbeddingTable
    t = EmbeddingTable(DIM, 0)
    t.insert_synthetic(11, 0, n)
    t.set_option("prefilter", 1)
    v = np.random.default_rng(C).standard_normal((C, DIM)).astype(np.float32)
    tv = EmbeddingTable(DIM, 0)
    tv.insert(v)
    q = torch.from_numpy(t.rows(0, 16 * 64)).cuda().reshape(64, 16, DIM)
    res = {"rows": n, "C": C}
    t.assign(v)   # (builds the table's mirror)
    for m in ms:
        idx = torch.zeros((16, m), dtype=torch.int64, device="cuda")
        dist = torch.zeros((16, m), dtype=torch.float32, device="cuda")

        def groups(first, count):
            t0 = time.perf_counter()
            for g in range(first, first + count):
                tv.knn_device(q[g].data_ptr(), 16, m, idx.data_ptr(), dist.data_ptr(), 0, batched=True)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        groups(0, 4)
        for max_dist in MAX_DISTS:
            t.assign_multi(v, m, max_dist)   # warm-up
            runs, base_s = [], 0.0
            for it in range(5):
                t0 = time.perf_counter()
                t.assign_multi(v, m, max_dist)
                runs.append(time.perf_counter() - t0)
                base_s += groups(it * 12, 12 if it < 4 else 16)   # 64 groups in all, alternating with the calls
            st = t.assign_multi_stats()
            med = statistics.median(runs)
            entry = {"host_s_median": med, "host_s": runs, "candidates_per_row": st["candidates"] / n, "hits_per_row": st["hits"] / n,
                     "launches": st["launches"], "baseline_s_per_group_of_16": base_s / 64,
                     "baseline_scaled_s": base_s / 64 * (n / 16), "ratio_baseline_over_assign_multi": base_s / 64 * (n / 16) / med}
            if m == 1 and max_dist == float("inf"):
                one = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    t.assign(v)
                    one.append(time.perf_counter() - t0)
                entry["mi_knn_assign_host_s_median"] = statistics.median(one)
                entry["mi_knn_assign_candidates_per_row"] = t.assign_stats()["candidates"] / n
            res[f"m{m}_max_dist_{max_dist}"] = entry
            print(f"m {m} max_dist {max_dist}: {json.dumps(entry)}", flush=True)
    tv.close()
    t.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=0, help="one m only (default: 1, 4, 16)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_multi_profile.json"))
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault(str(a.rows), {}).update(host_clocks(a.rows, (a.m,) if a.m else MS))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res[str(a.rows)]))
