"""What deleted rows cost the searches (DESIGN.md "Deleted rows"): 10 M synthetic rows, tables with 0, 0.1, 1 and 10 % of
their rows deleted, measured alternately in one process with device events around each search (warm iterations, median
and min): the single pass at k = 10 and k = 1000 (radix select), the two-stage search over the byte mirror at k = 10, and a
group of 16 queries through it (adaptive skipping of stage 1 off; mi_knn_prefilter_stats recorded to show stage 1 ran); then
mi_knn_delete of 10^5 ids on a table that already has 1 % deleted.  A delete is synchronous and runs on the table's own stream,
which a caller cannot put events on: its figure is the host clock around the call (host sort and checks, the upload, the
kernel, the wait), an upper bound of its device time.  Writes profiles/delete_profile.json.

    python tools/knn_delete_profile.py [--rows 10000000] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from image_search_amd import synth
    from image_search_amd.search import EmbeddingTable

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delete_profile.json"))
    a = ap.parse_args()
    fracs = [0.0, 0.001, 0.01, 0.1]
    rng = np.random.default_rng(1)
    tables = []
    for f in fracs:
        t = EmbeddingTable(768, 0)
        t.insert_synthetic(3, 0, a.rows)
        if f:
            t.delete(np.sort(rng.choice(a.rows, int(a.rows * f), replace=False)).astype(np.uint64))
        tables.append(t)
    qs = synth.corpus_rows(1003, 0, 16)
    d_q = torch.from_numpy(qs).cuda()
    stream = torch.cuda.Stream()   # a stream of its own: a NULL stream would send the search to the table's own stream

    def timed(t, nq, k, batched):
        d_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        d_d = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        t.knn_device(d_q.data_ptr(), nq, k, d_i.data_ptr(), d_d.data_ptr(), stream.cuda_stream, batched=batched)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    cases = {"single_k10": (0, 1, 10, False), "single_k1000": (0, 1, 1000, False),
             "two_stage_k10": (2, 1, 10, False), "group16_k10": (2, 16, 10, True)}
    res = {c: {str(f): [] for f in fracs} for c in cases}
    stats = {}
    for name, (pref, nq, k, batched) in cases.items():
        for t in tables:
            t.set_option("prefilter", pref)
            t.set_option("prefilter_adaptive", 0)
            for _ in range(3):
                timed(t, nq, k, batched)  # warm-up (the mirror is built by the first search)
        for _ in range(a.iters):
            for f, t in zip(fracs, tables):  # alternate the tables: drifts of the clock hit every fraction alike
                res[name][str(f)].append(timed(t, nq, k, batched))
        if pref:
            stats[name] = {str(f): t.prefilter_stats() for f, t in zip(fracs, tables)}
    out = {"rows": a.rows, "iters": a.iters, "device": torch.cuda.get_device_name(0), "ms": {},
           "prefilter_stats_candidates_fell_back": {n: {f: [int(c), bool(b)] for f, (c, b) in v.items()} for n, v in stats.items()}}
    for name in cases:
        out["ms"][name] = {}
        base = float(np.median(res[name]["0.0"]))
        for f in fracs:
            v = np.array(res[name][str(f)])
            out["ms"][name][str(f)] = {"median": float(np.median(v)), "min": float(v.min()),
                                       "vs_none": float(np.median(v) / base - 1.0)}
    # deletes of 10^5 live ids each on the table with 1 % deleted (not its first delete: nothing is allocated the first time here)
    t = tables[2]
    live = np.setdiff1d(np.arange(a.rows, dtype=np.uint64), t.deleted())
    pick = rng.permutation(live)[:5 * 100_000]
    wall = []
    for j in range(5):
        ids = np.sort(pick[j * 100_000:(j + 1) * 100_000])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert t.delete(ids) == ids.size
        wall.append((time.perf_counter() - t0) * 1e3)
    out["delete_1e5_ms_wall"] = {"median": float(np.median(wall)), "min": float(min(wall)), "all": wall}
    for t in tables:
        t.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
