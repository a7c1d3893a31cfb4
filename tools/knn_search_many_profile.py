"""What mi_knn_search_many / mi_knn_neighbors cost: --rows synthetic rows, dim 768.

    python tools/knn_search_many_profile.py [--rows 1000000] [--out profiles/search_many_profile.json]

Case a: knn_many with nq = 1 024 Gaussian queries, k = 10.  Case b: neighbors of a 65 536-row slice, k = 10.  Every case
runs in a child process of its own under a time limit; a case that fails ends the run.  Per case and per variant of the two
options ("many_sample": the stride of the threshold pass over the column tiles, "many_segments": column segments of a
launch; 0 = what the library chooses) the host clock of a call, median of 5 after 1 warm-up, with the candidates per query
and the stage-1 launches.  Baseline, what a user does without the feature: the same queries through
mi_knn_search_batched_device in groups of 16 on the same table in its best configuration ("prefilter" = 2, so the new
calls build their bf16 mirror inside the timed call), 64 groups timed in the same process alternating with the calls,
scaled to the query count.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, K = 768, 10
NQ_A, N_B = 1024, 65536
# (many_sample, many_segments)
VARIANTS = {"a": ((0, 0), (1, 0), (8, 0), (32, 0), (0, 1), (1, 1)), "b": ((0, 0), (1, 0), (8, 0), (32, 0), (0, 1))}


def run_case(case, n):
    import torch
    from image_search_amd.search import EmbeddingTable
    t = EmbeddingTable(DIM, 0)
    t.insert_synthetic(11, 0, n)
    t.set_option("prefilter", 2)
    nq = NQ_A if case == "a" else min(N_B, n)
    queries = np.random.default_rng(5).standard_normal((NQ_A, DIM)).astype(np.float32) if case == "a" else t.rows(0, 16 * 64)
    q = torch.from_numpy(queries[:16 * 64]).cuda().reshape(64, 16, DIM)
    kb = K if case == "a" else K + 1   # (the graph's route asks for k + 1 and drops the row itself)
    idx = torch.zeros((16, kb), dtype=torch.int64, device="cuda")
    dist = torch.zeros((16, kb), dtype=torch.float32, device="cuda")

    def groups(first, count):
        t0 = time.perf_counter()
        for g in range(first, first + count):
            t.knn_device(q[g].data_ptr(), 16, kb, idx.data_ptr(), dist.data_ptr(), 0, batched=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def call():
        return t.knn_many(queries, K) if case == "a" else t.neighbors(K, 0, nq)

    groups(0, 4)
    res = {"rows": n, "queries": nq, "k": K}
    first = None
    for sample, segments in VARIANTS[case]:
        t.set_option("many_sample", sample)
        t.set_option("many_segments", segments)
        got = call()   # warm-up
        if first is None:
            first = got
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1].view(np.uint32), first[1].view(np.uint32))
        runs, base_s = [], 0.0
        for it in range(5):
            t0 = time.perf_counter()
            call()
            runs.append(time.perf_counter() - t0)
            base_s += groups(it * 12, 12 if it < 4 else 16)   # 64 groups in all, alternating with the calls
        st = t.search_many_stats()
        med = statistics.median(runs)
        entry = {"host_s_median": med, "host_s": runs, "candidates_per_query": st["candidates"] / nq, "hits_per_query": st["hits"] / nq,
                 "launches": st["launches"], "tiles": st["tiles"], "baseline_s_per_group_of_16": base_s / 64,
                 "baseline_scaled_s": base_s / 64 * (nq / 16), "ratio_baseline_over_new": base_s / 64 * (nq / 16) / med}
        res[f"sample{sample}_segments{segments}"] = entry
        print(f"case {case} many_sample {sample} many_segments {segments}: {json.dumps(entry)}", flush=True)
    if case == "a":   # where the batched route would win: smaller query counts at the library's own choices
        t.set_option("many_sample", 0)
        t.set_option("many_segments", 0)
        for small in (16, 64, 256):
            t.knn_many(queries[:small], K)
            runs = []
            for _ in range(5):
                t0 = time.perf_counter()
                t.knn_many(queries[:small], K)
                runs.append(time.perf_counter() - t0)
            base = groups(0, 16) / 16 * (small / 16)
            res[f"nq{small}"] = {"host_s_median": statistics.median(runs), "baseline_scaled_s": base}
            print(f"case a nq {small}: {json.dumps(res[f'nq{small}'])}", flush=True)
    t.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--case", default="", help="a or b: run that case in this process and print its JSON (what the parent starts)")
    ap.add_argument("--limit", type=int, default=280, help="seconds a case may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_many_profile.json"))
    a = ap.parse_args()
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, a.rows)))
        sys.exit(0)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for case in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--case", case], timeout=a.limit,
                           stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.exit(f"case {case} ended with status {p.returncode}: nothing more is started")
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        res.setdefault(str(a.rows), {})[f"case_{case}"] = json.loads(line[len("RESULT "):])
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
