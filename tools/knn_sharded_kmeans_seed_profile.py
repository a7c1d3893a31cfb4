"""What k-means++ seeding costs across shards beside the single table and beside the route a sharded table had before
(DESIGN.md 5.37): --rows synthetic rows of dim 768, a seeded sample of --sample of them as `among`, C = 64 and C = 1024.

    python tools/knn_sharded_kmeans_seed_profile.py [--rows 1000000] [--out profiles/sharded_kmeans_seed_profile.json]
    rocprofv3 --kernel-trace --stats -d DIR -o seed -- python tools/knn_sharded_kmeans_seed_profile.py --kernels
                                                                     # device time per kernel, in a run of its own

(s) ShardedTable.kmeans_seed as 2 / 4 / 8 shards on ONE device, against (a) EmbeddingTable.kmeans_seed on one table of the same
rows and (b) the only route a sharded table had: read the sample's rows back one by one (rows()), build an EmbeddingTable of
them and seed there.  The variants alternate in one process; the median of --repeats host clocks after one warm-up each is
kept beside the fastest.  Every sharded result is compared with (a) for equality; (b) seeds the same candidates under other
ids, so its picks are compared through the sample.  Shards on one device share it: (s) / (a) is what the decomposition and
the exchange cost, not what several GPUs gain.
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

DIM = 768
SHARDS = (2, 4, 8)
SEEDS = (64, 1024)
OUT = os.path.join(ROOT, "profiles", "sharded_kmeans_seed_profile.json")


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def same(x, y):
    return (np.array_equal(x["rows"], y["rows"]) and np.array_equal(x["centroids"].view(np.uint32), y["centroids"].view(np.uint32))
            and x["potential"] == y["potential"])


def old_route(t, among, C):
    """(b): the sample read back row by row, a table of it on one device, the seeding there; rows as ids of t"""
    from image_search_amd.search import EmbeddingTable
    sample = np.concatenate([t.rows(int(r), 1) for r in among])
    one = EmbeddingTable(DIM, 0)
    one.insert(sample)
    got = one.kmeans_seed(C, 0)
    one.close()
    got["rows"] = among[got["rows"].astype(np.int64)]
    return got


def kernels(n, sample):
    """one sharded call of each C on 4 shards behind a warm-up, for a kernel trace"""
    from image_search_amd.search import ShardedTable
    among = np.sort(np.random.default_rng(0).choice(np.arange(n, dtype=np.uint64), size=sample, replace=False))
    t = ShardedTable(DIM, [0] * 4)
    t.insert_synthetic(11, 0, n)
    for C in SEEDS:
        for _ in range(2):
            print(C, t.kmeans_seed(C, 0, among)["potential"], t.kmeans_seed_stats(), flush=True)
    t.close()


def host_clocks(n, sample, repeats):
    from image_search_amd.search import EmbeddingTable, ShardedTable
    among = np.sort(np.random.default_rng(0).choice(np.arange(n, dtype=np.uint64), size=sample, replace=False))
    one = EmbeddingTable(DIM, 0)
    one.insert_synthetic(11, 0, n)
    res = {"rows": n, "sample": sample, "repeats": repeats, "C": {}}
    want = {C: one.kmeans_seed(C, 0, among) for C in SEEDS}      # (the warm-up of (a))
    tables = {}
    for shards in SHARDS:
        tables[shards] = ShardedTable(DIM, [0] * shards)
        tables[shards].insert_synthetic(11, 0, n)
    for C in SEEDS:
        clocks = {"single": []}
        equal = {}
        for shards, t in tables.items():                         # the warm-ups
            equal[shards] = same(t.kmeans_seed(C, 0, among), want[C])
            clocks[f"sharded_{shards}"], clocks[f"old_route_{shards}"] = [], []
        old_equal = same(old_route(tables[SHARDS[0]], among, C), want[C])
        for _ in range(repeats):
            clocks["single"].append(clock(lambda: one.kmeans_seed(C, 0, among))[0])
            for shards, t in tables.items():
                s, got = clock(lambda: t.kmeans_seed(C, 0, among))
                clocks[f"sharded_{shards}"].append(s)
                equal[shards] = equal[shards] and same(got, want[C])
                clocks[f"old_route_{shards}"].append(clock(lambda: old_route(t, among, C))[0])
        single = statistics.median(clocks["single"])
        out = {"single_ms": single * 1e3, "single_fastest_ms": min(clocks["single"]) * 1e3, "single_ms_per_seed": single * 1e3 / C,
               "potential": want[C]["potential"], "old_route_equal_to_single": bool(old_equal), "host_s": clocks, "shards": {}}
        for shards, t in tables.items():
            t.kmeans_seed(C, 0, among)
            s, o = statistics.median(clocks[f"sharded_{shards}"]), statistics.median(clocks[f"old_route_{shards}"])
            out["shards"][str(shards)] = {"block_rows": t.info()["block_rows"], "equal_to_single": bool(equal[shards]),
                                          "sharded_ms": s * 1e3, "sharded_fastest_ms": min(clocks[f"sharded_{shards}"]) * 1e3,
                                          "sharded_ms_per_seed": s * 1e3 / C, "old_route_ms": o * 1e3,
                                          "ratio_sharded_over_single": s / single, "ratio_sharded_over_old_route": s / o,
                                          "stats": t.kmeans_seed_stats()}
        res["C"][str(C)] = out
        print(C, json.dumps({k: v for k, v in out.items() if k != "host_s"}), flush=True)
    for t in tables.values():
        t.close()
    one.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--sample", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--kernels", action="store_true", help="only sharded calls on 4 shards, for a kernel trace")
    a = ap.parse_args()
    if a.kernels:
        kernels(a.rows, a.sample)
        sys.exit(0)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res[str(a.rows)] = host_clocks(a.rows, a.sample, a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    if not all(v["equal_to_single"] for c in res[str(a.rows)]["C"].values() for v in c["shards"].values()):
        sys.exit("a sharded result differs from the single table's")
