"""What the join of two row sets costs beside the single-table self-join, on one MI355X:

    python tools/join_between_profile.py [--rows 1000000] [--out profiles/join_between_profile.json]

  (c) the self-join (near_pairs) of --rows synthetic rows + 200 planted near-copies: the code path that existed before, and
      the yardstick;
  (a) the first half of those rows as table A against the second half (+ the planted rows) as table B (near_pairs_with),
      the column side read where it lies and through the staged copy ("join_stage" = 1);
  (b) the same rows as a sharded table of 1, 2, 4 and 8 shards on device 0 (ShardedTable.near_pairs).

All in one process, calls alternating, median of 3 after one warm-up each, on the host clock around the synchronous calls.
From tile counts alone (a) computes N^2 tiles against the self-join's (2 N)^2 / 2, half of (c), and (b) computes (c)'s tiles
(the identity of 5.29); the ratios and the staged copy's share are what 5.29 quotes beside these expectations.
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

DIM, PLANTED, MAX_DIST, SEED = 768, 200, 0.05, 11
OUT = os.path.join(ROOT, "profiles", "join_between_profile.json")


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def median3(f):
    clock(f)
    times, out = [], None
    for _ in range(3):
        s, out = clock(f)
        times.append(s)
    return statistics.median(times), times, out


def planted_rows(table, n):
    """near-copies of PLANTED rows of the first half, rescaled (sigma up to 0.4 of an element's size: some within MAX_DIST)"""
    rng = np.random.default_rng(SEED)
    src = np.sort(rng.choice(n // 2, PLANTED, replace=False))
    base = np.stack([table.rows(int(r), 1)[0] for r in src])
    sigma = np.linspace(0.0, 0.4, PLANTED)
    return ((base + sigma[:, None] * np.abs(base).mean() * rng.standard_normal((PLANTED, DIM)))
            * rng.uniform(0.1, 10.0, (PLANTED, 1))).astype(np.float32)


def run(n):
    from image_search_amd.search import EmbeddingTable, ShardedTable
    half = n // 2
    res = {"rows": n + PLANTED, "max_dist": MAX_DIST}

    one = EmbeddingTable(DIM, 0)
    one.insert_synthetic(SEED, 0, n)
    planted = planted_rows(one, n)
    one.insert(planted)
    s, times, pairs = median3(lambda: one.near_pairs(MAX_DIST))
    res["self_join"] = {"host_s_median": s, "host_s": times, "pairs": int(pairs[0].size), "stats": one.near_pairs_stats()}
    cross = (pairs[0] < half) & (pairs[1] >= n)           # what (a) must find: a in the first half, b a planted row
    want = (pairs[0][cross], pairs[1][cross], pairs[2][cross])

    ta, tb = EmbeddingTable(DIM, 0), EmbeddingTable(DIM, 0)
    ta.insert_synthetic(SEED, 0, half)
    tb.set_base(half)
    tb.insert_synthetic(SEED, half, n - half)
    tb.insert(planted)
    for name, stage in (("between_direct", 0), ("between_staged", 1)):
        ta.set_option("join_stage", stage)
        s, times, got = median3(lambda: ta.near_pairs_with(tb, MAX_DIST))
        found = got[1] >= n
        same = (np.array_equal(got[0][found], want[0]) and np.array_equal(got[1][found], want[1])
                and np.array_equal(got[2][found].view(np.uint32), want[2].view(np.uint32)))
        res[name] = {"host_s_median": s, "host_s": times, "pairs": int(got[0].size), "planted_pairs_equal_the_self_joins": bool(same),
                     "stats": ta.near_pairs_with_stats(), "ratio_over_self_join": s / res["self_join"]["host_s_median"]}
    res["staging_share_of_staged"] = 1.0 - res["between_direct"]["host_s_median"] / res["between_staged"]["host_s_median"]
    ta.close(); tb.close()

    res["sharded"] = {}
    for shards in (1, 2, 4, 8):
        t = ShardedTable(DIM, [0] * shards, 0)
        t.insert_synthetic(SEED, 0, n)
        t.insert(planted)
        s, times, got = median3(lambda: t.near_pairs(MAX_DIST))
        same = (np.array_equal(got[0], pairs[0]) and np.array_equal(got[1], pairs[1])
                and np.array_equal(got[2].view(np.uint32), pairs[2].view(np.uint32)))
        res["sharded"][str(shards)] = {"host_s_median": s, "host_s": times, "pairs": int(got[0].size), "equals_the_self_join": bool(same),
                                       "block_rows": t.info()["block_rows"], "stats": t.near_pairs_stats(),
                                       "ratio_over_self_join": s / res["self_join"]["host_s_median"]}
        t.close()
    one.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res[str(a.rows)] = run(a.rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res[str(a.rows)]))
