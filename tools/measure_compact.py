"""What a compaction costs and what it gives back: 10 M synthetic rows at dim 768 with 0.1, 1 and 10 % of
the rows deleted at random.

1. mi_knn_compact by the host clock around the synchronous call, median of `--reps` FRESH tables per fraction (a compaction
   cannot be repeated), against a device-to-device hipMemcpy of the moved bytes between two buffers of that size (the cost
   of touching those bytes once: the yardstick), with the straight / staged chunk counts.
2. The four searches of the deleted-rows cost table (tools/knn_delete_profile.py: single pass k = 10 and k = 1000, two-stage
   k = 10, a group of 16 through the two stages) with device events, on the first table of each fraction immediately before
   and after its compaction, alternating with a table that never had a deletion, in this process.

Writes profiles/compact_profile.json.

    python tools/measure_compact.py [--rows 10000000] [--reps 5] [--iters 10] [--fractions 0.001,0.01,0.1]
                                    [--chunk-rows S] [--no-searches]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"single_k10": (0, 1, 10, False), "single_k1000": (0, 1, 1000, False),
         "two_stage_k10": (2, 1, 10, False), "group16_k10": (2, 16, 10, True)}


def main():
    import torch

    from image_search_amd import synth
    from image_search_amd.search import EmbeddingTable

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--fractions", default="0.001,0.01,0.1")
    ap.add_argument("--chunk-rows", type=int, default=0, help='option "compact_chunk_rows" (0 = the default)')
    ap.add_argument("--no-searches", action="store_true", help="the compaction times alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_profile.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    d_q = torch.from_numpy(synth.corpus_rows(1003, 0, 16)).cuda()
    stream = torch.cuda.Stream()   # a stream of its own: a NULL stream would send the search to the table's own stream

    def table(frac):
        t = EmbeddingTable(768, 0)
        t.insert_synthetic(3, 0, a.rows)
        t.set_option("prefilter_adaptive", 0)
        t.set_option("compact_chunk_rows", a.chunk_rows)
        if frac:
            t.delete(np.sort(rng.choice(a.rows, int(a.rows * frac), replace=False)).astype(np.uint64))
        return t

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

    def searches(t, none):
        """median ms of the four searches on t and on the table without deletions, alternating"""
        out = {}
        for name, (pref, nq, k, batched) in CASES.items():
            ms = {"t": [], "none": []}
            for x in (t, none):
                x.set_option("prefilter", pref)
                for _ in range(3):
                    timed(x, nq, k, batched)   # warm-up (the first search builds or catches up the mirror)
            for _ in range(a.iters):
                ms["t"].append(timed(t, nq, k, batched))
                ms["none"].append(timed(none, nq, k, batched))
            out[name] = {"ms": float(np.median(ms["t"])), "none_ms": float(np.median(ms["none"])),
                         "vs_none": float(np.median(ms["t"]) / np.median(ms["none"]) - 1.0)}
        return out

    none = table(0.0)
    out = {"rows": a.rows, "reps": a.reps, "iters": a.iters, "compact_chunk_rows": a.chunk_rows, "device": torch.cuda.get_device_name(0), "fractions": {}}
    for frac in [float(f) for f in a.fractions.split(",")]:
        wall, stats, before, after = [], None, None, None
        for rep in range(a.reps):
            t = table(frac)
            if rep == 0 and not a.no_searches:
                before = searches(t, none)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = t.compact()
            wall.append((time.perf_counter() - t0) * 1e3)
            stats = t.compact_stats()
            assert res["removed"] == int(a.rows * frac) and len(t) == a.rows - res["removed"]
            if rep == 0 and not a.no_searches:
                after = searches(t, none)
            t.close()
        moved_bytes = int(stats["moved"]) * 768 * 4
        src = torch.empty(moved_bytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(moved_bytes, dtype=torch.uint8, device="cuda")
        copy = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src)
            torch.cuda.synchronize()
            copy.append((time.perf_counter() - t0) * 1e3)
        del src, dst
        torch.cuda.empty_cache()
        copy_ms = float(np.median(copy[1:]))
        out["fractions"][str(frac)] = {
            "compact_ms": {"median": float(np.median(wall)), "min": float(min(wall)), "all": wall},
            "memcpy_moved_bytes_ms": copy_ms, "ratio_to_memcpy": float(np.median(wall) / copy_ms), "moved_bytes": moved_bytes,
            "stats": stats, "searches_before": before, "searches_after": after}
    none.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
