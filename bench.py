"""bench.py — the reference's headline workload on MI355X.

BASELINE.json metric: "images/sec embedded (ViT-L/14 b=256) + queries/sec cosine
top-10 over 10M x 768".  One step = one pass of the hot path over one batch
(BASELINE config[3], "fused on HIP streams"): upload a pinned-host batch of 256
synthetic 224x224x3 images, embed it with the bf16 ViT-L/14, append the 256 rows to
the table on the device, answer one top-10 cosine query over this GPU's 10M x 768
fp32 shard plus the appended rows (the reference serves one query per request,
server/src/search.rs:20-102) and read the k results back.  The H2D of the batch and
the D2H of the results are INSIDE the timed region; the upload runs
under the previous batch's tower, the scan is queued asynchronously but on the device it
runs between two towers (step = tower + scan; measured) (mi_pipeline_*).
The query runs as the two-stage EXACT search (a byte mirror of the rows prefilters, the fp32
rows decide: ids and distance bits of the single pass; --prefilter 1 = the bf16
mirror, --no-prefilter = one pass over the fp32 rows, which is also what `roofline_knn` times);
with --full the run checks that both modes return the same ids and distance bits (`two_stage_equal`).

N > 1 (BASELINE config 5, one process per GPU): every rank embeds its own batch (replicas, no
collective) and owns its own 10M-row shard of an N x 10M table; each query's per-shard top-k
(12 k bytes) stays on the device, is all-gathered over RCCL in one collective and merged
identically on every rank (image_search_amd.search.ShardExchange) — weak scaling.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

`python bench.py --gpus N` without a launcher starts its own N ranks (a child
`python -m torch.distributed.run`, before anything here touches the GPU) and relays rank 0's line.
When the box has fewer GPUs than ranks (a rehearsal) the ranks share GPU 0 and exchange over gloo.

Rank 0 prints ONE JSON line.  `value` is whole-job images/s over the timed region
(ViT + query), `ms_per_step` the time of one timed step; "vit" is the forward's time inside
the timed region (HIP events on the ingest stream).  A plain run does only that: set-up,
warm-up, the timed steps.  --full adds everything else, each behind the timed steps: the same
steps with the single-pass query, the kNN kernel alone and the two-stage check ("knn"),
the rooflines, other BASELINE configs, the one-process sharded probe, the CPU baseline and,
with N > 1, the check that every rank merged the same lists.

--dump-outputs DIR writes what the last timed step computed (rank 0): the k ids (float64)
and distances of its query and the embeddings of its batch, as DIR/<name>.npy.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

VIT_FLOP_PER_IMAGE = 2 * 81_012_768_768  # SURVEY.md §2.1 / BASELINE.md §2: algorithmic MACs x 2
# Executed by this implementation: behind the last layer's attention only the CLS row is live, so that
# layer's out_proj / MLP / attention rows for the other 256 tokens are not computed (bit-identical output,
# tests/test_vit_gpu.py::test_cls_only_last_layer_is_bit_identical_to_the_full_one):
#   2*256*(2*1024*1024 + 2*1024*4096) + 4*257*64*16*256 FLOP per image less (q_proj and out_proj, the MLP,
#   the attention rows of the 256 non-CLS tokens).
VIT_FLOP_SKIPPED_PER_IMAGE = 2 * 256 * (2 * 1024 * 1024 + 2 * 1024 * 4096) + 4 * 257 * 64 * 16 * 256
PEAK_BF16_TFLOPS = 2500.0                # dense bf16 MFMA, MI355X_MICROARCH.md chip table
PEAK_HBM_GBS = 8000.0                    # HBM3E spec, same table
PEAK_F32_TFLOPS = 157.3                  # exact-f32 MFMA, same table
METRIC = "images/sec embedded (ViT-L/14 b=256) + queries/sec cosine top-10 over 10M x 768"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rows", type=int, default=10_000_000, help="table rows per GPU")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--full", action="store_true", help="behind the timed steps, also measure and check everything beyond the "
                    "headline figure (single-pass query, kNN kernel alone, rooflines, other configs, sharded probe, CPU baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra-configs", action="store_true", help="with --full: skip the BASELINE config 1 / 2 sub-lines")
    ap.add_argument("--front-overlap", type=int, default=None, choices=(0, 1), help="A/B: option front_overlap of the model (the next forward's "
                    "patch gather + patch GEMM on the copy stream, under the current forward)")
    ap.add_argument("--serial", action="store_true", help="A/B: synchronise after every step (no cross-step overlap)")
    ap.add_argument("--no-prefilter", action="store_true", help="A/B: the query as ONE pass over the fp32 rows (no mirror)")
    ap.add_argument("--prefilter", type=int, default=2, choices=(1, 2), help="mirror of the two-stage exact search: 2 = bytes (default), 1 = bf16")
    ap.add_argument("--backend", default="auto", help="torch.distributed backend: nccl (== RCCL), gloo, or auto = nccl when every rank has "
                                                      "its own GPU, gloo when ranks share one (rehearsals)")
    ap.add_argument("--sharded-probe", action="store_true", help="(internal) the ONE-process form over every visible GPU — mi_knn_sharded + "
                    "mi_pipeline_create_sharded — as a child of the N = 1 run; prints one JSON object")
    ap.add_argument("--dry-run", action="store_true", help="no GPU work: launch, rendezvous, the exchange + merge over fake per-rank lists "
                                                          "(what the CPU test of the self-launch path runs)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def self_launch(args) -> int:
    """`python bench.py --gpus N` with no launcher around it: start the N ranks as a CHILD process (never an exec:
    a process that has touched the GPU must not be replaced, and this one must not touch it at all), relay rank 0's
    JSON line, return the child's exit code."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL between processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    log(f"[bench] --gpus {args.gpus} without a launcher: starting {args.gpus} ranks: {' '.join(cmd)}")
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
    line = None
    for out in child.stdout:
        if out.lstrip().startswith('{"metric"'):
            line = out.strip()
        else:
            sys.stderr.write(out)
    rc = child.wait()
    if line is not None:
        print(line, flush=True)
    elif rc == 0:
        log("[bench] the ranks exited without a result line")
        rc = 1
    return rc


def _profile_meta():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import profile_meta
    return profile_meta


def gemm_in_situ(batch):
    """What the persistent GEMM reaches INSIDE the tower, from the newest committed rocprofv3 kernel statistics of this
    command run as ONE stream (profiles/rNN_bench_kernel_stats_single_stream.csv: kernel durations add up there; in the
    two-stream run they overlap) — not an observation of this run, and reported under `roofline.from_profile` only while
    the profile's stamp (tools/profile_meta.py: batch, model, git blob ids of the kernel sources at the time it was taken)
    matches the sources this run executes and this run's batch.  frac = the four linears' FLOPs / their kernel time."""
    import csv
    import glob
    import re
    found = []
    for f in glob.glob(os.path.join(ROOT, "profiles", "r*_bench_kernel_stats_single_stream.csv")):
        mo = re.match(r"r(\d+)_", os.path.basename(f))
        if mo:
            found.append((int(mo.group(1)), f))
    if not found:
        return {"source": None, "refused": "no profiles/rNN_bench_kernel_stats_single_stream.csv"}
    path = max(found)[1]
    pm = _profile_meta()
    rel = os.path.relpath(path, ROOT)
    meta, stale = pm.check(path)
    head = {"source": rel, "source_git_blob": pm.git_blob_id(path)}
    if stale:
        return dict(head, refused=stale)
    if meta.get("batch") != batch:
        return dict(head, refused=f"the profile was taken at batch {meta.get('batch')}, this run is batch {batch}")
    rows = list(csv.DictReader(open(path)))
    ns = sum(float(r["TotalDurationNs"]) for r in rows if "gemm_bf16_pp_kernel" in r["Name"])
    calls = max((int(r["Calls"]) for r in rows if "gemm_bf16_pp_kernel<6" in r["Name"]), default=0)
    forwards = calls / 46.0 if calls else 0   # EPI_RESID24: out_proj + fc2 of layers 0 .. 22 of ViT-L/14 (the stamped model)
    if not forwards or not ns:
        return dict(head, refused="no gemm_bf16_pp_kernel<6> rows in the profile")
    per_forward_ms = ns / forwards / 1e6
    flop = batch * 257 * 2.0 * (3 * 1024 * 1024 + 1024 * 1024 + 2 * 4096 * 1024) * 23   # the 23 full layers the kernel runs
    return dict(head, command="MI_CLIP_PARTS=1 rocprofv3 --kernel-trace --stats -- python3 bench.py --full (tools/round_profile.sh)",
                gemm_ms_per_forward=round(per_forward_ms, 3), forwards_in_profile=round(forwards, 1),
                TFLOP_per_s=round(flop / (per_forward_ms * 1e-3) / 1e12, 1),
                frac=round(flop / (per_forward_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                note="epilogues included: bias, the folded LayerNorm, the residual add and the row sums run inside these kernels")


def pmc_traffic(args):
    """profiles/pmc_latest.json (separate --pmc passes of this command), or (None, reason) when it was not taken on this
    code at this size"""
    path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    try:
        with open(path) as f:
            pmc = json.load(f)
    except (OSError, ValueError):
        return None, "no profiles/pmc_latest.json"
    if pmc.get("rows") != args.rows or pmc.get("batch") != args.batch:
        return None, f"taken at rows={pmc.get('rows')} batch={pmc.get('batch')}"
    _, stale = _profile_meta().check(path)
    if stale:
        return None, stale
    return pmc, None


def cpu_baseline(weights, cfg):
    """The CPU side of the same workload, timed on this host's cores on a bounded sample.  "port": the oracle
    (fixed summation orders: numpy ViT, OpenMP C kNN).  "library": the same two kernels as fast as torch-CPU runs
    them (oracle/vit_torch.py: oneDNN / MKL GEMMs, fused attention, topk) — the CPU number someone would deploy.
    Only this function and the parity tests touch oracle/."""
    import torch

    from image_search_amd import synth
    from oracle import vit_numpy, vit_torch
    from oracle.binding import load_oracle, orc_gen_f32, orc_knn

    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    # ViT: numpy fp32 restatement (BLAS threads = all cores): b = 1 (latency) and b = 8 (BASELINE.md §3
    # planned b = 32; at < 1 image/s that alone would be > 40 s of a run that must finish in minutes)
    px = synth.preprocess_rgb8(synth.images_u8(100, 32, cfg.image))
    vit_numpy.vit_forward(weights, cfg, px[:1], np.float32)  # warm BLAS
    t0 = time.perf_counter()
    vit_numpy.vit_forward(weights, cfg, px[:1], np.float32)
    t_one = time.perf_counter() - t0
    t0 = time.perf_counter()
    vit_numpy.vit_forward(weights, cfg, px[:8], np.float32)
    t_vit = time.perf_counter() - t0
    # kNN: C restatement (OpenMP), 1M x 768 rows, 5 queries
    orc = load_oracle()
    n = 1_000_000
    rows = orc_gen_f32(orc, 0, 0, n * 768, 1.0).reshape(n, 768)
    qs = synth.corpus_rows(1, 0, 5)
    orc_knn(orc, qs[0], rows, 10)
    t0 = time.perf_counter()
    for q in qs:
        orc_knn(orc, q, rows, 10)
    t_knn = (time.perf_counter() - t0) / len(qs)
    out = {
        "value": round(8 / t_vit, 3), "unit": "images/s", "cores": cores, "kind": "port",
        "sample": "oracle/vit_numpy.py fp32 ViT-L/14, ONE batch of 8 images (numpy+BLAS, all cores; b=1 latency beside it); "
                  "kNN below: oracle/oracle.c orc_knn (OpenMP) top-10 over 1M x 768, mean of 5 queries",
        "vit_b1_seconds": round(t_one, 3), "vit_b8_seconds": round(t_vit, 3),
        "knn": {"value": round(1.0 / t_knn, 2), "unit": "queries/s over 1M rows",
                "equiv_10M": round(0.1 / t_knn, 3), "threads": int(orc.orc_threads())},
    }
    # the library-grade CPU point: torch, all cores
    try:
        # the box may give this process fewer CPUs than it shows (a cgroup share): take the thread count torch's own
        # GEMM runs fastest with, and say which
        a = torch.randn(2048, 2048)
        best, threads = None, 1
        for nt in [n for n in (8, 16, 32, 64, 128, 256) if n <= max(cores, 8)]:
            torch.set_num_threads(nt)
            torch.mm(a, a)
            t0 = time.perf_counter()
            for _ in range(3):
                torch.mm(a, a)
            dt = time.perf_counter() - t0
            if best is None or dt < best:
                best, threads = dt, nt
        torch.set_num_threads(threads)
        W = vit_torch.load_weights(weights)
        vit_torch.vit_forward(W, cfg, px[:8])  # warm
        t0 = time.perf_counter()
        vit_torch.vit_forward(W, cfg, px[:8])
        t8 = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref32 = vit_torch.vit_forward(W, cfg, px)
        t32 = time.perf_counter() - t0
        port8 = vit_numpy.vit_forward(weights, cfg, px[:2], np.float32)
        agree = float(np.abs(ref32[:2].numpy() - port8).max() / np.sqrt((port8 ** 2).mean()))
        tr = torch.from_numpy(rows)
        norms = tr.norm(dim=1)
        tq = torch.from_numpy(qs)
        ti, _ = vit_torch.knn(tr, norms, tq[0], 10)
        oi, _ = orc_knn(orc, qs[0], rows, 10)
        t0 = time.perf_counter()
        for u in range(len(qs)):
            vit_torch.knn(tr, norms, tq[u], 10)
        tk = (time.perf_counter() - t0) / len(qs)
        out["library"] = {
            "kind": "library", "what": "oracle/vit_torch.py: torch-CPU fp32 (F.linear / scaled_dot_product_attention / topk), "
                                       "library summation order", "threads": threads,
            "threads_chosen_by": "fastest 2048^3 torch.mm among 8..256 threads (the box may grant fewer CPUs than it lists)",
            "vit_b8_images_per_sec": round(8 / t8, 2), "vit_b32_images_per_sec": round(32 / t32, 2),
            "vit_b32_TFLOP_per_s": round(32 * VIT_FLOP_PER_IMAGE / t32 / 1e12, 3),
            "vit_max_err_vs_port_over_rms": round(agree, 8),
            "knn_1m_queries_per_sec": round(1.0 / tk, 2), "knn_equiv_10M_queries_per_sec": round(0.1 / tk, 3),
            "knn_GB_per_s": round(n * 3072 / tk / 1e9, 1), "knn_top10_ids_equal_port": bool(np.array_equal(ti.numpy().astype(np.uint64), oi)),
        }
    except Exception as e:  # noqa: BLE001 — a baseline that cannot run must not take the GPU line with it
        out["library"] = {"kind": "library", "error": f"{type(e).__name__}: {e}"}
    return out


def sharded_probe(args) -> int:
    """BASELINE config 5 as the reference's ONE server process would run it (server/src/main.rs:30-35): one table over every
    visible GPU (on a one-GPU box: two shards on GPU 0), a tower replica per shard, ingest + query through
    mi_pipeline_create_sharded.  Small on purpose (it rides along with the N = 1 bench): rows_per_shard rows per shard."""
    import torch

    from image_search_amd import synth
    from image_search_amd.clip import PRECISION_BF16, Model
    from image_search_amd.search import EmbeddingTable, PinnedBuffer, Pipeline, ShardedTable

    n_dev = torch.cuda.device_count()
    devices = list(range(n_dev)) if n_dev > 1 else [0, 0]
    n = len(devices)
    rows_per_shard, batch = 1_000_000, args.batch
    cfg = synth.VitConfig.vit_l14()
    wpath, own_weights = os.environ.get("MI_BENCH_WEIGHTS", ""), False   # the parent bench's file, or (run by hand) one of its own
    if not wpath or not os.path.exists(wpath):
        wpath, own_weights = os.path.join(tempfile.gettempdir(), f"mi355clip_bench_vitl14_seed0_{os.getpid()}.safetensors"), True
        synth.save_safetensors(synth.vit_weights(cfg, 0), wpath, {"num_attention_heads": cfg.heads})
    out = {"devices": devices, "shards": n}
    # 1. the search: small table against one mi_knn (bit equality), then rows_per_shard per shard (timing)
    small = ShardedTable(768, devices, 256)
    small.insert_synthetic(5, 0, 200_000)
    one = EmbeddingTable(768, devices[0])
    one.insert_synthetic(5, 0, 200_000)
    qs = synth.corpus_rows(6, 0, 8)
    eq = True
    for k in (10, 1000):
        a, b = small.knn(qs, k), one.knn(qs, k)
        eq = eq and bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))
    out["transport"] = small.info()["transport"]
    out["exchange_stats"] = small.stats()   # collectives > 0 <=> the library's own ncclAllGather ran (distinct devices)
    out["equal_to_one_table"] = eq
    small.close(); one.close()
    big = ShardedTable(768, devices, batch)
    big.reserve(n * rows_per_shard + 64 * batch * n)
    big.insert_synthetic(0, 0, n * rows_per_shard)
    for mode in (0, 2):
        big.set_option("prefilter", mode)
        for u in range(3):
            big.knn(qs[u], args.k)
        t0 = time.perf_counter()
        pend = [big.knn_async(qs[u % 8], args.k) for u in range(24)]
        big.sync()
        ms = (time.perf_counter() - t0) / 24 * 1e3
        out["knn_ms_per_query" + ("_two_stage" if mode else "")] = round(ms, 4)
    out["rows"] = len(big)
    # 2. scan task + search handler in the one process: a replica per shard, chunks of n x batch images
    models = [Model.from_file(wpath, d, PRECISION_BF16) for d in (devices if n_dev > 1 else devices[:1])]
    if n_dev <= 1:
        models = models * n
    pipe = Pipeline(models, big)
    pins = [PinnedBuffer((n * batch, 3, cfg.image, cfg.image)) for _ in range(2)]
    img = synth.preprocess_rgb8(synth.images_u8(77, batch, cfg.image))
    for pb in pins:
        for j in range(n):
            pb.array[j * batch:(j + 1) * batch] = img
    steps = 4
    for i in range(2):
        pipe.ingest(pins[i & 1].array); pipe.query(qs[0], args.k)
    pipe.sync()
    t0 = time.perf_counter()
    res = []
    for i in range(steps):
        pipe.ingest(pins[i & 1].array)
        res.append(pipe.query(qs[i % 8], args.k))
    pipe.sync()
    dt = time.perf_counter() - t0
    out["pipeline_images_per_sec"] = round(steps * n * batch / dt, 1)
    out["pipeline_ms_per_step"] = round(dt / steps * 1e3, 3)
    out["pipeline_images_per_step"] = n * batch
    out["rows_after"] = len(big)
    out["shard_rows"] = [big.shard_rows(sidx) for sidx in range(n)]
    pipe.close()
    for m in set(models):
        m.close()
    big.close()
    for pb in pins:
        pb.close()
    if own_weights:
        os.unlink(wpath)
    # last, guarded, and with everything above already measured: on a real multi-GPU node this path has never run
    try:
        out["exchange_cost"] = exchange_cost(args, devices[0], float(os.environ.get("MI_BENCH_T_SCAN_MS", "0")) or None)
    except Exception as e:  # noqa: BLE001
        out["exchange_cost"] = {"error": f"{type(e).__name__}: {e}"}
    print("SHARDED_PROBE " + json.dumps(out), flush=True)
    return 0


def exchange_cost(args, device, t_scan=None):
    """What the exchange step itself costs, as far as ONE GPU can say: a one-shard table made with
    the RCCL transport runs the library's real path — ncclAllGather of the packed [k x u64 | k x f32] record on a
    one-rank communicator + the device merge + the readback — against the same table without an exchange.  Blocking
    searches (one query per request, server/src/search.rs:70-86), 1 M rows, the two-stage search.  A one-rank
    all-gather has no wire time: on 8 GPUs the ring adds 7 hops of xGMI latency for 120-byte records."""
    from image_search_amd import synth
    from image_search_amd.search import ShardedTable

    qs = synth.corpus_rows(6, 0, 8)
    res = {}
    for name, transport in (("no_exchange", None), ("rccl_one_rank", "rccl")):
        if transport:
            os.environ["MI_KNN_SHARDED_TRANSPORT"] = transport
        try:
            t = ShardedTable(768, [device], args.batch)
        finally:
            os.environ.pop("MI_KNN_SHARDED_TRANSPORT", None)
        t.insert_synthetic(0, 0, 1_000_000)
        t.set_option("prefilter", 2)
        for u in range(8):
            t.knn(qs[u], args.k)
        lat = []
        for u in range(64):
            t0 = time.perf_counter()
            t.knn(qs[u % 8], args.k)
            lat.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        pend = [t.knn_async(qs[u % 8], args.k) for u in range(64)]
        t.sync()
        thr = (time.perf_counter() - t0) / 64 * 1e3
        res[name] = {"transport": t.info()["transport"], "ms_per_blocking_search_median": round(float(np.median(lat)), 4),
                     "ms_per_blocking_search_min": round(float(np.min(lat)), 4), "ms_per_search_pipelined": round(thr, 4),
                     "stats": t.stats()}
        del pend
        t.close()
    ex_lat = res["rccl_one_rank"]["ms_per_blocking_search_median"] - res["no_exchange"]["ms_per_blocking_search_median"]
    ex_thr = res["rccl_one_rank"]["ms_per_search_pipelined"] - res["no_exchange"]["ms_per_search_pipelined"]
    if t_scan is None:   # run by hand: no parent bench measured the 10 M scan
        res.update({"rows": 1_000_000, "k": args.k, "exchange_ms_blocking": round(ex_lat, 4), "exchange_ms_pipelined": round(ex_thr, 4)})
        return res
    # t_scan: the two-stage scan of one GPU's 10 M rows as THIS run measured it (BENCH: knn.ms_per_query)
    res.update({"rows": 1_000_000, "k": args.k,
                "exchange_ms_blocking": round(ex_lat, 4), "exchange_ms_pipelined": round(ex_thr, 4),
                "projection_8_gpus": {"t_scan_ms": t_scan, "speedup_blocking": round(8 * t_scan / (t_scan + max(ex_lat, 0.0)), 2),
                                      "speedup_pipelined": round(8 * t_scan / (t_scan + max(ex_thr, 0.0)), 2),
                                      "note": "8 t_scan / (t_scan + t_exchange): a PROJECTION from a one-rank collective, unmeasured on > 1 GPU"}})
    return res


def run_sharded_probe(args, wpath, t_scan_ms=None):
    """the probe as a CHILD with its own deadline: a hang in a multi-GPU runtime call must not take the N = 1 line with it"""
    cmd = [sys.executable, os.path.abspath(__file__), "--sharded-probe", "--batch", str(args.batch), "--k", str(args.k)]
    try:
        env = dict(os.environ, MI_BENCH_WEIGHTS=wpath)
        if t_scan_ms:
            env["MI_BENCH_T_SCAN_MS"] = repr(float(t_scan_ms))
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    except subprocess.TimeoutExpired:
        return {"error": "timed out after 240 s"}
    for ln in r.stdout.splitlines():
        if ln.startswith("SHARDED_PROBE "):
            return json.loads(ln[len("SHARDED_PROBE "):])
    return {"error": f"rc {r.returncode}: {r.stderr.strip().splitlines()[-1] if r.stderr.strip() else 'no output'}"}


def dry_run(args, world, rank):
    """--dry-run: everything of the N-rank path that needs no GPU — launch, rendezvous, the packed all-gather and the
    merge through the C ABI — over fake per-rank lists whose merged answer is known."""
    import torch.distributed as dist

    from image_search_amd.search import ShardExchange
    if world > 1:
        dist.init_process_group("gloo")
    k = args.k
    # rank r holds global ids r, r + world, r + 2 world, ... with distance id / 1000: merged top-k = ids 0..k-1
    ids = (np.arange(k, dtype=np.uint64) * world + rank)
    dd = (ids.astype(np.float32) / np.float32(1000.0)).astype(np.float32)
    t0 = time.perf_counter()
    ok = True
    if world > 1:
        ex = ShardExchange(k, depth=2)
        for _ in range(args.warmup + args.steps):
            ex.submit(ids, dd)
            mi, md = ex.collect()
            ok = ok and np.array_equal(mi, np.arange(k, dtype=np.uint64)) and \
                np.array_equal(md, (np.arange(k, dtype=np.uint64).astype(np.float32) / np.float32(1000.0)))
        # the verdict of EVERY rank, not just rank 0's: all lists identical to the known answer everywhere
        import torch
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        ok = bool(flag.item())
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if rank == 0:
        print(json.dumps({"metric": METRIC, "value": 0.0, "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / max(1, args.steps + args.warmup) * 1e3, 3), "higher_is_better": True,
                          "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic", "dry_run": True,
                          "exchange_ok": bool(ok), "config": {"workload": "dry run: launch + rendezvous + exchange + merge only (no GPU work)"}}),
              flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0 if ok else 1


def main():
    args = parse_args()
    # dmabuf IPC: RCCL between processes needs it on this driver.  Set before torch / HIP is loaded, so that the documented
    # `python -m torch.distributed.run ... bench.py` form gets it as the self-launch form does.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args)  # nothing above imported torch or touched HIP

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started {world} ranks")
    if args.dry_run:
        return dry_run(args, world, rank)
    if args.sharded_probe:
        return sharded_probe(args)

    import torch
    import torch.distributed as dist

    from image_search_amd import synth
    from image_search_amd.clip import PRECISION_BF16, PRECISION_F32, Model
    from image_search_amd.search import EmbeddingTable, PinnedBuffer, Pipeline, ShardExchange

    n_dev = max(1, torch.cuda.device_count())   # counting devices does not initialise the GPU
    shared_gpu = world > n_dev                  # a rehearsal: several ranks on one GPU
    backend = args.backend
    if backend == "auto":
        backend = "gloo" if shared_gpu else "nccl"   # RCCL refuses one GPU twice
    local = local % n_dev
    torch.cuda.set_device(local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)

    def barrier():
        if world > 1:
            dist.barrier()

    # ---- untimed setup -------------------------------------------------------------
    cfg = synth.VitConfig.vit_l14()
    # one file per run (two benches on one box must not race on it): the rendezvous port names a multi-rank job, the pid a single one
    job = os.environ.get("MASTER_PORT", "") if world > 1 else ""
    wpath = os.path.join(tempfile.gettempdir(), f"mi355clip_bench_vitl14_seed0_{job or os.getpid()}.safetensors")
    weights = None
    if rank == 0:
        t0 = time.time()
        weights = synth.vit_weights(cfg, 0)
        synth.save_safetensors(weights, wpath + ".tmp", {"num_attention_heads": cfg.heads})
        os.replace(wpath + ".tmp", wpath)
        log(f"[bench] seeded ViT-L/14 weights written in {time.time() - t0:.1f}s")
    barrier()
    model = Model.from_file(wpath, local, PRECISION_BF16)
    if args.front_overlap is not None:
        model.set_option("front_overlap", args.front_overlap)
    total_steps = args.warmup + args.steps
    # the step's input: a batch in PINNED host memory (what the server's decode threads would fill),
    # two buffers so that batch i+1 uploads under the forward of batch i
    pins = [PinnedBuffer((args.batch, 3, cfg.image, cfg.image)) for _ in range(2)]
    for j, pb in enumerate(pins):
        pb.array[:] = synth.preprocess_rgb8(synth.images_u8(1000 + 2 * rank + j, args.batch, cfg.image))

    appended = (2 * total_steps + 1) * args.batch          # the headline loop, then the same steps with the single-pass query
    table = EmbeddingTable(768, local, base=rank * (args.rows + appended))
    table.reserve(args.rows + appended)  # the appended rows never reallocate the table
    table.insert_synthetic(0, rank * args.rows, args.rows)
    if not args.no_prefilter:
        table.set_option("prefilter", args.prefilter)  # the mirror is built by the first (warm-up) query and caught up by every later one
    n_q = 64
    queries = synth.corpus_rows(1, 0, n_q)
    pipe = Pipeline(model, table)
    lag = 0 if args.serial else 1           # results of query i are consumed while query i+1 scans
    ex = ShardExchange(args.k, depth=4) if world > 1 else None
    merged, pending, last = [], [], {}

    def consume(leave):
        """host side of the exchange, `leave` queries behind the scan"""
        if ex is None:
            return
        if not ex.on_device:
            pipe.drain(leave)                # results of the older queries are on the host now
            while len(pending) > leave:
                ex.submit(*pending.pop(0))
        while ex.in_flight() > (leave if ex.on_device else 0):
            merged.append(ex.collect())

    def step(i):
        # BASELINE config 4: H2D of the batch -> bf16 tower -> rows appended on the device -> top-k over
        # table + appended rows -> D2H of the k results; the scan of step i runs on the search stream
        # (mi_pipeline_*, include/mi355clip.h).  N > 1: the k results stay on the device, are all-gathered
        # (one collective of 12 k bytes per rank) and merged on every rank one step behind the scan.
        pipe.ingest(pins[i & 1].array)
        if ex is not None and ex.on_device:
            ex.query(pipe, queries[i % n_q])
        else:
            last["query"] = pipe.query(queries[i % n_q], args.k)   # filled in by the sync that delivers it
            pending.append(last["query"])
        if args.serial:
            pipe.sync()
        consume(lag)

    def finish():
        pipe.sync()
        consume(0)
        pending.clear()

    def timed(first, n):
        """exactly n steps between barrier + synchronize on both sides; the maximum over ranks"""
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            step(first + i)
        finish()
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    for i in range(args.warmup):
        step(i)
    finish()
    pipe.stats(reset=True)
    merged.clear()
    elapsed = timed(args.warmup, args.steps)
    n_f, ms_f, n_s, ms_s = pipe.stats()
    n_merged = len(merged)
    if args.dump_outputs and rank == 0:
        # the last timed step: its query's k results (N > 1: the merged lists every rank receives) and its batch's rows
        last_ids, last_dist = merged[-1] if world > 1 else last["query"]
        emb = table.rows(len(table) - args.batch, args.batch)
        if emb.nbytes > 48 << 20:   # the dump stays under 64 MB: a fixed, seeded sample of the rows
            emb = emb[np.sort(np.random.default_rng(0).choice(args.batch, (48 << 20) // emb[0].nbytes, replace=False))]
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in (("knn_ids", last_ids.astype(np.float64)), ("knn_distances", last_dist.astype(np.float32)),
                        ("embeddings", emb)):
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
    # The same steps once more with the query as ONE pass over the fp32 rows (the kernel that carries the kNN roofline
    # credit): `value_single_pass_query`.  Behind the headline loop, never inside it; the table was reserved for these rows too.
    elapsed_single = None
    if args.full and not args.no_prefilter:
        table.set_option("prefilter", 0)
        step(total_steps)
        finish()
        elapsed_single = timed(total_steps + 1, args.steps)
        table.set_option("prefilter", args.prefilter)
        del merged[n_merged:]
    ms_vit = ms_f / max(n_f, 1)          # HIP events on the ingest stream around each forward, timed region only
    ms_knn_overlapped = ms_s / max(n_s, 1)
    exchange_check = None
    if args.full and world > 1:
        # every rank must hold the same merged lists, each sorted and made of ids of all shards' ranges
        mine = np.stack([np.concatenate([m[0].view(np.uint8), m[1].view(np.uint8)]) for m in merged]) if merged else np.zeros((0, 1), np.uint8)
        g = [None] * world
        dist.all_gather_object(g, mine.tobytes())
        same = all(x == g[0] for x in g)
        sorted_ok = all(bool(np.all(np.diff(m[1]) >= 0)) for m in merged)
        exchange_check = {"queries_merged": len(merged), "identical_on_every_rank": bool(same), "sorted": bool(sorted_ok)}
        if rank == 0 and not (same and sorted_ok and len(merged) == args.steps):
            log(f"[bench] exchange check FAILED: {exchange_check}")

    extra = {}
    two_stage_equal = None
    if args.full and rank == 0:
        # ---- the kNN kernel by itself (same table): HIP events on the launch stream --------------
        stream = torch.cuda.Stream()
        d_q = torch.from_numpy(queries).cuda()
        ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731

        def time_knn(tbl, k, reps, keep=0):
            """ms per query; with keep > 0 also the (ids, distance bits) of the first `keep` queries"""
            d_i = torch.empty((max(keep, 1), k), dtype=torch.int64, device="cuda")
            d_d = torch.empty((max(keep, 1), k), dtype=torch.float32, device="cuda")
            for i in range(max(2, keep)):
                j = i if i < keep else 0
                tbl.knn_device(d_q[i % n_q].data_ptr(), 1, k, d_i[j].data_ptr(), d_d[j].data_ptr(), stream.cuda_stream)
            stream.synchronize()
            kept = (d_i.cpu().numpy().copy(), d_d.cpu().numpy().view(np.uint32).copy()) if keep else None
            a, b = ev(), ev()
            a.record(stream)
            for i in range(reps):
                tbl.knn_device(d_q[i % n_q].data_ptr(), 1, k, d_i[0].data_ptr(), d_d[0].data_ptr(), stream.cuda_stream)
            b.record(stream)
            stream.synchronize()
            ms = a.elapsed_time(b) / reps
            return (ms, kept) if keep else ms

        # the single pass over the fp32 rows (the roofline kernel), then what the step actually ran
        table.set_option("prefilter", 0)
        ms_knn, ref_res = time_knn(table, args.k, 20, keep=16)
        ms_knn_two, pref_cand, pref_fell_back = None, 0, False
        if not args.no_prefilter:
            table.set_option("prefilter", args.prefilter)
            ms_knn_two, two_res = time_knn(table, args.k, 20, keep=16)
            pref_cand, pref_fell_back = table.prefilter_stats()
            two_stage_equal = bool(np.array_equal(ref_res[0], two_res[0]) and np.array_equal(ref_res[1], two_res[1]))
            if not two_stage_equal:
                log("[bench] the two-stage search and the single pass DISAGREE on the timed queries")
    pipe.close()

    if args.full and rank == 0 and world == 1 and not args.no_extra_configs:
        # BASELINE config 3 (1 M rows; k = 10 and the reference's k = 1000) and config 2 (fp32 b = 32)
        rows_total = len(table)
        t1m = EmbeddingTable(768, local)
        t1m.insert_synthetic(0, 0, 1_000_000)
        for k in (10, 1000):
            ms = time_knn(t1m, k, 50)
            extra[f"knn_1m_k{k}"] = {"config": f"cosine top-{k} over 1M x 768 f32, 1 query per pass", "ms_per_query": round(ms, 4),
                                     "queries_per_sec": round(1e3 / ms, 1), "GB_per_s": round(3.072 / ms * 1e3, 1),
                                     "frac_of_hbm_peak": round(3.072 / ms * 1e3 / PEAK_HBM_GBS, 4)}
        if not args.no_prefilter:
            t1m.set_option("prefilter", args.prefilter)
            for k in (10, 1000):
                ms = time_knn(t1m, k, 50)
                extra[f"knn_1m_k{k}"]["two_stage_ms_per_query"] = round(ms, 4)
        t1m.close()
        table.set_option("prefilter", 0)
        ms, ref1000 = time_knn(table, 1000, 10, keep=4)
        extra["knn_10m_k1000"] = {"config": f"cosine top-1000 over {rows_total} x 768 f32 (the reference's K)", "ms_per_query": round(ms, 4),
                                  "GB_per_s": round(rows_total * 3072 / ms / 1e6, 1),
                                  "frac_of_hbm_peak": round(rows_total * 3072 / ms / 1e6 / PEAK_HBM_GBS, 4)}
        if not args.no_prefilter:
            table.set_option("prefilter", args.prefilter)
            ms, two1000 = time_knn(table, 1000, 10, keep=4)
            extra["knn_10m_k1000"]["two_stage_ms_per_query"] = round(ms, 4)
            eq = bool(np.array_equal(ref1000[0], two1000[0]) and np.array_equal(ref1000[1], two1000[1]))
            extra["knn_10m_k1000"]["two_stage_equal"] = eq
            two_stage_equal = bool(two_stage_equal and eq)
            table.set_option("prefilter", 0)
        # the throughput form: 8 queries per call (mi_knn_search_batched_device) — one pass over the fp32 rows, or, with the
        # byte mirror, one stage-1 pass for all 8 and a stage 2 each; same ids and distance bits as 8 single searches
        def time_batched(tbl, k, nq, reps):
            d_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            d_d = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            for _ in range(2):
                tbl.knn_device(d_q.data_ptr(), nq, k, d_i.data_ptr(), d_d.data_ptr(), stream.cuda_stream, batched=True)
            stream.synchronize()
            a, b = ev(), ev()
            a.record(stream)
            for _ in range(reps):
                tbl.knn_device(d_q.data_ptr(), nq, k, d_i.data_ptr(), d_d.data_ptr(), stream.cuda_stream, batched=True)
            b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b) / reps, d_i.cpu().numpy().copy(), d_d.cpu().numpy().view(np.uint32).copy()
        ms8, i8, b8 = time_batched(table, args.k, 8, 10)
        extra["knn_10m_batched8"] = {"config": f"8 queries per call, cosine top-{args.k} over {rows_total} x 768 f32, one pass over the fp32 rows",
                                     "ms_per_call": round(ms8, 4), "queries_per_sec": round(8e3 / ms8, 1)}
        if not args.no_prefilter and args.prefilter == 2:
            table.set_option("prefilter", 2)
            ms8t, i8t, b8t = time_batched(table, args.k, 8, 10)
            extra["knn_10m_batched8"].update({"two_stage_ms_per_call": round(ms8t, 4), "two_stage_queries_per_sec": round(8e3 / ms8t, 1),
                                              "two_stage_equal": bool(np.array_equal(i8, i8t) and np.array_equal(b8, b8t)),
                                              "stage1": "int8 MFMA over the byte mirror, one launch per kernel for the group"})
            two_stage_equal = bool(two_stage_equal and extra["knn_10m_batched8"]["two_stage_equal"])
            # 16 queries per call: one group on the matrix pipe; the reference answers from two passes of 8 over the fp32 rows
            ms16t, i16t, b16t = time_batched(table, args.k, 16, 10)
            table.set_option("prefilter", 0)
            _, i16a, b16a = time_batched(table, args.k, 8, 1)
            d_q2 = d_q[8:16].contiguous()
            d_i2 = torch.empty((8, args.k), dtype=torch.int64, device="cuda"); d_d2 = torch.empty((8, args.k), dtype=torch.float32, device="cuda")
            table.knn_device(d_q2.data_ptr(), 8, args.k, d_i2.data_ptr(), d_d2.data_ptr(), stream.cuda_stream, batched=True)
            stream.synchronize()
            ref_i = np.concatenate([i16a, d_i2.cpu().numpy()]); ref_b = np.concatenate([b16a, d_d2.cpu().numpy().view(np.uint32)])
            extra["knn_10m_batched16"] = {"config": f"16 queries per call, cosine top-{args.k} over {rows_total} x 768 f32, two-stage exact search, one group",
                                          "two_stage_ms_per_call": round(ms16t, 4), "two_stage_queries_per_sec": round(16e3 / ms16t, 1),
                                          "two_stage_equal": bool(np.array_equal(i16t, ref_i) and np.array_equal(b16t, ref_b))}
            two_stage_equal = bool(two_stage_equal and extra["knn_10m_batched16"]["two_stage_equal"])
        m32 = Model.from_file(wpath, local, PRECISION_F32)
        d_img = torch.from_numpy(np.ascontiguousarray(pins[0].array[:32])).cuda()
        d_emb = torch.empty((32, cfg.proj), dtype=torch.float32, device="cuda")
        for _ in range(2):
            m32.forward_device(d_img.data_ptr(), 32, d_emb.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        a, b = ev(), ev()
        a.record(stream)
        for _ in range(5):
            m32.forward_device(d_img.data_ptr(), 32, d_emb.data_ptr(), stream.cuda_stream)
        b.record(stream)
        stream.synchronize()
        ms = a.elapsed_time(b) / 5
        tf = 32 * VIT_FLOP_PER_IMAGE / (ms * 1e-3) / 1e12
        extra["vit_fp32_b32"] = {"config": "ViT-L/14 image encoder, batch=32 fp32 (exact-f32 MFMA, the parity path), inputs resident",
                                 "ms_per_batch": round(ms, 3), "images_per_sec": round(32e3 / ms, 1), "TFLOP_per_s": round(tf, 1),
                                 "frac_of_f32_mfma_peak": round(tf / PEAK_F32_TFLOPS, 4)}
        # the parity precision at the headline batch (server/src/clip.rs:112-118 computes in fp32; north_star's 1e-4 holds here)
        nb = args.batch
        d_img = torch.from_numpy(np.ascontiguousarray(pins[0].array[:nb])).cuda()
        d_emb = torch.empty((nb, cfg.proj), dtype=torch.float32, device="cuda")
        m32.forward_device(d_img.data_ptr(), nb, d_emb.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        a, b = ev(), ev()
        a.record(stream)
        for _ in range(5):
            m32.forward_device(d_img.data_ptr(), nb, d_emb.data_ptr(), stream.cuda_stream)
        b.record(stream)
        stream.synchronize()
        ms = a.elapsed_time(b) / 5
        tf = nb * VIT_FLOP_PER_IMAGE / (ms * 1e-3) / 1e12
        if nb != 32:   # at --batch 32 the line above is this one
            extra[f"vit_fp32_b{nb}"] = {"config": f"ViT-L/14 image encoder, batch={nb} fp32 (exact-f32 MFMA, the parity path: <= 1e-4 of the oracle), inputs resident",
                                    "ms_per_batch": round(ms, 3), "images_per_sec": round(nb * 1e3 / ms, 1), "TFLOP_per_s": round(tf, 1),
                                    "frac_of_f32_mfma_peak": round(tf / PEAK_F32_TFLOPS, 4)}
        m32.close()

    failed = False
    if rank == 0:
        imgs = world * args.batch * args.steps
        out = {
            "metric": METRIC,
            "value": round(imgs / elapsed, 2),
            "unit": "images/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic",
            "config": {"workload": f"BASELINE config 4: per step, H2D of a pinned batch of {args.batch} 224x224x3 f32 images -> bf16 ViT-L/14 "
                                   f"(random-init seeded weights) -> {args.batch} rows appended to the table on the device -> cosine "
                                   f"top-{args.k} query over {args.rows}+ x 768 fp32 rows per GPU -> D2H of the k results; fused on HIP "
                                   "streams (the upload runs under the previous batch's tower; the scan is asynchronous to the host and runs between towers)"
                                   + ("; query = ONE pass over the fp32 rows" if args.no_prefilter else
                                      ("; query = two-stage EXACT search: a byte mirror of the rows with a per-row scale (+25 % HBM) prefilters, the rows a "
                                       "rigorous per-row error bound cannot exclude" if args.prefilter == 2 else
                                       "; query = two-stage EXACT search: a bf16 mirror of the rows (+50 % HBM) prefilters, the rows within a "
                                       "data-independent error bound of the k-th") + " are re-evaluated from the fp32 rows: ids and distance bits of the single pass")
                                   + (f"; BASELINE config 5 shape: {world} ranks x {args.rows} rows, per-shard top-k all-gathered ({backend}) and merged on every rank"
                                      if world > 1 else "")
                                   + ("; --serial: no overlap" if args.serial else ""),
                       "batch": args.batch, "rows_per_gpu": args.rows, "k": args.k, "queries_per_step": 1,
                       "transfers_in_timed_region": True,
                       "sharding": "ViT replicas; table row-sharded, all-gather of per-shard top-k",
                       "backend": backend if world > 1 else None, "ranks_share_one_gpu": bool(shared_gpu)},
            "vit": {"images_per_sec": round(world * args.batch / (ms_vit * 1e-3), 1), "ms_per_batch": round(ms_vit, 3),
                    "note": "HIP events on the ingest stream around each forward of the timed region (one forward at a time on the ingest stream)"},
        }
        if args.full:
            executed = VIT_FLOP_PER_IMAGE - VIT_FLOP_SKIPPED_PER_IMAGE
            tf_exec = args.batch * executed / (ms_vit * 1e-3) / 1e12
            tf_alg = args.batch * VIT_FLOP_PER_IMAGE / (ms_vit * 1e-3) / 1e12
            knn_gbs = len(table) * 768 * 4 / (ms_knn * 1e-3) / 1e9
            pmc, pmc_refused = pmc_traffic(args)
            traffic_ok = pmc is not None
            pmc = pmc or {}
            out.update({
                "value_single_pass_query": round(imgs / elapsed_single, 2) if elapsed_single else None,
                "ms_per_step_single_pass_query": round(elapsed_single / args.steps * 1e3, 3) if elapsed_single else None,
                "knn": {"queries_per_sec": round(1e3 / (ms_knn_two or ms_knn), 2), "ms_per_query": round(ms_knn_two or ms_knn, 4),
                        "ms_per_query_in_the_pipeline": round(ms_knn_overlapped, 4),
                        "ms_per_query_single_pass": round(ms_knn, 4),
                        "mode": "single pass over the fp32 rows" if args.no_prefilter else
                                f"two-stage exact ({'byte' if args.prefilter == 2 else 'bf16'} mirror prefilter + fp32 re-evaluation)",
                        "two_stage_equal": two_stage_equal, "fell_back": bool(pref_fell_back),
                        "rows_searched_per_sec": round(world * len(table) / ((ms_knn_two or ms_knn) * 1e-3), 0), "dtype": "f32"},
                "roofline": {"bound": "mfma", "kernel": "ViT-L/14 forward (gemm_bf16_pp_kernel x 96 with the LayerNorms and residual adds in its epilogues + "
                                                        "attention, two half-chunk streams)",
                             "achieved": round(tf_exec, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                             "frac": round(tf_exec / PEAK_BF16_TFLOPS, 4),
                             "traffic": pmc.get("vit_hbm_bytes") if traffic_ok else None,
                             "traffic_source": "profiles/pmc_latest.json: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command "
                                               "(tools/round_profile.sh), NOT an observation of this run; fabric-side bytes incl. Infinity-Cache hits"
                                               + ("" if traffic_ok else f"; REFUSED: {pmc_refused}"),
                             "from_profile": {"note": "read from committed profiles, not observed by this run; each entry is refused (no numbers) "
                                                      "when its stamp does not match the kernel sources and batch of this run",
                                              "gemm_in_situ": gemm_in_situ(args.batch)},
                             "executed_gflop_per_image": round(executed / 1e9, 2),
                             "algorithmic_gflop_per_image": round(VIT_FLOP_PER_IMAGE / 1e9, 2),
                             "frac_on_algorithmic_flops": round(tf_alg / PEAK_BF16_TFLOPS, 4),
                             "note": "achieved/frac count the FLOPs this implementation EXECUTES (the last layer runs on the CLS rows only: "
                                     "3.5 % of the algorithmic 162.03 GFLOP/image are dead rows of the reference graph, output bit-identical); "
                                     "the algorithmic-count fraction is beside it"},
                "roofline_knn": {"bound": "hbm", "kernel": "knn_scan_kernel<12,WaveTopReg> (+2 merge launches), alone on the chip",
                                 "achieved": round(knn_gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                 "frac": round(knn_gbs / PEAK_HBM_GBS, 4),
                                 "traffic": pmc.get("knn_scan_hbm_bytes") if traffic_ok else None,
                                 "traffic_source": "profiles/pmc_latest.json (separate --pmc passes of this command, not this run)",
                                 "note": "the single-pass scan over the fp32 rows: algorithmic bytes = rows x 768 x 4"},
            })
            if ms_knn_two:
                row_bytes = 768 + 12 if args.prefilter == 2 else 768 * 2 + 4      # mirror row + its per-row floats
                two_bytes = len(table) * (row_bytes + 4 * 5 + (4 if args.prefilter == 2 else 0))  # + the coarse keys written once and read four times (+ the bound factors in the collect)
                out["roofline_knn"]["two_stage"] = {
                    "ms_per_query": round(ms_knn_two, 4), "bytes_read_and_written": two_bytes,
                    "GB_per_s_of_those_bytes": round(two_bytes / (ms_knn_two * 1e-3) / 1e9, 1),
                    "frac_of_hbm_peak_on_those_bytes": round(two_bytes / (ms_knn_two * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                    "speedup_over_single_pass": round(ms_knn / ms_knn_two, 3),
                    "rows_re_evaluated_last_query": pref_cand, "fell_back_to_single_pass": pref_fell_back,
                    "equal_to_single_pass": two_stage_equal,
                    "traffic_stage1": pmc.get("knn_two_stage_stage1_hbm_bytes") if traffic_ok and args.prefilter == 2 else None}
            if exchange_check is not None:
                out["exchange"] = exchange_check
                failed = failed or not (exchange_check["identical_on_every_rank"] and exchange_check["sorted"]
                                        and exchange_check["queries_merged"] == args.steps)
            if extra:
                out["other_configs"] = extra
            if world == 1 and not args.no_extra_configs:
                # the ONE-process form (mi_knn_sharded + mi_pipeline_create_sharded) over every GPU this process can see, as a
                # child with its own deadline; on a one-GPU box: two shards and two replicas on GPU 0
                out.setdefault("other_configs", {})["one_process_sharded"] = run_sharded_probe(args, wpath, ms_knn_two or ms_knn)
            if world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(weights, cfg)
            failed = failed or two_stage_equal is False
        print(json.dumps(out), flush=True)

    model.close()
    table.close()
    for pb in pins:
        pb.close()
    barrier()
    if rank == 0:
        try:
            os.unlink(wpath)
        except OSError:
            pass
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
