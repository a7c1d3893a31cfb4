"""MI_PRECISION_BF16X3 against the fp32 and bf16 image towers, ViT-L/14, one process.

  python tools/x3_profile.py [--n 256] [--reps 20] [--out profiles/x3_profile.json]
      loads the tower in F32, BF16X3 and BF16 from one seeded checkpoint, warms all three up, then alternates them
      (F32, BF16X3, BF16, F32, ...) for --reps rounds on resident inputs, each forward timed by device events; reports ms,
      images/s, the three-pass GEMMs' executed TFLOP/s over the whole forward (3x the algorithmic FLOPs of the encoder
      linears: a lower bound on the GEMMs' own rate) and max|BF16X3 - F32| / rms(F32)
  rocprofv3 --kernel-trace --stats -d D -o x --output-format csv -- python3 tools/x3_profile.py --only 3 --reps 5
      the workload for per-kernel times (BF16X3 forwards only: warm-up + --reps)
  python tools/x3_profile.py --stats D/.../x_kernel_stats.csv --forwards 7 [--out profiles/x3_kernels.txt]
      that run's kernel stats per forward, with the GEMM kinds' executed TFLOP/s
"""
import argparse
import csv
import json
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

NAMES = {0: "F32", 3: "BF16X3", 1: "BF16"}


def gemm_flops(cfg, n):
    """Algorithmic FLOPs of the encoder linears as the tower runs them: layers 0 .. L-2 on every token row, the last
    layer's K | V on every row and its q, out_proj, fc1, fc2 on the CLS rows only."""
    S, D, FF, L = cfg.tokens, cfg.hidden, cfg.ff, cfg.layers
    full = 2 * S * D * (3 * D + D + 2 * FF)
    last = 2 * S * D * 2 * D + 2 * D * (D + D + 2 * FF)
    return n * ((L - 1) * full + last)


def stats_table(path, forwards, out):
    from image_search_amd import synth
    cfg = synth.VitConfig.vit_l14()
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    lines = [f"kernel stats of {forwards} BF16X3 forwards (ViT-L/14, b = 256), per forward ({os.path.basename(path)})",
             "sums of kernel durations: with two half-chunk streams (option parts = 2) kernels overlap and the sum exceeds the",
             "forward's time; MI_CLIP_PARTS=1 gives each kernel the device alone", ""]
    lines.append(f"{'ms/fwd':>8} {'share':>6} {'calls/fwd':>9}  kernel")
    x3_ns = 0.0
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns = float(r["TotalDurationNs"])
        name = r["Name"]
        short = re.sub(r"\(.*\)$", "", name).replace("void ", "").replace("unsigned short", "u16")
        if re.search(r"gemm_bf16_pp_kernel<\d+, unsigned short, (true|false), true>", name):
            x3_ns += ns
        lines.append(f"{ns / forwards / 1e6:8.2f} {ns / total:6.1%} {int(r['Calls']) / forwards:9.1f}  {short}")
    lines.append("")
    lines.append(f"all kernels: {total / forwards / 1e6:.2f} ms per forward")
    if x3_ns:
        f = 3 * gemm_flops(cfg, 256)
        lines.append(f"three-pass GEMMs: {x3_ns / forwards / 1e6:.2f} ms per forward = {f / (x3_ns / forwards * 1e-9) / 1e12:.0f} "
                     f"TFLOP/s executed (3 x {gemm_flops(cfg, 256) / 1e12:.2f} TFLOP per forward)")
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", type=int, default=None, help="one precision only (the rocprofv3 workload)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None, help="summarise a rocprofv3 kernel-stats CSV instead")
    ap.add_argument("--forwards", type=int, default=0)
    ap.add_argument("--parts", type=int, default=None, help="option parts of every handle (default: the library's, 2)")
    a = ap.parse_args()
    if a.stats:
        stats_table(a.stats, a.forwards, a.out)
        return

    import torch
    from image_search_amd import synth
    from image_search_amd.clip import Model

    cfg = synth.VitConfig.vit_l14()
    path = os.path.join(tempfile.gettempdir(), f"x3_profile_{os.getpid()}.safetensors")
    synth.save_safetensors(synth.vit_weights(cfg, 0), path, {"num_attention_heads": cfg.heads})
    precs = [a.only] if a.only is not None else [0, 3, 1]
    models = {}
    try:
        for p in precs:
            t0 = time.time()
            models[p] = Model.from_file(path, 0, p)
            if a.parts is not None:
                models[p].set_option("parts", a.parts)
            print(f"{NAMES[p]}: loaded in {time.time() - t0:.1f} s", flush=True)
    finally:
        os.unlink(path)
    n = a.n
    px = synth.preprocess_rgb8(synth.images_u8(100, n, cfg.image))
    d_in = torch.from_numpy(px).cuda()
    outs = {p: torch.empty((n, cfg.proj), dtype=torch.float32, device="cuda") for p in precs}
    st = torch.cuda.Stream()
    for p in precs:   # warm-up: workspaces, function attributes, clocks
        for _ in range(2):
            models[p].forward_device(d_in.data_ptr(), n, outs[p].data_ptr(), st.cuda_stream)
    st.synchronize()
    ev = {p: [] for p in precs}
    for _ in range(a.reps):
        for p in precs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            models[p].forward_device(d_in.data_ptr(), n, outs[p].data_ptr(), st.cuda_stream)
            e1.record(st)
            ev[p].append((e0, e1))
    st.synchronize()
    res = {"model": "ViT-L/14 (24 layers, hidden 1024, ff 4096, 257 tokens), seeded weights", "batch": n, "reps": a.reps,
           "parts": a.parts if a.parts is not None else "library default (2)",
           "order": [NAMES[p] for p in precs], "device": torch.cuda.get_device_name(0), "precisions": {}}
    for p in precs:
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev[p]])
        res["precisions"][NAMES[p]] = {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(ms.min()), 3),
                                       "ms_max": round(float(ms.max()), 3), "images_per_s": round(n / float(np.median(ms)) * 1e3, 1)}
    if 3 in precs:
        ms = res["precisions"]["BF16X3"]["ms_median"]
        res["precisions"]["BF16X3"]["gemm_tflops_executed_over_forward"] = round(3 * gemm_flops(cfg, n) / (ms * 1e-3) / 1e12, 1)
    if 0 in precs and 3 in precs:
        ref = outs[0].cpu().numpy().astype(np.float64)
        rms = float(np.sqrt((ref ** 2).mean()))
        for p in precs:
            if p == 0:
                continue
            err = float(np.abs(outs[p].cpu().numpy() - ref).max() / rms)
            res["precisions"][NAMES[p]]["max_err_vs_f32_over_rms"] = float(f"{err:.3g}")
        res["x3_time_over_f32"] = round(res["precisions"]["BF16X3"]["ms_median"] / res["precisions"]["F32"]["ms_median"], 4)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    for m in models.values():
        m.close()


if __name__ == "__main__":
    main()
