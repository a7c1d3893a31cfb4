"""Builds libmi355clip.so (the C-ABI library, include/mi355clip.h) for gfx950 in-tree.

hipcc cross-compiles without a GPU, so this runs in the build container; the
resulting .so travels to the GPU box with the repo snapshot (it is git-ignored,
not gpurun-ignored).
"""
from __future__ import annotations

import os
import shutil
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libmi355clip.so")
SOURCES = ["core.hip", "knn.hip", "vit.hip", "preprocess.hip", "pipeline.hip", "sharded.hip", "sharded_calls.hip", "index.hip", "join.hip", "assign.hip",
           "assign_multi.hip", "search_many.hip", "kmeans_seed.hip", "diverse.hip", "compound.hip", "page.hip",
           "grouped.hip", "where.hip", "ordered.hip", "density.hip", "join_between.hip", "summary.hip", "density_sharded.hip",
           "kmeans_sharded.hip", "summary_sharded.hip", "density_levels.hip", "kmeans_seed_sharded.hip",
           "representatives.hip", "window.hip", "compact.hip"]
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off",
         "-Wall", "-Wno-unused-function", "-Wno-unused-const-variable"]


def _hipcc() -> str:
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_lib(force: bool = False, verbose: bool = False) -> str:
    srcs = [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(PKG), "include", "mi355clip.h"))
    if not force and not _stale(LIB, srcs + headers):
        return LIB   # a library newer than every source needs no object files (they do not travel with a copied tree)
    objs = []
    for s in srcs:
        o = s[:-4] + ".o"
        if force or _stale(o, [s] + headers):
            cmd = [_hipcc()] + FLAGS + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
        objs.append(o)
    if force or _stale(LIB, objs):
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-ldl", "-o", LIB]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build_lib(verbose=True))
