"""The weight loader in front of the towers (image_search_amd/csrc/weights.h), without a GPU: half-precision files from the
writers, the readers under the address and undefined-behaviour sanitizers over a deterministic corpus of broken files
(tests/cpp/test_weights_host.cpp, a stand-alone program), and the same hostile files through mi_weights_list."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from image_search_amd import synth
from image_search_amd.clip import list_weights

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_synthetic_mpk import write_mpk  # noqa: E402


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32) << 16).view(np.float32)


def _raw_safetensors(path):
    blob = open(path, "rb").read()
    n = int.from_bytes(blob[:8], "little")
    return json.loads(blob[8:8 + n]), blob[8 + n:]


# ---- the writers ------------------------------------------------------------------------------------------------------

# sha256 of what the writers produced for VitConfig.tiny(), seed 1, before they knew any dtype but F32
_F32_FILES = {
    "safetensors": "f67dfaef638dff10a41d7e18709f7f108154a445aa3243bab841875a81d02957",
    "": "87a2c0b5c168da027cf4bf49b4ad9bb85e9b09b90ad18c4afedb31eb1a5d4d63",
    "legacy": "e53309c8dd2aacd32b54f61c6c9a4cfe6e01519303b425447846d3086ac2c5e0",
    "decomposed_ln": "c017c1b2c924a264d53b9ec6caeb0699095b581194704614d4d76b6574b20e8b",
    "decomposed_ln uncoalesced": "321aee88e3c2caaae0adada9d28d365bf683fd22976e982e0b3c53f2e322ea1e",
    "decomposed_ln legacy": "2dcc7e394f07534caccac6d5718d316558370f7c375e1c0fe575547f0247cebf",
}


def test_default_writers_keep_their_bytes(tmp_path):
    """dtype="F32", given or left out, is what the goldens and every older test were written with: the same bytes as before."""
    import hashlib
    cfg = synth.VitConfig.tiny()
    w = synth.vit_weights(cfg, 1)
    p = str(tmp_path / "w.bin")

    def digest():
        return hashlib.sha256(open(p, "rb").read()).hexdigest()

    for extra in ({}, {"dtype": "F32"}):
        synth.save_safetensors(w, p, {"num_attention_heads": cfg.heads}, **extra)
        assert digest() == _F32_FILES["safetensors"]
        for key in list(_F32_FILES)[1:]:
            words = key.split()
            write_mpk(w, cfg, p, legacy="legacy" in words, decomposed_ln="decomposed_ln" in words, coalesced="uncoalesced" not in words, **extra)
            assert digest() == _F32_FILES[key], key


@pytest.mark.parametrize("dtype", ["F16", "BF16"])
def test_half_precision_safetensors_writer_roundtrip(tmp_path, dtype):
    """The F16 file read back by the safetensors package holds numpy's float16 rounding of every tensor; the BF16 file (numpy
    has no such type, so its bytes are read here) the round-to-nearest-even upper halves; dtype strings and offsets fit."""
    cfg = synth.VitConfig.tiny()
    w = synth.vit_weights(cfg, 1)
    w["vision_model.pre_layrnorm.bias"] = np.array([0.0, -0.0, 1e-8, -6e-8, 65504.0, 65519.9, 1e-40, 3.3e38] + [1.0] * 120, np.float32)
    p = str(tmp_path / "w.safetensors")
    synth.save_safetensors(w, p, {"num_attention_heads": cfg.heads}, dtype=dtype)
    header, data = _raw_safetensors(p)
    assert header.pop("__metadata__") == {"num_attention_heads": str(cfg.heads)}
    assert list(header) == list(w)
    end = 0
    for name, a in w.items():
        h = header[name]
        assert h["dtype"] == dtype and h["shape"] == list(a.shape) and h["data_offsets"] == [end, end + 2 * a.size], name
        end += 2 * a.size
        raw = np.frombuffer(data[h["data_offsets"][0]:h["data_offsets"][1]], "<u2")
        if dtype == "BF16":
            assert np.array_equal(raw, (bf16_round(a).view(np.uint32) >> 16).astype(np.uint16).reshape(-1)), name
            assert np.array_equal(synth.round_to(a, dtype).view(np.uint32), bf16_round(a).view(np.uint32)), name
        else:
            with np.errstate(over="ignore"):
                assert np.array_equal(raw, a.astype(np.float16).view(np.uint16).reshape(-1)), name
    assert end == len(data)
    if dtype == "F16":
        from safetensors.numpy import load_file
        back = load_file(p)
        assert set(back) == set(w)
        with np.errstate(over="ignore"):
            assert all(back[k].dtype == np.float16 and np.array_equal(back[k].view(np.uint16), w[k].astype(np.float16).view(np.uint16)) for k in w)
            assert all(np.array_equal(back[k].astype(np.float32).view(np.uint32), synth.round_to(w[k], "F16").view(np.uint32)) for k in w)
    # the rounding really moved the values, and a second rounding moves nothing
    r = synth.round_to(w["visual_projection.weight"], dtype)
    assert not np.array_equal(r, w["visual_projection.weight"]) and np.array_equal(synth.round_to(r, dtype), r)
    with pytest.raises(KeyError):
        synth.save_safetensors(w, p, dtype="F64")


@pytest.mark.parametrize("dtype", ["F16", "BF16"])
def test_weights_list_prints_the_file_dtype(mi, tmp_path, dtype):
    """mi_weights_list on half-precision files: the dtype column is the file's, names and shapes are those of the F32 file —
    for safetensors and for the three inventories of a Burn record (whose Linear weights come back [out, in])."""
    cfg = synth.VitConfig.tiny()
    w = synth.vit_weights(cfg, 1)
    f32, p = str(tmp_path / "f32.safetensors"), str(tmp_path / "half.safetensors")
    synth.save_safetensors(w, f32, {"num_attention_heads": cfg.heads})
    synth.save_safetensors(w, p, {"num_attention_heads": cfg.heads}, dtype=dtype)
    want = list_weights(f32)
    assert [(n, s) for n, _, s in want] == [(n, tuple(a.shape)) for n, a in w.items()] and {d for _, d, _ in want} == {"F32"}
    got = list_weights(p)
    assert got == [(n, dtype, s) for n, _, s in want]
    mpk = str(tmp_path / "vision_model.mpk")
    for kw in ({}, {"decomposed_ln": True}, {"decomposed_ln": True, "coalesced": False}):
        write_mpk(w, cfg, mpk, dtype=dtype, **kw)
        got = [t for t in list_weights(mpk) if not t[0].startswith("(set aside)")]
        assert sorted(got) == sorted((n, dtype, s) for n, _, s in want), kw
    write_mpk(w, cfg, mpk, dtype=dtype, legacy=True)      # lists of numbers: no dtype in the file, fp32 values
    assert sorted(list_weights(mpk)) == sorted(want)


# ---- the readers under the sanitizers ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/cpp/test_weights_host.cpp built with the sanitizers and run once, as a child; its scratch directory keeps the
    hostile files it wrote out by name and the list of what each must end in."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    work = tmp_path_factory.mktemp("weights_host")
    exe = str(work / "test_weights_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_weights_host.cpp"), "-o", exe])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = ":".join(filter(None, [env.get("ASAN_OPTIONS"), "max_allocation_size_mb=64"]))
    out = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=120, env=env)
    return work, out


def test_readers_under_the_sanitizers(program):
    """All 65 536 half and bfloat16 patterns, valid files of both formats value by value, every truncation, single-byte
    corruption of the structure and the hostile cases: read, or refused with MI_ERR_IO / MI_ERR_UNSUPPORTED — no other
    exception, no sanitizer report, no allocation above 64 MB for files of a few KB, under a second each."""
    _, out = program
    print(out.stdout[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-4000:] + out.stderr[-4000:]


_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from image_search_amd import _lib
mi = _lib.lib()
need = ctypes.c_size_t()
for line in open(sys.argv[2] + "/hostile.txt"):
    name, want = line.split()
    rc = mi.mi_weights_list((sys.argv[2] + "/" + name).encode(), None, 0, ctypes.byref(need))
    print(json.dumps([name, want, rc, mi.mi_last_error().decode(errors="replace") if rc else ""]), flush=True)
print("done")
"""


def test_hostile_files_through_the_library(built, program):
    """The hand-written hostile files through mi_weights_list, in a child interpreter (a crash is a failed assertion here, not
    a dead test run): nothing unwinds across the ABI — MI_ERR_IO (-2) or MI_ERR_UNSUPPORTED (-5) with a message, or, where
    the program's list says the file is fine, MI_OK."""
    work, ran = program
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-2000:]
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(work)], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines and lines[-1] == "done", out.stdout[-2000:] + out.stderr[-2000:]
    seen = [json.loads(l) for l in lines[:-1]]
    assert len(seen) >= 60 and len(seen) == sum(1 for _ in open(str(work / "hostile.txt")))
    for name, want, rc, msg in seen:
        if want == "refuse":
            assert rc in (-2, -5) and msg, (name, rc, msg)
        elif want == "accept":
            assert rc == 0, (name, rc, msg)
        else:
            assert rc == 0 or (rc in (-2, -5) and msg), (name, rc, msg)
    assert sum(1 for _, want, _, _ in seen if want == "refuse") >= 45
