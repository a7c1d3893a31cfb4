"""Half-precision checkpoint files through the towers on a real MI355X, and the geometries refused at load.

For a file dtype T in {F16, BF16}: `wr` are the synthetic weights rounded to T, file A holds `wr` as F32 and file B holds them
as T — the same real numbers.  The towers must give the same bits from either file (the conversion in the loader is exact),
and file B at MI_PRECISION_F32 must meet the numpy oracle on `wr` at the fp32 tower's own bar, 1e-4 (tests/test_vit_gpu.py):
that keeps the first check from passing when both files are misread the same way."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from image_search_amd import synth
from image_search_amd._lib import lib
from image_search_amd.clip import PRECISION_BF16, PRECISION_BF16X3, PRECISION_F32, Model, TextModel
from oracle import vit_numpy

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_synthetic_mpk import write_mpk  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = ["F16", "BF16"]
GEOMETRIES = {
    "tiny": synth.VitConfig.tiny(),                                                                  # D 128, L 2, S 17, proj 64
    "d256": synth.VitConfig(hidden=256, layers=4, heads=4, ff=1024, patch=14, image=56, proj=64),    # ln_fold and BF16X3 apply
}


def close(out, ref, tol):
    rms = float(np.sqrt((np.asarray(ref, np.float64) ** 2).mean()))
    return np.allclose(out, ref, rtol=tol, atol=tol * rms), float(np.abs(out - ref).max() / rms)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def vision(built, tmp_path_factory):
    """(cfg, wr, file A, file B, pixels, fp32 oracle on wr) per (geometry, dtype), made once"""
    out = {}
    d = tmp_path_factory.mktemp("vision")
    for geom, cfg in GEOMETRIES.items():
        w = synth.vit_weights(cfg, 5)
        px = synth.preprocess_rgb8(synth.images_u8(77, 3, cfg.image))
        for dtype in DTYPES:
            wr = {k: synth.round_to(v, dtype) for k, v in w.items()}
            assert any(not np.array_equal(wr[k], w[k]) for k in w)
            a, b = str(d / f"{geom}_{dtype}_as_f32.safetensors"), str(d / f"{geom}_{dtype}.safetensors")
            synth.save_safetensors(wr, a, {"num_attention_heads": cfg.heads})
            synth.save_safetensors(wr, b, {"num_attention_heads": cfg.heads}, dtype=dtype)
            assert os.path.getsize(b) < 0.51 * os.path.getsize(a)
            out[geom, dtype] = (cfg, wr, a, b, px, vit_numpy.vit_forward(wr, cfg, px, np.float32))
    return out


def _forward(path, precision, px, ln_fold=None):
    m = Model.from_file(path, 0, precision)
    if ln_fold is not None:
        m.set_option("ln_fold", ln_fold)
    out = m.forward(px)
    m.close()
    return out


# tiny (D 128) has no LayerNorm-free loop ("ln_fold" needs D % 256 == 0) and no BF16X3: its bf16 tower is the LayerNorm one
MODES = [("tiny", PRECISION_F32, None), ("tiny", PRECISION_BF16, None),
         ("d256", PRECISION_F32, None), ("d256", PRECISION_BF16, 1), ("d256", PRECISION_BF16, 0), ("d256", PRECISION_BF16X3, None)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom,precision,ln_fold", MODES, ids=["tiny-f32", "tiny-bf16", "d256-f32", "d256-bf16-fold", "d256-bf16-ln", "d256-bf16x3"])
def test_same_numbers_same_bits(vision, dtype, geom, precision, ln_fold):
    cfg, wr, a, b, px, ref = vision[geom, dtype]
    out_a, out_b = _forward(a, precision, px, ln_fold), _forward(b, precision, px, ln_fold)
    assert np.isfinite(out_a).all() and out_a.shape == (3, cfg.proj)
    assert same_bits(out_a, out_b), float(np.abs(out_a - out_b).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_and_the_right_numbers(vision, dtype, geom):
    cfg, wr, a, b, px, ref = vision[geom, dtype]
    ok, err = close(_forward(b, PRECISION_F32, px), ref, 1e-4)
    print(f"{geom} {dtype}: max|err|/rms = {err:.2e}")
    assert ok, err


@pytest.mark.parametrize("dtype", DTYPES)
def test_text_tower(built, tmp_path, dtype):
    cfg = synth.TextConfig.tiny()
    w = synth.vit_weights(cfg, 6)
    wr = {k: synth.round_to(v, dtype) for k, v in w.items()}
    a, b = str(tmp_path / "as_f32.safetensors"), str(tmp_path / "half.safetensors")
    synth.save_safetensors(wr, a, {"num_attention_heads": cfg.heads})
    synth.save_safetensors(wr, b, {"num_attention_heads": cfg.heads}, dtype=dtype)
    ids = synth.token_ids(cfg, 9, 3)
    for precision in (PRECISION_F32, PRECISION_BF16):
        outs = []
        for path in (a, b):
            m = TextModel.from_file(path, 0, precision)
            outs.append(m.embed(ids))
            m.close()
        assert np.isfinite(outs[0]).all() and same_bits(outs[0], outs[1]), precision
        if precision == PRECISION_F32:
            ok, err = close(outs[1], vit_numpy.text_forward(wr, cfg, ids, np.float32), 1e-4)
            print(f"text {dtype}: max|err|/rms = {err:.2e}")
            assert ok, err


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inventory", [{}, {"decomposed_ln": True}], ids=["fused-ln", "decomposed-ln"])
def test_burn_records(vision, tmp_path, dtype, inventory):
    cfg, wr, _, st, px, ref = vision["tiny", dtype]
    a, b = str(tmp_path / "as_f32.mpk"), str(tmp_path / "half.mpk")
    write_mpk(wr, cfg, a, **inventory)
    write_mpk(wr, cfg, b, dtype=dtype, **inventory)
    assert os.path.getsize(b) < 0.55 * os.path.getsize(a)
    for precision in (PRECISION_F32, PRECISION_BF16):
        out_a, out_b = _forward(a, precision, px), _forward(b, precision, px)
        assert np.isfinite(out_a).all() and same_bits(out_a, out_b), precision
        assert same_bits(out_b, _forward(st, precision, px)), precision        # and the safetensors file of the same dtype
        if precision == PRECISION_F32:
            ok, err = close(out_b, ref, 1e-4)
            assert ok, err


# ---- what cannot run is refused at load ---------------------------------------------------------------------------------

def _vision_cases():
    """name -> (weights, metadata, allowed codes): LOADS only — no forward ever runs at a geometry the library does not claim"""
    tiny = synth.VitConfig.tiny()
    D = tiny.hidden
    base = synth.vit_weights(tiny, 2)
    v = "vision_model."

    def of(cfg):
        return synth.vit_weights(cfg, 2), {"num_attention_heads": cfg.heads}, (-5,)

    def edited(name, tensor):
        return {**base, v + name: tensor}, {"num_attention_heads": tiny.heads}, (-5,)

    def without(name):
        w = dict(base)
        del w[v + name]
        return w, {"num_attention_heads": tiny.heads}, (-2, -5)

    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    cases = {
        "hidden 640, 10 heads": of(synth.VitConfig(hidden=640, layers=1, heads=10, ff=256, patch=14, image=28, proj=64)),
        "hidden 192": of(synth.VitConfig(hidden=192, layers=1, heads=3, ff=256, patch=14, image=28, proj=64)),
        "hidden 896, 14 heads": of(synth.VitConfig(hidden=896, layers=1, heads=14, ff=128, patch=2, image=4, proj=8)),
        "ff 200": of(synth.VitConfig(hidden=128, layers=2, heads=2, ff=200, patch=14, image=56, proj=64)),
        # ViT-H/14's attention: 1280 is a width the LayerNorms are built for, but its 16 heads are 80 wide
        "hidden 1280, 16 heads": of(synth.VitConfig(hidden=1280, layers=1, heads=16, ff=128, patch=2, image=4, proj=8)),
        "11 positions": edited("embeddings.position_embedding.weight", z(11, D)),     # not G * G + 1 (10 is: a 3 x 3 grid)
        "1 position": edited("embeddings.position_embedding.weight", z(1, D)),
        "patch 14 x 16": edited("embeddings.patch_embedding.weight", z(D, 3, 14, 16)),
        "positions [S, D + 1]": edited("embeddings.position_embedding.weight", z(tiny.tokens, D + 1)),
        "layer 1 without fc2.bias": without("encoder.layers.1.mlp.fc2.bias"),
        "layer 1 without layer_norm1.weight": without("encoder.layers.1.layer_norm1.weight"),
        "layer 1 without q_proj.weight": without("encoder.layers.1.self_attn.q_proj.weight"),
    }
    for heads in ("0", "-2", "abc"):
        cases[f"num_attention_heads {heads!r}"] = (dict(base), {"num_attention_heads": heads}, (-5,))
    return cases


def _refused(load, path, precision, codes, name):
    h = ctypes.c_void_p(0xdead)
    rc = load(path.encode(), 0, precision, ctypes.byref(h))
    msg = lib().mi_last_error().decode()
    assert rc in codes and not h.value and len(msg) > 10, (name, precision, rc, msg)
    return msg


def test_what_cannot_run_is_refused_at_load(vision, tmp_path):
    cfg, wr, a, b, px, ref = vision["tiny", "F16"]
    before = {p: _forward(b, p, px) for p in (PRECISION_F32, PRECISION_BF16)}
    path = str(tmp_path / "case.safetensors")
    for name, (w, meta, codes) in _vision_cases().items():
        synth.save_safetensors(w, path, meta, dtype="F16")
        for precision in (PRECISION_F32, PRECISION_BF16):
            msg = _refused(lib().mi_clip_load, path, precision, codes, name)
        if name.startswith("hidden 640"):
            assert "640" in msg and "LayerNorm" in msg, msg
        if name.startswith("hidden 1280"):
            assert "1280" in msg and "16 heads" in msg and "head_dim 64" in msg, msg
    # 10 positions are the class token and a 3 x 3 grid: a geometry the library runs, so it loads (42 x 42 pixels)
    synth.save_safetensors({**wr, "vision_model.embeddings.position_embedding.weight": np.zeros((10, cfg.hidden), np.float32)}, path,
                           {"num_attention_heads": cfg.heads}, dtype="F16")
    m = Model.from_file(path, 0, PRECISION_F32)
    assert (m.tokens, m.image, m.hidden) == (10, 42, cfg.hidden)
    m.close()
    # more tokens than the bf16 attention kernels hold: refused for bf16 where the first forward used to fail
    big = synth.VitConfig(hidden=128, layers=1, heads=2, ff=128, patch=2, image=36, proj=8)     # 18 x 18 + 1 = 325 tokens
    synth.save_safetensors(synth.vit_weights(big, 2), path, {"num_attention_heads": 2})
    assert "288" in _refused(lib().mi_clip_load, path, PRECISION_BF16, (-5,), "325 tokens")

    # the text tower behind the same door
    tcfg = synth.TextConfig.tiny()
    tw = synth.vit_weights(tcfg, 2)
    t = "text_model."
    wide = synth.TextConfig(hidden=640, layers=1, heads=10, ff=256, vocab=50, positions=8, proj=8)
    text_cases = {
        "hidden 640, 10 heads": (synth.vit_weights(wide, 2), {"num_attention_heads": 10}, (-5,)),
        "ff 200": (synth.vit_weights(synth.TextConfig(hidden=128, layers=1, heads=2, ff=200, vocab=50, positions=8, proj=8), 2), {"num_attention_heads": 2}, (-5,)),
        "positions [S, D + 1]": ({**tw, t + "embeddings.position_embedding.weight": np.zeros((tcfg.positions, tcfg.hidden + 1), np.float32)},
                                 {"num_attention_heads": tcfg.heads}, (-5,)),
        "layer 1 without fc1.bias": ({k: x for k, x in tw.items() if k != t + "encoder.layers.1.mlp.fc1.bias"}, {"num_attention_heads": tcfg.heads}, (-2, -5)),
        "layer 1 without layer_norm1.weight": ({k: x for k, x in tw.items() if k != t + "encoder.layers.1.layer_norm1.weight"},
                                               {"num_attention_heads": tcfg.heads}, (-2, -5)),
    }
    for heads in ("0", "-2", "abc"):
        text_cases[f"num_attention_heads {heads!r}"] = (tw, {"num_attention_heads": heads}, (-5,))
    for name, (w, meta, codes) in text_cases.items():
        synth.save_safetensors(w, path, meta, dtype="BF16")
        for precision in (PRECISION_F32, PRECISION_BF16):
            _refused(lib().mi_clip_load_text, path, precision, codes, "text: " + name)
    long_text = synth.TextConfig(hidden=128, layers=1, heads=2, ff=128, vocab=50, positions=300, proj=8)
    synth.save_safetensors(synth.vit_weights(long_text, 2), path, {"num_attention_heads": 2})
    assert "288" in _refused(lib().mi_clip_load_text, path, PRECISION_BF16, (-5,), "text: 300 positions")

    # a valid load and forward afterwards: the bits of before
    for p, want in before.items():
        assert same_bits(_forward(b, p, px), want), p
