"""MI_PRECISION_BF16X3 on a real MI355X: the image tower within 1e-4 on bf16 MFMA.

Every encoder GEMM runs as three bf16 MFMA passes over hi | lo halves of both operands (x_hi w_hi + x_lo w_hi + x_hi w_lo,
one fp32 accumulator) in the persistent 256x256 kernel; attention and the residual stream stay fp32.
  op level   : the three epilogues (fp32 q|k|v, hi | lo fc1 output, fp32 residual add in place) against fp64, exact where
               the operands are exact sums hi + lo, over grids, tile orders and the split last round
  model level: the L/14 golden and a small qualifying tower within 1e-4 (the tolerance of tests/test_vit_gpu.py's fp32 path)
  batch 256  : against the fp32 path within 1e-4, outlier channels included
  same bits  : chunking, the CLS-only last layer, the two-stream split, the fused pipeline
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from image_search_amd import ops, synth
from image_search_amd._lib import c_vp, lib
from image_search_amd.clip import PRECISION_BF16X3, PRECISION_F32, Model
from image_search_amd.search import EmbeddingTable, Pipeline
from oracle import vit_numpy

pytestmark = pytest.mark.gpu

X3 = PRECISION_BF16X3


def close(out, ref, tol):
    rms = float(np.sqrt((np.asarray(ref, np.float64) ** 2).mean()))
    return np.allclose(out, ref, rtol=tol, atol=tol * rms), float(np.abs(out - ref).max() / rms)


def gelu(a):
    return a / (1 + np.exp(-1.702 * a))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def save(tmp_path_factory, cfg, w, name):
    path = str(tmp_path_factory.mktemp("w") / name)
    synth.save_safetensors(w, path, {"num_attention_heads": cfg.heads})
    return path


@pytest.fixture(scope="module")
def l14(built, tmp_path_factory):
    cfg = synth.VitConfig.vit_l14()
    g = np.load(os.path.join(GOLDEN, "vit_l14.npz"))
    w = synth.vit_weights(cfg, int(g["seed"]))
    return cfg, w, save(tmp_path_factory, cfg, w, "l14.safetensors"), g


# ---- op level ------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(300, 3072, 1024), (257, 1024, 4096), (1000, 4096, 1024), (64, 1024, 1024)])
def test_x3_linear_epilogues_against_fp64(built, shape):
    """The three epilogues at the tower's shapes: q|k|v (fp32 out), fc1 (quick_gelu, hi | lo out), out_proj / fc2 (x += ...)."""
    m, n, k = shape
    rng = np.random.default_rng(31)
    x = rng.standard_normal((m, k)).astype(np.float32)
    w = (rng.standard_normal((n, k)) * k ** -0.5).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    res = rng.standard_normal((m, n)).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64).T + b
    scale = float(np.abs(ref).max())
    assert np.abs(ops.linear(x, w, b, ops.EPI_BIAS, X3) - ref).max() <= 3e-5 * scale
    assert np.abs(ops.linear(x, w, b, ops.EPI_BIAS_QGELU, X3) - gelu(ref)).max() <= 3e-5 * scale
    assert np.abs(ops.linear(x, w, b, ops.EPI_BIAS_RESID, X3, out=res) - (ref + res)).max() <= 3e-5 * scale
    # plain bf16 on the same data is ~1e-2 off: the bar above is one bf16 cannot meet
    assert np.abs(ops.linear(x, w, b, ops.EPI_BIAS, 1) - ref).max() > 3e-4 * scale


def test_x3_linear_exact_where_the_split_is_exact(built):
    """Integers (lo = 0) give the exact product; so do operands that are an exact hi + lo pair against integers — the
    lo plane of X in pass 2 and of W in pass 3 must be read from the right place."""
    rng = np.random.default_rng(5)
    m, n, k = 700, 512, 320
    xi = rng.integers(-3, 4, (m, k)).astype(np.float32)
    wi = rng.integers(-2, 3, (n, k)).astype(np.float32)
    b = rng.integers(-5, 6, n).astype(np.float32)
    assert np.array_equal(ops.linear(xi, wi, b, ops.EPI_BIAS, X3), xi @ wi.T + b)
    xf = (xi + rng.integers(-3, 4, (m, k)) / 512).astype(np.float32)    # 1 + 3/512 needs 10 significant bits: lo != 0
    wf = (wi + rng.integers(-3, 4, (n, k)) / 512).astype(np.float32)
    for xx, ww in ((xf, wi), (xi, wf)):
        ref = xx.astype(np.float64) @ ww.astype(np.float64).T + b
        assert np.array_equal(ops.linear(xx, ww, b, ops.EPI_BIAS, X3), ref.astype(np.float32))
        res = rng.integers(-8, 9, (m, n)).astype(np.float32)
        assert np.array_equal(ops.linear(xx, ww, b, ops.EPI_BIAS_RESID, X3, out=res), (ref + res).astype(np.float32))


@pytest.mark.parametrize("order", [0, 4])
def test_x3_persistent_gemm_random_shapes_grids_and_split_tail(built, monkeypatch, order):
    """Seeded sweep over (rows, N, K, workgroup count, split last round, tile order), every epilogue, exact on operands
    whose split is exact (see above): several tiles per workgroup, the counted store/load queue across tile boundaries
    and the quadrant tasks of a short last round."""
    rng = np.random.default_rng(2027 + order)
    monkeypatch.setenv("MI_OP_GEMM_ORDER", str(order))
    for case in range(16):
        grid = int(rng.choice([1, 2, 3, 5, 8, 13, 32, 256]))
        split = int(rng.integers(0, 2))
        m = int(rng.integers(1, 7)) * 256 - int(rng.integers(0, 200))
        n = int(rng.choice([256, 512, 1024, 2048] if order == 4 else [256, 512, 768]))
        k = int(rng.integers(2, 10)) * 64
        monkeypatch.setenv("MI_OP_GRID", str(grid))
        monkeypatch.setenv("MI_GEMM_SPLIT", str(split))
        x = rng.integers(-2, 3, (m, k)).astype(np.float32)
        w = rng.integers(-1, 2, (n, k)).astype(np.float32)
        if case % 2:   # the lo plane of W (pass 3) carries bits
            w = (w + rng.integers(-3, 4, (n, k)) / 512).astype(np.float32)
        else:          # ... of X (pass 2)
            x = (x + rng.integers(-3, 4, (m, k)) / 512).astype(np.float32)
        b = rng.integers(-3, 4, n).astype(np.float32)
        ref = x.astype(np.float64) @ w.astype(np.float64).T + b
        tag = (case, grid, split, m, n, k)
        assert np.array_equal(ops.linear(x, w, b, ops.EPI_BIAS, X3), ref.astype(np.float32)), tag
        res = rng.integers(-4, 5, (m, n)).astype(np.float32)
        assert np.array_equal(ops.linear(x, w, b, ops.EPI_BIAS_RESID, X3, out=res), (ref + res).astype(np.float32)), tag
        g = gelu(ref)
        assert np.abs(ops.linear(x, w, b, ops.EPI_BIAS_QGELU, X3) - g).max() <= 2e-5 * max(1.0, float(np.abs(g).max())), tag


def test_x3_linear_shape_rule(built):
    x = np.ones((64, 128), np.float32)
    with pytest.raises(Exception):
        ops.linear(x, np.ones((384, 128), np.float32), np.zeros(384, np.float32), ops.EPI_BIAS, X3)   # n % 256
    with pytest.raises(Exception):
        ops.linear(np.ones((64, 64), np.float32), np.ones((256, 64), np.float32), np.zeros(256, np.float32), ops.EPI_BIAS, X3)  # k < 128
    with pytest.raises(Exception):
        ops.linear(x, np.ones((256, 128), np.float32), None, ops.EPI_STORE_F32, X3)


# ---- model level ---------------------------------------------------------------------

def test_l14_x3_matches_the_golden_within_1e4(l14):
    cfg, w, path, g = l14
    px = synth.preprocess_rgb8(synth.images_u8(int(g["image_seed"]), int(g["n_img"]), cfg.image))
    m = Model.from_file(path, 0, X3)
    out = m.forward(px)
    m.close()
    ok, err = close(out, g["embeds_hf_f32"], 1e-4)
    assert ok, err
    ok, err = close(out, g["embeds_f64"], 1e-4)
    assert ok, err


def test_small_qualifying_tower_against_the_fp64_oracle(built, tmp_path_factory):
    cfg = synth.VitConfig(hidden=256, layers=2, heads=4, ff=1024, patch=14, image=56, proj=64)
    w = synth.vit_weights(cfg, 11)
    path = save(tmp_path_factory, cfg, w, "small.safetensors")
    px = synth.preprocess_rgb8(synth.images_u8(12, 5, cfg.image))
    m = Model.from_file(path, 0, X3)
    out = m.forward(px)
    m.close()
    ok, err = close(out, vit_numpy.vit_forward(w, cfg, px, np.float64), 1e-4)
    assert ok, err


@pytest.mark.parametrize("variant", ["plain", "outliers", "outliers_compensated"])
def test_batch256_against_the_fp32_path(l14, tmp_path_factory, variant):
    cfg, w, path, g = l14
    if variant != "plain":
        w2 = synth.plant_outlier_channels(w, compensate=variant == "outliers_compensated")
        path = save(tmp_path_factory, cfg, w2, f"{variant}.safetensors")
    px = synth.preprocess_rgb8(synth.images_u8(4243, 256, cfg.image))
    m = Model.from_file(path, 0, PRECISION_F32)
    ref = m.forward(px)
    m.close()
    m = Model.from_file(path, 0, X3)
    out = m.forward(px)
    m.close()
    assert np.isfinite(out).all()
    ok, err = close(out, ref, 1e-4)
    assert ok, (variant, err)


# ---- same bits -------------------------------------------------------------------------

def test_rows_do_not_depend_on_chunking_last_layer_form_or_streams(l14):
    cfg, w, path, g = l14
    px = synth.preprocess_rgb8(synth.images_u8(4244, 257, cfg.image))
    m = Model.from_file(path, 0, X3)
    ref = m.forward(px)                       # chunks of 256 + 1 (max_batch), two half-chunk streams
    assert np.array_equal(bits(np.concatenate([m.forward(px[:256]), m.forward(px[256:])])), bits(ref))
    sub = px[:40]
    fast = m.forward(sub)
    assert np.array_equal(bits(fast), bits(ref[:40]))
    m.set_option("full_last", 1)
    assert np.array_equal(bits(m.forward(sub)), bits(fast))
    m.set_option("full_last", 0)
    m.set_option("parts", 1)
    assert np.array_equal(bits(m.forward(sub)), bits(fast))
    m.set_option("parts", 2)
    m.set_option("store_nt", 0)
    assert np.array_equal(bits(m.forward(sub)), bits(fast))
    m.close()


def test_pipeline_ingest_writes_the_rows_embed_returns(l14):
    cfg, w, path, g = l14
    px = synth.preprocess_rgb8(synth.images_u8(4245, 40, cfg.image))
    m = Model.from_file(path, 0, X3)
    ref = m.forward(px)
    t = EmbeddingTable(cfg.proj, 0)
    t.insert_synthetic(9, 0, 1000)
    p = Pipeline(m, t)
    first = p.ingest(px)
    p.sync()
    assert np.array_equal(bits(t.rows(first, 40)), bits(ref))
    p.close()
    t.close()
    m.close()


# ---- error codes -----------------------------------------------------------------------

def test_x3_error_codes(l14, tmp_path_factory):
    cfg, w, path, g = l14
    h = c_vp()
    assert lib().mi_clip_load(path.encode(), 0, 4, ctypes.byref(h)) == -1          # precision 4 and above: invalid
    assert lib().mi_clip_load_text(path.encode(), 0, X3, ctypes.byref(h)) == -5     # no text tower in BF16X3
    tiny = synth.VitConfig.tiny()                                                 # hidden 128: not the persistent GEMM's
    tiny_path = save(tmp_path_factory, tiny, synth.vit_weights(tiny, 1), "tiny.safetensors")
    assert lib().mi_clip_load(tiny_path.encode(), 0, X3, ctypes.byref(h)) == -5
    m = Model.from_file(path, 0, X3)
    for key in ("ln_fold", "x24", "qkv_layout"):
        assert lib().mi_clip_set_option(m._h, key.encode(), 1) == -5, key
        assert lib().mi_clip_set_option(m._h, key.encode(), 0) == 0, key
    m.close()
