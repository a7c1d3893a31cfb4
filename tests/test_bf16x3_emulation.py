"""The accuracy argument of MI_PRECISION_BF16X3, checkable without a GPU.

The tiny golden tower in numpy, with every encoder linear (q/k/v, out_proj, fc1, fc2) replaced by an emulated bf16 MFMA
GEMM: operands rounded to bf16 (nearest even), products summed in fp32.  The patch embedding, LayerNorms, attention and
head stay fp32, as in the kernels.  bf16x3 splits both operands, v = hi + lo with hi = bf16(v), lo = bf16(v - hi), and
sums x_hi w_hi + x_lo w_hi + x_hi w_lo; splitting the activations alone (weights hi only, about what BF16_SPLIT does)
leaves the weights' rounding in and misses the 1e-4 bar.
"""
import os

import numpy as np

from conftest import GOLDEN
from image_search_amd import synth
from oracle import vit_numpy


def bf16(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32) << 16).view(np.float32)


def split(a):
    a = np.asarray(a, np.float32)
    hi = bf16(a)
    return hi, bf16(a - hi)


def gemm_x3(x, w):
    (xh, xl), (wh, wl) = split(x), split(w)
    return (xh @ wh.T).astype(np.float32) + (xl @ wh.T).astype(np.float32) + (xh @ wl.T).astype(np.float32)


def gemm_act_split(x, w):
    xh, xl = split(x)
    wh = bf16(w)
    return (xh @ wh.T).astype(np.float32) + (xl @ wh.T).astype(np.float32)


def forward(W, cfg, px, gemm):
    """oracle/vit_numpy.vit_forward in fp32 with `gemm(x, w)` for the encoder linears."""
    ln, qg = vit_numpy._layer_norm, vit_numpy._quick_gelu
    v = "vision_model."
    n = px.shape[0]
    D, P, G, H, dh = cfg.hidden, cfg.patch, cfg.grid, cfg.heads, cfg.head_dim
    pt = px.reshape(n, 3, G, P, G, P).transpose(0, 2, 4, 1, 3, 5).reshape(n, G * G, 3 * P * P)
    pe = pt @ W[v + "embeddings.patch_embedding.weight"].reshape(D, 3 * P * P).T
    cls = np.broadcast_to(W[v + "embeddings.class_embedding"], (n, 1, D))
    h = np.concatenate([cls, pe], axis=1) + W[v + "embeddings.position_embedding.weight"]
    h = ln(h, W[v + "pre_layrnorm.weight"], W[v + "pre_layrnorm.bias"], cfg.eps)
    S = h.shape[1]

    def lin(x, name):
        y = gemm(x.reshape(-1, x.shape[-1]), W[name + ".weight"]) + W[name + ".bias"]
        return y.reshape(x.shape[:-1] + (-1,)).astype(np.float32)

    for i in range(cfg.layers):
        p = f"{v}encoder.layers.{i}."
        y = ln(h, W[p + "layer_norm1.weight"], W[p + "layer_norm1.bias"], cfg.eps)
        q, k, vv = (lin(y, p + f"self_attn.{t}_proj").reshape(n, S, H, dh).transpose(0, 2, 1, 3) for t in "qkv")
        s = (q @ k.transpose(0, 1, 3, 2)) * np.float32(dh ** -0.5)
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        ctx = ((e / e.sum(axis=-1, keepdims=True)) @ vv).transpose(0, 2, 1, 3).reshape(n, S, D)
        h = h + lin(ctx, p + "self_attn.out_proj")
        y = ln(h, W[p + "layer_norm2.weight"], W[p + "layer_norm2.bias"], cfg.eps)
        h = h + lin(qg(lin(y, p + "mlp.fc1")), p + "mlp.fc2")
    pooled = ln(h[:, 0, :], W[v + "post_layernorm.weight"], W[v + "post_layernorm.bias"], cfg.eps)
    return pooled @ W["visual_projection.weight"].T


def rel_err(out, ref):
    rms = float(np.sqrt((np.asarray(ref, np.float64) ** 2).mean()))
    ok = np.allclose(out, ref, rtol=1e-4, atol=1e-4 * rms)
    return ok, float(np.abs(out - ref).max() / rms)


def _tiny():
    cfg = synth.VitConfig.tiny()
    g = np.load(os.path.join(GOLDEN, "vit_tiny.npz"))
    w = {k: v.astype(np.float32) for k, v in synth.vit_weights(cfg, int(g["seed"])).items()}
    px = synth.preprocess_rgb8(synth.images_u8(int(g["image_seed"]), int(g["n_img"]), cfg.image))
    return cfg, w, px, g["embeds_f64"]


def test_emulated_fp32_gemm_reproduces_the_golden():
    cfg, w, px, ref = _tiny()
    ok, err = rel_err(forward(w, cfg, px, lambda x, wt: x @ wt.T), ref)
    assert ok and err < 1e-5, err


def test_bf16x3_with_fp32_attention_meets_1e4():
    cfg, w, px, ref = _tiny()
    ok, err = rel_err(forward(w, cfg, px, gemm_x3), ref)
    assert ok and err < 5e-5, err


def test_splitting_the_activations_alone_does_not():
    cfg, w, px, ref = _tiny()
    ok, err = rel_err(forward(w, cfg, px, gemm_act_split), ref)
    assert not ok and err > 1e-3, err
