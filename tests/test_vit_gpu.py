"""Seam A parity on a real MI355X, through the C ABI (mi_clip_* and the op hooks).

Tolerances (north_star: "within 1e-4 relative on embedding floats"):
  fp32 path : |y - ref| <= 1e-4 * (|ref| + rms(ref))      (np.allclose rtol = atol/rms = 1e-4)
  bf16 path : reported, and bounded at 3e-2 * rms(ref) — bf16 operands cannot meet 1e-4 over
              24 layers (SURVEY.md §7 "hard parts"); it is the throughput path, fp32 the parity path.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from image_search_amd import ops, synth
from image_search_amd._lib import MiError
from image_search_amd.clip import PRECISION_BF16, PRECISION_F32, Model, clip_vit_large_patch14
from oracle import vit_numpy

pytestmark = pytest.mark.gpu


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32) << 16).view(np.float32)


def close(out, ref, tol):
    rms = float(np.sqrt((np.asarray(ref, np.float64) ** 2).mean()))
    return np.allclose(out, ref, rtol=tol, atol=tol * rms), float(np.abs(out - ref).max() / rms)


@pytest.fixture(scope="module")
def tiny(built, tmp_path_factory):
    cfg = synth.VitConfig.tiny()
    g = np.load(os.path.join(GOLDEN, "vit_tiny.npz"))
    w = synth.vit_weights(cfg, int(g["seed"]))
    path = str(tmp_path_factory.mktemp("w") / "tiny.safetensors")
    synth.save_safetensors(w, path, {"num_attention_heads": cfg.heads})
    px = synth.preprocess_rgb8(synth.images_u8(int(g["image_seed"]), int(g["n_img"]), cfg.image))
    return cfg, w, path, px, g


@pytest.fixture(scope="module")
def l14(built, tmp_path_factory):
    cfg = synth.VitConfig.vit_l14()
    g = np.load(os.path.join(GOLDEN, "vit_l14.npz"))
    w = synth.vit_weights(cfg, int(g["seed"]))
    path = str(tmp_path_factory.mktemp("w") / "l14.safetensors")
    synth.save_safetensors(w, path, {"num_attention_heads": cfg.heads})
    u8 = synth.images_u8(int(g["image_seed"]), int(g["n_img"]), cfg.image)
    return cfg, w, path, u8, g


# ---- per-op parity ------------------------------------------------------------------

@pytest.mark.parametrize("prec", [PRECISION_F32, PRECISION_BF16])
def test_linear_exact_on_integers_asymmetric(built, prec):
    rng = np.random.default_rng(0)
    x = rng.integers(-3, 4, (256, 128)).astype(np.float32)
    w = rng.integers(-3, 4, (384, 128)).astype(np.float32)
    b = rng.integers(-5, 6, 384).astype(np.float32)
    assert np.array_equal(ops.linear(x, w, b, ops.EPI_BIAS, prec), x @ w.T + b)
    assert np.array_equal(ops.linear(x, w, None, ops.EPI_STORE_F32, prec), x @ w.T)


@pytest.mark.parametrize("prec,tol", [(PRECISION_F32, 2e-6), (PRECISION_BF16, 1.2e-2)])
@pytest.mark.parametrize("shape", [(300, 384, 1024), (257, 1024, 4096), (1000, 4096, 1024), (64, 128, 640)])
def test_linear_epilogues(built, prec, tol, shape):
    m, n, k = shape
    rng = np.random.default_rng(1)
    x = rng.standard_normal((m, k)).astype(np.float32)
    w = (rng.standard_normal((n, k)) * k ** -0.5).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    res = rng.standard_normal((m, n)).astype(np.float32)
    xr, wr = (bf16_round(x), bf16_round(w)) if prec else (x, w)
    ref = xr.astype(np.float64) @ wr.astype(np.float64).T + b
    scale = float(np.abs(ref).max())
    assert np.abs(ops.linear(x, w, b, ops.EPI_BIAS, prec) - ref).max() <= tol * scale
    assert np.abs(ops.linear(x, w, b, ops.EPI_BIAS_RESID, prec, out=res) - (ref + res)).max() <= 3e-6 * scale
    assert np.abs(ops.linear(x, w, b, ops.EPI_BIAS_QGELU, prec) - ref / (1 + np.exp(-1.702 * ref))).max() <= tol * scale


@pytest.mark.parametrize("prec,tol", [(PRECISION_F32, 2e-6), (PRECISION_BF16, 1.2e-2)])
@pytest.mark.parametrize("shape", [(257, 2304, 768), (300, 1280, 5120), (64, 512, 2048)])
def test_linear_epilogues_at_the_other_widths(built, prec, tol, shape):
    """test_linear_epilogues at the q/k/v shape of a 768-wide tower (nine column tiles), the fc2 shape of a 1280-wide one
    (K = 5120) and the fc2 shape of a 512-wide one on 64 rows — same operands' recipe, same tolerances."""
    m, n, k = shape
    rng = np.random.default_rng(1)
    x = rng.standard_normal((m, k)).astype(np.float32)
    w = (rng.standard_normal((n, k)) * k ** -0.5).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    res = rng.standard_normal((m, n)).astype(np.float32)
    xr, wr = (bf16_round(x), bf16_round(w)) if prec else (x, w)
    ref = xr.astype(np.float64) @ wr.astype(np.float64).T + b
    scale = float(np.abs(ref).max())
    assert np.abs(ops.linear(x, w, b, ops.EPI_BIAS, prec) - ref).max() <= tol * scale
    assert np.abs(ops.linear(x, w, b, ops.EPI_BIAS_RESID, prec, out=res) - (ref + res)).max() <= 3e-6 * scale
    assert np.abs(ops.linear(x, w, b, ops.EPI_BIAS_QGELU, prec) - ref / (1 + np.exp(-1.702 * ref))).max() <= tol * scale


@pytest.mark.parametrize("grid", ["8", "3", "64"])
def test_persistent_gemm_rounds_and_split_tail(built, monkeypatch, grid):
    """bf16 persistent 256x256 kernel: several tiles per workgroup, the counted store/LDS-DMA
    queue across tile boundaries, and the quadrant tasks of a short last round — exact on
    small integers, so any stale tile or misplaced store shows."""
    monkeypatch.setenv("MI_OP_GRID", grid)
    rng = np.random.default_rng(7)
    for (m, n, k) in ((2304, 512, 256), (2304, 512, 128), (700, 1024, 320), (256, 256, 64 * 9)):
        x = rng.integers(-2, 3, (m, k)).astype(np.float32)
        w = rng.integers(-1, 2, (n, k)).astype(np.float32)
        b = rng.integers(-3, 4, n).astype(np.float32)
        ref = x @ w.T + b
        assert np.abs(ref).max() <= 256  # exactly representable in bf16
        assert np.array_equal(ops.linear(x, w, b, ops.EPI_BIAS, PRECISION_BF16), ref), (m, n, k)
    x = rng.standard_normal((2304, 256)).astype(np.float32); w = (rng.standard_normal((512, 256)) / 16).astype(np.float32)
    b = rng.standard_normal(512).astype(np.float32)
    ref = bf16_round(x).astype(np.float64) @ bf16_round(w).astype(np.float64).T + b
    got = ops.linear(x, w, b, ops.EPI_BIAS_QGELU, PRECISION_BF16)
    assert np.abs(got - ref / (1 + np.exp(-1.702 * ref))).max() <= 1.2e-2 * np.abs(ref).max()


@pytest.mark.parametrize("prec,tol", [(PRECISION_F32, 5e-6), (PRECISION_BF16, 6e-3)])
@pytest.mark.parametrize("S", [17, 50, 197, 257])
def test_attention(built, prec, tol, S):
    rng = np.random.default_rng(2)
    n, H = 2, 3
    D = 64 * H
    qkv = rng.standard_normal((n, S, 3 * D)).astype(np.float32)
    qkv[0, 5, :D] *= 6.0  # one sharply peaked query row
    r = bf16_round(qkv) if prec else qkv
    q, k, v = [r[..., i * D:(i + 1) * D].reshape(n, S, H, 64).transpose(0, 2, 1, 3).astype(np.float64) for i in range(3)]
    if prec and S > 64:
        # attn32 works in the exp2 domain: a plain q (this hook) is scaled by log2(e)/8 and rounded to bf16 once
        # more on its way into the MFMA; in the tower that factor sits in W_q / b_q and q is rounded once
        c2 = np.float32(0.125 * 1.4426950408889634)
        q = bf16_round(q.astype(np.float32) * c2).astype(np.float64) / np.float64(c2)
    s = q @ k.transpose(0, 1, 3, 2) * 0.125
    e = np.exp(s - s.max(-1, keepdims=True))
    ref = ((e / e.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(n, S, D)
    assert np.abs(ops.attention(qkv, H, prec) - ref).max() <= tol * np.abs(ref).max()


@pytest.mark.parametrize("S", [5, 16, 77, 80, 81, 197, 208, 257, 272, 273])
def test_attention_fp32_on_the_matrix_pipe_and_one_thread_per_query_agree(built, monkeypatch, S):
    """The parity path's attention runs on exact-f32 MFMAs for S <= 272 (attn_f32_mfma_kernel: LDS images of 80 / 208 / 272
    key rows) and one thread per query beyond: both against numpy fp64 at 5e-6, on both sides of every size boundary, with a
    sharply peaked query and a partly masked last key tile."""
    rng = np.random.default_rng(300 + S)
    n, H = 2, 2
    D = 64 * H
    qkv = rng.standard_normal((n, S, 3 * D)).astype(np.float32)
    qkv[0, S // 2, :D] *= 6.0
    q, k, v = [qkv[..., i * D:(i + 1) * D].reshape(n, S, H, 64).transpose(0, 2, 1, 3).astype(np.float64) for i in range(3)]
    sc = q @ k.transpose(0, 1, 3, 2) * 0.125
    p = np.exp(sc - sc.max(-1, keepdims=True))
    ref = (p / p.sum(-1, keepdims=True) @ v).transpose(0, 2, 1, 3).reshape(n, S, D)
    got = ops.attention(qkv, H, PRECISION_F32)
    assert np.abs(got - ref).max() <= 5e-6 * np.abs(ref).max()
    monkeypatch.setenv("MI_OP_ATTN_F32_MFMA", "0")
    old = ops.attention(qkv, H, PRECISION_F32)
    assert np.abs(old - ref).max() <= 5e-6 * np.abs(ref).max()


def _peaked_qkv(S, n, H, beta, gamma, seed):
    """Query i attends to exactly one key pi(i): keys are random +-1 codes (dims 8..63) plus a common
    component (dims 0..7 = +1); q_i = beta * code(pi(i)) - gamma * common.  Scores (natural units):
    (beta * 56 - 8 gamma) / 8 on the chosen key, at most about (beta * 28 - 8 gamma) / 8 elsewhere."""
    rng = np.random.default_rng(seed)
    D = 64 * H
    qkv = np.zeros((n, S, 3 * D), np.float32)
    pi = np.stack([rng.permutation(S) for _ in range(n * H)]).reshape(n, H, S)
    for b in range(n):
        for h in range(H):
            code = rng.choice([-1.0, 1.0], (S, 64)).astype(np.float32)
            code[:, :8] = 1.0
            q = beta * code[pi[b, h]]
            q[:, :8] = -gamma
            qkv[b, :, h * 64:(h + 1) * 64] = q
            qkv[b, :, D + h * 64:D + (h + 1) * 64] = code
            qkv[b, :, 2 * D + h * 64:2 * D + (h + 1) * 64] = rng.integers(-4, 5, (S, 64))
    return qkv, pi


@pytest.mark.parametrize("S", [65, 100, 128, 197, 224, 257, 288])
@pytest.mark.parametrize("beta,gamma,why", [(4.0, 0.0, "in range: the unshifted pass"),
                                            (48.0, 0.0, "numerators overflow: shifted pass"),
                                            (4.0, 200.0, "every numerator underflows: shifted pass")])
def test_attention32_one_hot_and_exponent_window(built, S, beta, gamma, why):
    """attn32 (32-query tiles, no max pass): each query must return exactly its key's V row — any wrong
    key / column / tile mapping shows — also when the scores leave the window that the unshifted
    softmax numerators can represent, on both sides."""
    n, H = 2, 2
    D = 64 * H
    qkv, pi = _peaked_qkv(S, n, H, beta, gamma, 11 + S)
    out = ops.attention(qkv, H, PRECISION_BF16)
    for b in range(n):
        for h in range(H):
            want = qkv[b, pi[b, h], 2 * D + h * 64:2 * D + (h + 1) * 64]
            got = out[b, :, h * 64:(h + 1) * 64]
            assert np.abs(got - want).max() <= 2e-3, (why, S, b, h, np.abs(got - want).max())


@pytest.mark.parametrize("S", [50, 77, 100, 197, 224, 288])
def test_old_bf16_attention_kernel_one_hot(built, monkeypatch, S):
    """The 16-query-tile kernel (attn_ver 1, MI_OP_ATTN=1) at its other instantiations — <64,50>, <96,0>, <224,0> below and at
    its last key tile, <224,197>, <288,0>: every query returns exactly its key's V row, so a wrong key, column or tile mapping
    shows as another row."""
    monkeypatch.setenv("MI_OP_ATTN", "1")
    n, H = 2, 2
    D = 64 * H
    qkv, pi = _peaked_qkv(S, n, H, 4.0, 0.0, 11 + S)
    out = ops.attention(qkv, H, PRECISION_BF16)
    for b in range(n):
        for h in range(H):
            want = qkv[b, pi[b, h], 2 * D + h * 64:2 * D + (h + 1) * 64]
            got = out[b, :, h * 64:(h + 1) * 64]
            assert np.abs(got - want).max() <= 2e-3, (S, b, h, np.abs(got - want).max())


def test_attention32_forced_shift_and_old_kernel_agree(built, monkeypatch):
    rng = np.random.default_rng(5)
    n, H, S = 3, 2, 257
    qkv = rng.standard_normal((n, S, 3 * 64 * H)).astype(np.float32)
    qkv[1, 9, :64 * H] *= 5.0
    base = ops.attention(qkv, H, PRECISION_BF16)
    monkeypatch.setenv("MI_OP_ATTN_SHIFT", "1")
    shifted = ops.attention(qkv, H, PRECISION_BF16)
    monkeypatch.delenv("MI_OP_ATTN_SHIFT")
    monkeypatch.setenv("MI_OP_ATTN", "1")
    old = ops.attention(qkv, H, PRECISION_BF16)
    scale = np.abs(base).max()
    assert np.abs(shifted - base).max() <= 8e-3 * scale     # same mathematics, bf16 numerators rounded at another scale
    assert np.abs(old - base).max() <= 8e-3 * scale         # the 16-query-tile kernel (q rounded before its scale)


@pytest.mark.parametrize("S,n,H", [(257, 20, 16), (197, 5, 12), (100, 3, 2), (257, 1, 16)])
def test_attention32_row_pitch_and_pair_order_do_not_change_a_bit(built, monkeypatch, S, n, H):
    """The tower pads the rows of q|k|v (a head's 128-byte pieces then spread over the memory channels) and starts the
    32 workgroups that share an XCD on different heads.  Both are layouts / orders: the kernel on padded rows (NaN patterns
    between them) and with either start order returns the bits of the dense, plain-order run — persistent grid (n * H >
    256 pairs), short grids and one image."""
    rng = np.random.default_rng(40 + S)
    qkv = rng.standard_normal((n, S, 3 * 64 * H)).astype(np.float32)
    monkeypatch.setenv("MI_OP_ATTN_ORDER", "0")
    base = ops.attention(qkv, H, PRECISION_BF16)
    assert np.isfinite(base).all()
    for pad, order in ((0, 1), (64, 0), (128, 1), (192, 1), (1024, 0)):
        monkeypatch.setenv("MI_OP_ATTN_QKV_PAD", str(pad))
        monkeypatch.setenv("MI_OP_ATTN_ORDER", str(order))
        got = ops.attention(qkv, H, PRECISION_BF16)
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (pad, order)
    # head-major planes [3][H][Mp][64] (option "qkv_layout" = 1): a head's K / V / q of one image is one contiguous block,
    # the next image's rows lie right behind it and NaN patterns behind the last one — rows >= S must still read as zeros
    monkeypatch.delenv("MI_OP_ATTN_QKV_PAD")
    monkeypatch.setenv("MI_OP_ATTN_LAYOUT", "1")
    for order, nt in ((0, 1), (1, 1), (1, 0)):
        monkeypatch.setenv("MI_OP_ATTN_ORDER", str(order))
        monkeypatch.setenv("MI_OP_ATTN_NT", str(nt))   # the cache policy of the K / V / q stream: a hint, never a value
        got = ops.attention(qkv, H, PRECISION_BF16)
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), ("planes", order, nt)
    monkeypatch.delenv("MI_OP_ATTN_LAYOUT")
    monkeypatch.setenv("MI_OP_ATTN_NT", "0")
    assert np.array_equal(ops.attention(qkv, H, PRECISION_BF16).view(np.uint32), base.view(np.uint32)), "rows, default cache policy"


def _layernorm_against_fp64(prec, tol, D, rows):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((rows, D)) * 3 + 1).astype(np.float32)
    w = rng.standard_normal(D).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    xd = x.astype(np.float64)
    d = xd - xd.mean(-1, keepdims=True)
    ref = d / np.sqrt((d * d).mean(-1, keepdims=True) + 1e-5) * w + b
    got = ops.layernorm(x, w, b, 1e-5, prec)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= tol * np.abs(ref).max()


@pytest.mark.parametrize("prec,tol", [(PRECISION_F32, 2e-6), (PRECISION_BF16, 5e-3)])
@pytest.mark.parametrize("D", [128, 256, 384, 512, 768, 1024, 1280, 1536, 1664])
def test_layernorm(built, prec, tol, D):
    """Every width of the LayerNorm dispatch (D = 64 * VEC * NT): 37 rows are nine full workgroups of four and one row."""
    _layernorm_against_fp64(prec, tol, D, 37)


@pytest.mark.parametrize("prec,tol", [(PRECISION_F32, 2e-6), (PRECISION_BF16, 5e-3)])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("D", [384, 1664])
def test_layernorm_ragged_last_workgroup_at_the_two_lane_pair_widths(built, prec, tol, D, rows):
    """VEC = 2 with NT = 3 and 13: one row alone in its workgroup, and a full workgroup followed by one row."""
    _layernorm_against_fp64(prec, tol, D, rows)


# ---- whole model ----------------------------------------------------------------------

def test_tiny_fp32_matches_transformers_golden_and_oracle(tiny):
    cfg, w, path, px, g = tiny
    m = clip_vit_large_patch14.Model.from_file(path, 0, PRECISION_F32)
    assert (m.image, m.patch, m.tokens, m.hidden, m.layers, m.heads, m.ff, m.proj) == (56, 14, 17, 128, 2, 2, 512, 64)
    out = m.forward(px)
    ok, err = close(out, g["embeds_hf_f32"], 1e-4)
    assert ok, err
    ok, err = close(out, vit_numpy.vit_forward(w, cfg, px, np.float32), 1e-4)
    assert ok, err
    assert m.forward(px[:0]).shape == (0, 64)           # n = 0: clip.rs:112-118
    assert np.array_equal(m.forward(px[1:2]), out[1:2])  # batch-independent, deterministic
    m.close()


def test_tiny_bf16_within_stated_bound(tiny):
    cfg, w, path, px, g = tiny
    m = Model.from_file(path, 0, PRECISION_BF16)
    ok, err = close(m.forward(px), g["embeds_f64"], 3e-2)
    assert ok, err
    m.close()


def test_l14_fp32_matches_golden(l14):
    """BASELINE config[1] in miniature: full ViT-L/14, fp32, vs the committed golden embeddings."""
    cfg, w, path, u8, g = l14
    m = Model.from_file(path, 0, PRECISION_F32)
    assert (m.tokens, m.hidden, m.layers, m.heads, m.ff, m.proj) == (257, 1024, 24, 16, 4096, 768)
    px = synth.preprocess_rgb8(u8)
    out = m.forward(px)
    ok, err = close(out, g["embeds_hf_f32"], 1e-4)
    assert ok, err
    ok, err = close(out, g["embeds_f64"], 1e-4)
    assert ok, err
    # fused u8 path == preprocess-then-embed (image_prepare_resnet, clip.rs:153-175)
    assert np.array_equal(m.forward_rgb8(u8), out)
    m.close()


def test_l14_fp32_batch32_is_baseline_config_2(l14):
    """BASELINE config 2 at its own batch size: "ViT-L/14 image encoder, batch = 32 fp32, correctness vs CPU"
    (/root/reference/server/src/clip.rs:112-124 with a chunk of 32).  M = 32 * 257 = 8 224 token rows: other tile counts
    and another tail round than the n = 2 / n = 4 runs the fixtures cover.  Rows {0, 15, 16, 31} against the numpy
    oracle (fp32 arithmetic, <= 1e-4), rows 0-1 against the committed transformers golden, and rows 0-1 bit-equal to
    the n = 2 run: the fp32 GEMM's result for a row must not depend on how many rows the batch holds."""
    cfg, w, path, u8, g = l14
    u8_32 = synth.images_u8(int(g["image_seed"]), 32, cfg.image)
    assert np.array_equal(u8_32[:2], u8)                       # the generator is counter-based: same first images
    px = synth.preprocess_rgb8(u8_32)
    m = Model.from_file(path, 0, PRECISION_F32)
    out = m.forward(px)
    assert out.shape == (32, 768) and np.isfinite(out).all()
    rows = [0, 15, 16, 31]
    ref = vit_numpy.vit_forward(w, cfg, px[rows], np.float32)
    ok, err = close(out[rows], ref, 1e-4)
    assert ok, err
    ok, err = close(out[:2], g["embeds_hf_f32"], 1e-4)
    assert ok, err
    two = m.forward(px[:2])
    assert np.array_equal(two.view(np.uint32), out[:2].view(np.uint32))
    m.close()


def test_l14_bf16_batch_and_chunking(l14, monkeypatch):
    cfg, w, path, u8, g = l14
    px = synth.preprocess_rgb8(u8)
    m = Model.from_file(path, 0, PRECISION_BF16)
    out = m.forward(px)
    ok, err = close(out, g["embeds_f64"], 3e-2)
    assert ok, err
    big = np.concatenate([px] * 3)[:5]        # 5 images, chunked as 2+2+1 below
    ref5 = m.forward(big)
    m.close()
    monkeypatch.setenv("MI_CLIP_MAX_BATCH", "2")
    m2 = Model.from_file(path, 0, PRECISION_BF16)
    assert np.array_equal(m2.forward(big), ref5)
    assert np.array_equal(ref5[:2], out) and np.array_equal(ref5[2:4], out)
    m2.close()


def test_device_entry_point_matches_host_entry_point(tiny):
    import torch
    cfg, w, path, px, g = tiny
    m = Model.from_file(path, 0, PRECISION_F32)
    ref = m.forward(px)
    d_in = torch.from_numpy(px).cuda()
    d_out = torch.empty((px.shape[0], 64), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        m.forward_device(d_in.data_ptr(), px.shape[0], d_out.data_ptr(), st.cuda_stream)
    st.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), ref)
    m.close()


@pytest.mark.parametrize("inventory", [{}, {"decomposed_ln": True}, {"decomposed_ln": True, "coalesced": False}],
                         ids=["fused-ln", "decomposed-ln", "decomposed-ln-uncoalesced"])
@pytest.mark.parametrize("prec", [PRECISION_F32, PRECISION_BF16])
def test_model_from_burn_mpk_equals_model_from_safetensors(tiny, tmp_path, prec, inventory):
    """Model::from_file on the kind of file `-w` names (vision_model.mpk, server/src/server_arguments.rs:8-9): the
    same tensors through the Burn-record reader (shape / module / order mapping, Linear weights transposed back) must
    give the very same embeddings as the safetensors file — for LayerNorm modules, for the DECOMPOSED LayerNorm of the
    opset-16 graph the reference really builds (clip/scripts/upgrade_opset.py:9-28: gamma / beta as bare constants, scalar
    and integer constants interleaved) and for that graph with MatMul + Add not coalesced into Linear modules.
    Still parity unpinned: no file written by burn-import itself exists offline."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from make_synthetic_mpk import write_mpk
    cfg, w, path, px, g = tiny
    mpk = str(tmp_path / "vision_model.mpk")
    write_mpk(w, cfg, mpk, **inventory)
    a = Model.from_file(path, 0, prec)
    b = Model.from_file(mpk, 0, prec)
    assert (b.tokens, b.hidden, b.layers, b.ff, b.proj) == (a.tokens, a.hidden, a.layers, a.ff, a.proj)
    assert np.array_equal(a.forward(px).view(np.uint32), b.forward(px).view(np.uint32))
    a.close(); b.close()


def test_load_errors_are_codes(built, mi, tmp_path):
    h = ctypes.c_void_p()
    assert mi.mi_clip_load(b"/nonexistent/x.safetensors", 0, 0, ctypes.byref(h)) == -2 and not h.value
    bad = tmp_path / "bad.safetensors"
    bad.write_bytes(b"\x10\x00\x00\x00\x00\x00\x00\x00{\"a\":1}        ")
    assert mi.mi_clip_load(str(bad).encode(), 0, 0, ctypes.byref(h)) == -2
    assert mi.mi_clip_load(str(bad).encode(), 0, 7, ctypes.byref(h)) == -1      # bad precision
    cfg = synth.VitConfig.tiny()
    w = synth.vit_weights(cfg, 1)
    del w["visual_projection.weight"]
    p = str(tmp_path / "missing.safetensors")
    synth.save_safetensors(w, p)
    with pytest.raises(MiError, match="visual_projection.weight"):
        Model.from_file(p, 0, 0)


# ---- text tower (server/src/clip.rs:19-23) ---------------------------------

from image_search_amd.clip import TextModel


@pytest.mark.parametrize("name,cfg", [("tiny", synth.TextConfig.tiny()), ("l14", synth.TextConfig.clip_l14())])
def test_text_tower_fp32_matches_transformers_golden_and_oracle(built, tmp_path, name, cfg):
    g = np.load(os.path.join(GOLDEN, f"text_{name}.npz"))
    w = synth.vit_weights(cfg, int(g["seed"]))
    path = str(tmp_path / "text.safetensors")
    synth.save_safetensors(w, path, {"num_attention_heads": cfg.heads})
    ids = synth.token_ids(cfg, int(g["ids_seed"]), int(g["n_seq"]))
    m = TextModel.from_file(path)
    assert (m.positions, m.hidden, m.layers, m.proj) == (cfg.positions, cfg.hidden, cfg.layers, cfg.proj)
    out = m.embed(ids)
    ok, err = close(out, g["embeds_hf_f32"], 1e-4)           # transformers CLIPTextModelWithProjection
    assert ok, err
    ok, err = close(out, g["embeds_f64"], 1e-4)
    assert ok, err
    ok, err = close(out, vit_numpy.text_forward(w, cfg, ids, np.float32), 1e-4)
    assert ok, err
    # causality: tokens after the EOS do not change the pooled embedding; more sequences than one pass
    ids2 = ids.copy()
    for i in range(ids2.shape[0]):
        e = int(ids2[i].argmax())
        ids2[i, e + 1:] = 0
    assert np.array_equal(m.embed(ids2), out)
    assert m.embed(ids[:0]).shape == (0, cfg.proj)
    many = np.concatenate([ids] * 3)
    assert np.array_equal(m.embed(many)[-ids.shape[0]:], out)


@pytest.mark.parametrize("name,cfg", [("tiny", synth.TextConfig.tiny()), ("l14", synth.TextConfig.clip_l14())])
def test_text_tower_bf16_within_the_bf16_bound_and_causal(built, tmp_path, name, cfg):
    """The request-path text tower (bf16 MFMA GEMMs on 77 rows, causal mask in the bf16 attention kernel) against the
    transformers golden at the bf16 bound of the image tower (3e-2 * rms); fp32 stays the parity path."""
    from image_search_amd.clip import PRECISION_BF16 as BF16
    g = np.load(os.path.join(GOLDEN, f"text_{name}.npz"))
    w = synth.vit_weights(cfg, int(g["seed"]))
    path = str(tmp_path / "text.safetensors")
    synth.save_safetensors(w, path, {"num_attention_heads": cfg.heads})
    ids = synth.token_ids(cfg, int(g["ids_seed"]), int(g["n_seq"]))
    m = TextModel.from_file(path, 0, BF16)
    out = m.embed(ids)
    ok, err = close(out, g["embeds_f64"], 3e-2)
    assert ok, err
    print(f"text tower {name} bf16: max|err|/rms = {err:.2e}")
    ids2 = ids.copy()                         # causality: tokens behind the EOS do not reach the pooled row
    for i in range(ids2.shape[0]):
        ids2[i, int(ids2[i].argmax()) + 1:] = 0
    assert np.array_equal(m.embed(ids2), out)
    assert np.array_equal(m.embed(np.concatenate([ids] * 3))[-ids.shape[0]:], out)
    m.close()


def test_one_text_query_takes_the_skinny_gemm_path_within_the_same_bound(built, tmp_path):
    """server/src/clip.rs:19-23 embeds ONE query per search: n == 1 on the CLIP-L text geometry runs on the skinny GEMMs
    (vit.hip forward_text_one: every workgroup one K chunk, all loads in flight at once).  Same graph, same bf16 rounding
    points (fc2's output stays fp32): each row must meet the bf16 bound against the transformers golden on its own, agree
    with the batched kernels far inside that bound, and keep the causal mask."""
    from image_search_amd.clip import PRECISION_BF16 as BF16
    cfg = synth.TextConfig.clip_l14()
    g = np.load(os.path.join(GOLDEN, "text_l14.npz"))
    w = synth.vit_weights(cfg, int(g["seed"]))
    path = str(tmp_path / "text.safetensors")
    synth.save_safetensors(w, path, {"num_attention_heads": cfg.heads})
    ids = synth.token_ids(cfg, int(g["ids_seed"]), int(g["n_seq"]))
    m = TextModel.from_file(path, 0, BF16)
    batched = m.embed(ids)                                         # n > 1: the batched kernels
    rms = float(np.sqrt((np.asarray(g["embeds_f64"], np.float64) ** 2).mean()))
    for i in range(ids.shape[0]):
        one = m.embed(ids[i:i + 1])                                # n == 1: the skinny path
        err = float(np.abs(one[0] - g["embeds_f64"][i]).max() / rms)
        assert err <= 3e-2, (i, err)
        assert float(np.abs(one[0] - batched[i]).max() / rms) <= 2e-2
        m.set_option("text_fast", 0)
        assert np.array_equal(m.embed(ids[i:i + 1])[0], batched[i])   # the same query through the batched kernels: their bits
        m.set_option("text_fast", 1)
        cut = ids[i:i + 1].copy()
        cut[0, int(cut[0].argmax()) + 1:] = 0                      # tokens behind the EOS cannot reach the pooled row
        assert np.array_equal(m.embed(cut), one)
        assert np.array_equal(m.embed(ids[i:i + 1]), one)          # deterministic: fixed summation orders throughout
        # out_proj inside the attention launch (default) against the two-launch form with its bf16 delta: another rounding
        # sequence of the same graph, both inside the bound, the causal mask kept
        m.set_option("text_fuse", 0)
        two = m.embed(ids[i:i + 1])
        err2 = float(np.abs(two[0] - g["embeds_f64"][i]).max() / rms)
        assert err2 <= 3e-2 and float(np.abs(two[0] - one[0]).max() / rms) <= 2e-2, (i, err2)
        assert np.array_equal(m.embed(cut), two)
        m.set_option("text_fuse", 1)
        assert np.array_equal(m.embed(ids[i:i + 1]), one)
        print(f"text query {i}, skinny path: max|err|/rms = {err:.2e} (attention + out_proj in one launch), {err2:.2e} (two launches)")
    # the captured graph holds buffer addresses: a larger batch reallocates the workspace, the graph must go with it
    first = m.embed(ids[:1])
    for _ in range(3):
        assert np.array_equal(m.embed(ids[:1]), first)             # eager, capturing, replayed
    big = np.concatenate([ids] * 40)                               # grows the workspace (and takes the batched kernels)
    assert np.array_equal(m.embed(big)[:ids.shape[0]], batched)
    for _ in range(4):
        assert np.array_equal(m.embed(ids[:1]), first)             # a fresh eager / capture / replay cycle on the new buffers
    # options that re-size the IMAGE tower's activation sets are refused on a text handle (its workspace is another one:
    # freeing m->ws under it would leave the text buffers dangling), and refusing leaves the handle usable
    for key, value in (("qkv_pad", 64), ("parts", 1)):
        with pytest.raises(Exception):
            m.set_option(key, value)
    assert np.array_equal(m.embed(ids[:1]), first)
    m.close()


def test_text_tower_errors_are_codes(built, tmp_path):
    cfg = synth.TextConfig.tiny()
    path = str(tmp_path / "text.safetensors")
    synth.save_safetensors(synth.vit_weights(cfg, 2), path, {"num_attention_heads": cfg.heads})
    m = TextModel.from_file(path)
    bad = synth.token_ids(cfg, 1, 2)
    bad[1, 3] = cfg.vocab
    with pytest.raises(MiError) as e:
        m.embed(bad)
    assert e.value.code == -1
    from image_search_amd._lib import c_vp, lib
    h = c_vp()
    assert lib().mi_clip_load_text(path.encode(), 0, 2, ctypes.byref(h)) == -5                    # no split mode for text
    assert lib().mi_clip_load(path.encode(), 0, PRECISION_F32, ctypes.byref(h)) != 0             # no vision tensors in the file
    out = np.zeros((1, cfg.proj), np.float32)
    assert lib().mi_clip_embed(m._h, out.ctypes.data, 1, out.ctypes.data) == -1                   # image entry point, text handle


@pytest.mark.parametrize("order", [0, 1, 2, 4])
def test_persistent_gemm_random_shapes_and_grids(built, monkeypatch, order):
    """Seeded sweep over (rows, N, K, workgroup count, tile order): full rounds, split tails of every size, K depths
    from 2 to 13 K tiles, with and without the activation — exact on small integers every time.  order = the
    column-group tile order of the persistent kernel (0 = row-major; the tower's default is 4, which needs N >= 2048)."""
    rng = np.random.default_rng(2026)
    monkeypatch.setenv("MI_OP_GEMM_ORDER", str(order))
    for case in range(24):
        grid = int(rng.choice([1, 2, 3, 5, 8, 13, 16, 32, 256]))
        m = int(rng.integers(1, 9)) * 256 - int(rng.integers(0, 200))
        n = int(rng.choice([256, 512, 768, 1024, 2048, 3072] if order == 4 else [256, 512, 768, 1024]))
        k = int(rng.integers(2, 14)) * 64
        monkeypatch.setenv("MI_OP_GRID", str(grid))
        x = rng.integers(-2, 3, (m, k)).astype(np.float32)
        w = rng.integers(-1, 2, (n, k)).astype(np.float32)
        b = rng.integers(-3, 4, n).astype(np.float32)
        ref = x @ w.T + b
        assert np.abs(ref).max() <= 256
        got = ops.linear(x, w, b, ops.EPI_BIAS, PRECISION_BF16)
        assert np.array_equal(got, ref), (case, grid, m, n, k)


@pytest.mark.parametrize("ln_fold", [1, 0])
def test_ab_hooks_of_the_bf16_tower_do_not_change_a_bit(l14, ln_fold):
    """im2col_rows (the LDS-staged patch gather), ln_nt (non-temporal write-back of the residual stream) and gemm_order
    (which tile a workgroup of the persistent GEMM visits when) move bytes differently, never compute differently: 40 images
    (two half-chunk streams), every combination, the same bits — in the LayerNorm-free layer loop (ln_fold = 1, the default)
    and in the LayerNorm one.  x24 = 0 (fp32 residual rows under ln_fold = 0) is another rounding, inside the bf16 bound."""
    cfg, w, path, u8, g = l14
    px = synth.preprocess_rgb8(synth.images_u8(78, 40, cfg.image))
    m = Model.from_file(path, 0, PRECISION_BF16)
    m.set_option("ln_fold", ln_fold)
    ref = m.forward(px)
    if not ln_fold:
        m.set_option("x24", 0)
        o32 = m.forward(px)
        m.set_option("x24", 1)
        assert np.abs(o32 - ref).max() <= 3e-2 * float(np.sqrt((ref.astype(np.float64) ** 2).mean()))
        assert np.array_equal(m.forward(px).view(np.uint32), ref.view(np.uint32))
    for rows_, nt, order in ((0, 0, 4), (0, 1, 0), (1, 3, 3), (1, 0, 8)):
        m.set_option("im2col_rows", rows_)
        m.set_option("ln_nt", nt)
        m.set_option("gemm_order", order)   # the persistent GEMM's tile order (0 = row-major, default 4)
        assert np.array_equal(m.forward(px).view(np.uint32), ref.view(np.uint32)), (rows_, nt, order)
    # the row pitch of q|k|v (padded by default so that a head's pieces spread over the memory channels; 0 = the dense
    # rows of rounds 1-4) and the pair a workgroup of the persistent attention starts on: layouts and orders, not arithmetic.
    # 40 and 41 images: whole and ragged halves; a grow-and-shrink sequence of the pitch on ONE handle (it re-sizes the
    # activation sets); the CLS-only last layer scatters its query rows into the padded rows as well
    px41 = synth.preprocess_rgb8(synth.images_u8(79, 41, cfg.image))
    ref41 = m.forward(px41)
    for pad, order in ((0, 0), (192, 1), (64, 0), (0, 1), (1024, 1), (128, 1)):
        m.set_option("qkv_pad", pad)
        m.set_option("attn_order", order)
        assert np.array_equal(m.forward(px).view(np.uint32), ref.view(np.uint32)), (pad, order)
        assert np.array_equal(m.forward(px41).view(np.uint32), ref41.view(np.uint32)), (pad, order)
    # q|k|v as head-major planes, written so by the q/k/v GEMM's epilogue and by the last layer's K|V launch and query
    # scatter (option "qkv_layout"): other addresses, the same values
    for layout, order, split in ((1, 1, 1), (1, 0, 0), (0, 1, 1), (1, 1, 1)):
        m.set_option("qkv_layout", layout)
        m.set_option("attn_order", order)
        m.set_option("split_tail", split)
        m.set_option("attn_nt", split)   # nt or default cache policy on attention's K / V / q stream
        m.set_option("store_nt", order)  # ... and on the persistent GEMM's q|k|v / h stores (default 1)
        assert np.array_equal(m.forward(px).view(np.uint32), ref.view(np.uint32)), ("layout", layout, order, split)
        assert np.array_equal(m.forward(px41).view(np.uint32), ref41.view(np.uint32)), ("layout", layout, order, split)
        assert np.array_equal(m.forward(px41[:3]).view(np.uint32), ref41[:3].view(np.uint32)), ("layout, one stream", layout)
    m.set_option("full_last", 1)
    assert np.array_equal(m.forward(px41).view(np.uint32), ref41.view(np.uint32))
    m.set_option("attn_nt", 0)
    m.set_option("store_nt", 0)
    assert np.array_equal(m.forward(px41).view(np.uint32), ref41.view(np.uint32))
    m.set_option("attn_nt", 1)
    m.set_option("store_nt", 1)
    m.set_option("qkv_layout", 0)
    m.set_option("qkv_pad", 64)
    assert np.array_equal(m.forward(px41).view(np.uint32), ref41.view(np.uint32))
    with pytest.raises(Exception):
        m.set_option("qkv_layout", 2)
    with pytest.raises(Exception):
        m.set_option("qkv_pad", 32)    # 128-byte row segments of the GEMM epilogue: multiples of 64 elements only
    with pytest.raises(Exception):
        m.set_option("attn_order", 2)
    m.close()


def test_clock_probe_reads_a_plausible_shader_clock(built):
    from image_search_amd._lib import check, lib
    v = ctypes.c_float()
    check(lib().mi_op_clock_probe(0, None, ctypes.byref(v)))
    assert 300.0 < v.value < 3500.0, v.value


@pytest.mark.parametrize("prec,ln_fold", [(PRECISION_F32, 0), (PRECISION_BF16, 1), (PRECISION_BF16, 0)])
def test_cls_only_last_layer_is_bit_identical_to_the_full_one(l14, monkeypatch, prec, ln_fold):
    """Behind the last layer's attention only the CLS row is live; computing just that row must give
    the very bits of the full last layer (same per-row arithmetic), for one and for two half-chunks."""
    cfg, w, path, u8, g = l14
    px = synth.preprocess_rgb8(synth.images_u8(77, 40, cfg.image))      # 40 images: two half-chunk streams in bf16
    m = Model.from_file(path, 0, prec)
    if prec == PRECISION_BF16:
        m.set_option("ln_fold", ln_fold)
    fast = m.forward(px)
    m.set_option("full_last", 1)
    full = m.forward(px)
    assert np.array_equal(fast.view(np.uint32), full.view(np.uint32))
