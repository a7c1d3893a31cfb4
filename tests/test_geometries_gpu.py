"""The towers at every geometry the loader accepts, not only ViT-L/14: two layers each, on a real MI355X through the C ABI.

include/mi355clip.h promises that a checkpoint with head_dim 64, hidden size 128 .. 1664 and up to 288 tokens loads AND runs.
The other suites forward image towers at hidden 128 / 256 / 768 (17 tokens) and 1024 (257 tokens), all with patch 14; here:

  name    hidden heads   ff  patch image proj tokens   what only this geometry reaches
  p32       768    12  3072    32   224  512     50    im2col_kernel<bf16> (the LDS gather does not fit), a 7 x 7 grid,
                                                       attn_bf16_kernel<64,50> on dense token rows, attn_f32_mfma_kernel<80>
  p16       768    12  3072    16   224  512    197    im2col_rows_kernel with Kp == K, attn32_bf16_kernel<224,197>, the CLS-only
                                                       last layer at S = 197, attn_f32_mfma_kernel<208> (and <208,true> in BF16X3)
  w1280    1280    20  5120    14   224 1024    257    LayerNorm NT = 5, 40 sum blocks per row (ln_stats_kernel's second trip),
                                                       15- and 20-tile GEMM rows, 80 K tiles
  w384      384     6  1536    16    64   96     17    LayerNorm VEC = 2, NT = 3; no LayerNorm-free loop, no BF16X3
  w512      512     8  2048    14    56  128     17    LayerNorm NT = 2
  w1536    1536    24  6144    14    56  128     17    LayerNorm NT = 6, 48 sum blocks per row
  w1664    1664    26  6656    14    56  128     17    LayerNorm VEC = 2, NT = 13 (head_kernel: 53 KB of static LDS); no ln_fold

and text towers of hidden 512 and 1280.  Configurations are named by shape, not by model: ViT-H/14 has 16 heads of 80 and is
refused at load (tests/test_weights_gpu.py).

The reference of every tower is oracle/vit_numpy.py on synth.vit_weights, itself pinned to the transformers goldens by
tests/test_oracle.py.  fp32 and MI_PRECISION_BF16X3: the project's parity bar, 1e-4 (close()).  bf16: the project's stated
bound, max |err| / rms <= 3e-2, which two layers sit far inside — the sharp part there is the set of identities, compared by
bits: everything that only moves bytes differently (tile order, row pitch, plane layout, chunking, the CLS-only last layer)
must return the very same embedding.
"""
import numpy as np
import pytest

from image_search_amd import synth
from image_search_amd._lib import MiError
from image_search_amd.clip import PRECISION_BF16, PRECISION_BF16X3, PRECISION_F32, Model, TextModel
from oracle import vit_numpy

pytestmark = pytest.mark.gpu

MI_ERR_UNSUPPORTED = -5

IMAGE_GEOMETRIES = {
    "p32": dict(hidden=768, heads=12, ff=3072, patch=32, image=224, proj=512),
    "p16": dict(hidden=768, heads=12, ff=3072, patch=16, image=224, proj=512),
    "w1280": dict(hidden=1280, heads=20, ff=5120, patch=14, image=224, proj=1024),
    "w384": dict(hidden=384, heads=6, ff=1536, patch=16, image=64, proj=96),
    "w512": dict(hidden=512, heads=8, ff=2048, patch=14, image=56, proj=128),
    "w1536": dict(hidden=1536, heads=24, ff=6144, patch=14, image=56, proj=128),
    "w1664": dict(hidden=1664, heads=26, ff=6656, patch=14, image=56, proj=128),
}
TOKENS = {"p32": 50, "p16": 197, "w1280": 257, "w384": 17, "w512": 17, "w1536": 17, "w1664": 17}
TEXT_GEOMETRIES = {
    "t512": dict(hidden=512, heads=8, ff=2048, vocab=2000, positions=77, proj=512),
    "t1280": dict(hidden=1280, heads=20, ff=5120, vocab=2000, positions=77, proj=1280),
}
LAYERS = 2


def close(out, ref, tol):
    rms = float(np.sqrt((np.asarray(ref, np.float64) ** 2).mean()))
    return np.allclose(out, ref, rtol=tol, atol=tol * rms), float(np.abs(out - ref).max() / rms)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Geometry:
    pass


@pytest.fixture(scope="module", params=list(IMAGE_GEOMETRIES))
def geom(built, tmp_path_factory, request):
    """Weights written once per geometry; 40 images (two half-chunk streams in bf16), the first 3 of them with both oracles."""
    g = Geometry()
    g.name = request.param
    g.cfg = synth.VitConfig(layers=LAYERS, **IMAGE_GEOMETRIES[g.name])
    assert g.cfg.tokens == TOKENS[g.name] and g.cfg.head_dim == 64
    g.w = synth.vit_weights(g.cfg, 17)
    g.path = str(tmp_path_factory.mktemp("geom") / f"{g.name}.safetensors")
    synth.save_safetensors(g.w, g.path, {"num_attention_heads": g.cfg.heads})
    g.px40 = synth.preprocess_rgb8(synth.images_u8(303, 40, g.cfg.image))
    g.px3 = g.px40[:3]
    g.ref64 = vit_numpy.vit_forward(g.w, g.cfg, g.px3, np.float64)
    g.ref32 = vit_numpy.vit_forward(g.w, g.cfg, g.px3, np.float32)
    # what the loader decides from the shapes (vit.hip: fold_ready, attn32_applies, the BF16X3 check of load_weights)
    g.tiles256 = g.cfg.hidden % 256 == 0 and g.cfg.ff % 256 == 0
    g.attn32 = 64 < g.cfg.tokens <= 288
    return g


# ---- fp32: the parity path ---------------------------------------------------------------------------------------------

def test_fp32_tower_meets_the_parity_bar(geom):
    g = geom
    m = Model.from_file(g.path, 0, PRECISION_F32)
    c = g.cfg
    assert (m.image, m.patch, m.tokens, m.hidden, m.layers, m.heads, m.ff, m.proj) == \
        (c.image, c.patch, c.tokens, c.hidden, LAYERS, c.heads, c.ff, c.proj)
    out = m.forward(g.px3)
    ok32, e32 = close(out, g.ref32, 1e-4)
    ok64, e64 = close(out, g.ref64, 1e-4)
    print(f"{g.name} fp32: max|err|/rms = {e32:.2e} (fp32 oracle), {e64:.2e} (fp64 oracle)")
    assert ok32, e32
    assert ok64, e64
    assert same_bits(m.forward(g.px3[1:2]), out[1:2])            # batch-independent, deterministic
    m.set_option("full_last", 1)                                 # the CLS-only last layer against the full one
    assert same_bits(m.forward(g.px3), out)
    m.set_option("full_last", 0)
    m.set_option("attn_f32_mfma", 0)                             # one thread per query instead of the matrix pipe
    old = m.forward(g.px3)
    ok32, e32 = close(old, g.ref32, 1e-4)
    ok64, e64 = close(old, g.ref64, 1e-4)
    print(f"{g.name} fp32, attn_f32_mfma = 0: max|err|/rms = {e32:.2e} (fp32 oracle), {e64:.2e} (fp64 oracle)")
    assert ok32, e32
    assert ok64, e64
    m.set_option("full_last", 1)
    assert same_bits(m.forward(g.px3), old)
    m.close()


# ---- bf16: the bound, and the identities by bits ----------------------------------------------------------------------

def _looked_at(g, n):
    return n * g.cfg.tokens * (1 + 2 * (LAYERS - 1))   # the embedding's statistics + two per LayerNorm-free layer


@pytest.mark.parametrize("ln_fold", [1, 0], ids=["ln_fold", "layernorm"])
def test_bf16_tower_bound_and_identities(geom, ln_fold):
    g = geom
    m = Model.from_file(g.path, 0, PRECISION_BF16)
    if ln_fold and not g.tiles256:
        # hidden 384 / 1664: no 256-wide tiles, so no LayerNorm-free loop — the option is refused and the handle still forwards
        base = m.forward(g.px3)
        with pytest.raises(MiError) as e:
            m.set_option("ln_fold", 1)
        assert e.value.code == MI_ERR_UNSUPPORTED
        assert m.ln_fold_stats() == (0, 0)
        assert same_bits(m.forward(g.px3), base)
        err = float(np.abs(base - g.ref64).max() / np.sqrt((g.ref64 ** 2).mean()))
        assert err <= 3e-2, err
        m.close()
        return
    m.set_option("ln_fold", ln_fold)
    assert m.ln_fold_stats() == (0, 0)
    out3 = m.forward(g.px3)
    assert m.ln_fold_stats(reset=True) == ((0, _looked_at(g, 3)) if ln_fold else (0, 0))
    err = float(np.abs(out3 - g.ref64).max() / np.sqrt((g.ref64 ** 2).mean()))
    print(f"{g.name} bf16, ln_fold = {ln_fold}: max|err|/rms = {err:.2e} (fp64 oracle, {LAYERS} layers)")
    assert np.isfinite(out3).all()
    assert err <= 3e-2, err
    out40 = m.forward(g.px40)                                     # two half-chunk streams
    assert m.ln_fold_stats(reset=True) == ((0, _looked_at(g, 40)) if ln_fold else (0, 0))
    assert np.isfinite(out40).all()
    # a row must not depend on its batch: one image, a one-stream batch and the two-stream batch
    assert same_bits(out40[:3], out3)
    assert same_bits(m.forward(g.px40[:1]), out40[:1])
    assert same_bits(m.forward(g.px40[:7]), out40[:7])

    def unchanged(what):
        assert same_bits(m.forward(g.px40), out40), (g.name, ln_fold, what, "40 images")
        assert same_bits(m.forward(g.px3), out3), (g.name, ln_fold, what, "3 images")

    # bytes move differently, bits do not: (option, the other value, the default)
    for key, other, default in (("full_last", 1, 0), ("im2col_rows", 0, 1), ("gemm_order", 0, 4), ("split_tail", 0, 1),
                                ("parts", 1, 2)):
        m.set_option(key, other)
        unchanged((key, other))
        m.set_option(key, default)
    unchanged("defaults restored")
    if g.attn32:
        # the row pitch of q|k|v, head-major planes and the pair a workgroup of the persistent attention starts on
        for pad in (0, 64, 128):
            m.set_option("qkv_pad", pad)
            unchanged(("qkv_pad", pad))
        for layout, order, pad in ((1, 1, 128), (1, 0, 0), (0, 0, 64), (1, 1, 64)):
            m.set_option("qkv_layout", layout)
            m.set_option("attn_order", order)
            m.set_option("qkv_pad", pad)
            unchanged(("qkv_layout", layout, "attn_order", order, "qkv_pad", pad))
        m.set_option("full_last", 1)                              # the last layer's query scatter into planes / padded rows
        unchanged(("qkv_layout", 1, "full_last", 1))
        m.set_option("full_last", 0)
        m.set_option("qkv_layout", 0)
        m.set_option("attn_order", 1)
        m.set_option("qkv_pad", 128)
        unchanged("attention defaults restored")
    if ln_fold:
        # the planes carry NaN / Inf patterns through encode and decode; nothing of a poisoned image reaches another one
        m.ln_fold_stats(reset=True)
        bad = g.px40.copy()
        bad[3, 1, 20, 20] = np.nan
        bad[25, 0, 5, 7] = np.inf
        out = m.forward(bad)
        assert np.isnan(out[3]).all() and np.isnan(out[25]).all()
        keep = [i for i in range(40) if i not in (3, 25)]
        assert same_bits(out[keep], out40[keep])
    m.close()


# ---- MI_PRECISION_BF16X3 --------------------------------------------------------------------------------------------------

def test_bf16x3_tower_meets_the_parity_bar_or_is_refused_at_load(geom):
    """The three-pass GEMM is the persistent 256 x 256 kernel only: a geometry without 256-wide tiles is refused when the
    file is read (never at the first forward); every other one runs at the fp32 tower's bar."""
    g = geom
    if not g.tiles256:
        with pytest.raises(MiError) as e:
            Model.from_file(g.path, 0, PRECISION_BF16X3)
        assert e.value.code == MI_ERR_UNSUPPORTED and "256" in str(e.value), str(e.value)
        return
    m = Model.from_file(g.path, 0, PRECISION_BF16X3)
    out = m.forward(g.px3)
    ok, err = close(out, g.ref64, 1e-4)
    print(f"{g.name} bf16x3: max|err|/rms = {err:.2e} (fp64 oracle)")
    assert ok, err
    assert same_bits(m.forward(g.px3[1:2]), out[1:2])
    m.set_option("full_last", 1)
    assert same_bits(m.forward(g.px3), out)
    m.close()


# ---- text towers ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=list(TEXT_GEOMETRIES))
def text(built, tmp_path_factory, request):
    g = Geometry()
    g.name = request.param
    g.cfg = synth.TextConfig(layers=LAYERS, **TEXT_GEOMETRIES[g.name])
    g.w = synth.vit_weights(g.cfg, 19)
    g.path = str(tmp_path_factory.mktemp("text") / f"{g.name}.safetensors")
    synth.save_safetensors(g.w, g.path, {"num_attention_heads": g.cfg.heads})
    g.ids = synth.token_ids(g.cfg, 23, 3)
    g.cut = g.ids.copy()                      # tokens behind the EOS: must not reach the pooled row
    for i in range(g.cut.shape[0]):
        g.cut[i, int(g.cut[i].argmax()) + 1:] = 0
    assert not np.array_equal(g.cut, g.ids)
    g.ref64 = vit_numpy.text_forward(g.w, g.cfg, g.ids, np.float64)
    g.ref32 = vit_numpy.text_forward(g.w, g.cfg, g.ids, np.float32)
    return g


def _text_identities(g, m, out):
    assert same_bits(m.embed(g.cut), out)                                        # causal
    assert m.embed(g.ids[:0]).shape == (0, g.cfg.proj)
    assert same_bits(m.embed(np.concatenate([g.ids] * 3))[-g.ids.shape[0]:], out)
    # one sequence: at these widths there is no skinny-GEMM path, so the batched kernels run whatever "text_fast" says
    for fast in (1, 0, 1):
        m.set_option("text_fast", fast)
        for i in range(g.ids.shape[0]):
            assert same_bits(m.embed(g.ids[i:i + 1]), out[i:i + 1]), (g.name, "text_fast", fast, i)


def test_text_tower_fp32_meets_the_parity_bar(text):
    g = text
    m = TextModel.from_file(g.path)
    assert (m.positions, m.hidden, m.layers, m.heads, m.ff, m.proj) == \
        (g.cfg.positions, g.cfg.hidden, LAYERS, g.cfg.heads, g.cfg.ff, g.cfg.proj)
    out = m.embed(g.ids)
    ok32, e32 = close(out, g.ref32, 1e-4)
    ok64, e64 = close(out, g.ref64, 1e-4)
    print(f"text {g.name} fp32: max|err|/rms = {e32:.2e} (fp32 oracle), {e64:.2e} (fp64 oracle)")
    assert ok32, e32
    assert ok64, e64
    _text_identities(g, m, out)
    m.close()


def test_text_tower_bf16_within_the_bf16_bound(text):
    g = text
    m = TextModel.from_file(g.path, 0, PRECISION_BF16)
    out = m.embed(g.ids)
    err = float(np.abs(out - g.ref64).max() / np.sqrt((g.ref64 ** 2).mean()))
    print(f"text {g.name} bf16: max|err|/rms = {err:.2e} (fp64 oracle, {LAYERS} layers)")
    assert np.isfinite(out).all()
    assert err <= 3e-2, err
    _text_identities(g, m, out)
    m.close()
