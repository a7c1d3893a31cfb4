"""The handles when what they own comes and goes: a tower's workspace regrown and rebuilt, its upload buffers regrown, a
captured text query dropped with the buffers it names, a pipeline's lane and slot buffers regrown, and every handle closed and
made again many times over.  Each owner frees what it took when its handle closes; what a test can see of that is that nothing
computed changes by a bit from step to step and from cycle to cycle, and that a load which fails leaves a process in which the
next load works.  (Free device memory is not asserted: the figure is device-wide, and the devices are shared.)"""
import ctypes

import numpy as np
import pytest

from image_search_amd import synth
from image_search_amd.clip import PRECISION_BF16, Model, TextModel
from image_search_amd.search import EmbeddingTable, Pipeline
from oracle import vit_numpy

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def tiny(built, tmp_path_factory):
    cfg = synth.VitConfig.tiny()
    path = str(tmp_path_factory.mktemp("handles") / "tiny.safetensors")
    synth.save_safetensors(synth.vit_weights(cfg, 5), path, {"num_attention_heads": cfg.heads})
    px = synth.preprocess_rgb8(synth.images_u8(41, 72, cfg.image))
    return cfg, path, px


def test_image_tower_ten_load_close_cycles(tiny):
    cfg, path, px = tiny
    small, large = synth.photo_u8(7, 37, 53), synth.photo_u8(8, 300, 401)
    first = None
    for cycle in range(10):
        m = Model.from_file(path, 0, PRECISION_BF16)
        try:
            one = m.forward(px[:1])
            three = m.forward(px[:3])                     # the workspace regrows
            assert same_bits(three[:1], one)
            for key, value in (("parts", 1), ("parts", 2), ("qkv_pad", 64), ("qkv_pad", 128)):
                m.set_option(key, value)                  # the workspace is dropped and rebuilt by the next forward
                assert same_bits(m.forward(px[:3]), three), (cycle, key, value)
            a = m.forward_images([small])
            b = m.forward_images([large])                 # the source and intermediate buffers regrow
            assert same_bits(m.forward_images([small]), a)
            assert same_bits(m.forward_images([large, small]), np.concatenate([b, a]))
            assert same_bits(m.forward(px[:3]), three)
            if first is None:
                first = (three, a, b)
            assert same_bits(three, first[0]) and same_bits(a, first[1]) and same_bits(b, first[2]), cycle
        finally:
            m.close()


def test_text_graph_goes_with_the_workspace_it_names(built, tmp_path):
    """One bf16 query on the skinny-GEMM path (hidden 768, ff 3072: the only geometry that path and its captured graph are built
    for; two layers) — eager, captured, replayed — around everything that must drop the graph.  "text_fuse" 0 is
    another rounding sequence of the same graph: inside the bounds tests/test_vit_gpu.py holds it to (3e-2 * rms against the
    fp64 reference, 2e-2 * rms against the fused form)."""
    cfg = synth.TextConfig(hidden=768, layers=2, heads=12, ff=3072, vocab=1000, positions=77, proj=64)
    w = synth.vit_weights(cfg, 6)
    path = str(tmp_path / "text.safetensors")
    synth.save_safetensors(w, path, {"num_attention_heads": cfg.heads})
    ids = synth.token_ids(cfg, 29, 3)
    ref = vit_numpy.text_forward(w, cfg, ids[:1], np.float64)
    rms = float(np.sqrt((ref ** 2).mean()))
    m = TextModel.from_file(path, 0, PRECISION_BF16)
    try:
        first = m.embed(ids[:1])                                   # eager
        assert float(np.abs(first - ref).max() / rms) <= 3e-2
        for _ in range(2):
            assert same_bits(m.embed(ids[:1]), first)              # captured, replayed
        batch = m.embed(ids)                                       # the workspace regrows: the graph must go
        assert batch.shape == (3, cfg.proj) and np.isfinite(batch).all()
        for _ in range(3):
            assert same_bits(m.embed(ids[:1]), first)              # eager, captured and replayed on the new buffers
        m.set_option("text_fuse", 0)
        two = m.embed(ids[:1])
        print(f"text_fuse 0: max|err|/rms = {float(np.abs(two - ref).max() / rms):.2e} (fp64), "
              f"{float(np.abs(two - first).max() / rms):.2e} (fused form)")
        assert float(np.abs(two - ref).max() / rms) <= 3e-2 and float(np.abs(two - first).max() / rms) <= 2e-2
        m.set_option("text_fuse", 1)
        assert same_bits(m.embed(ids[:1]), first)
    finally:
        m.close()


def test_pipeline_five_create_free_cycles(tiny):
    cfg, path, px = tiny
    m = Model.from_file(path, 0, PRECISION_BF16)
    ref = EmbeddingTable(cfg.proj)
    try:
        rows = np.concatenate([m.forward(px[:2]), m.forward(px[2:72])])   # the batches the pipeline will run
        ref.insert(rows)
        want = {k: ref.knn(rows[5], k) for k in (3, 70)}
        for cycle in range(5):
            t = EmbeddingTable(cfg.proj)
            p = Pipeline(m, t)
            try:
                assert p.ingest(px[:2]) == 0
                assert p.ingest(px[2:72]) == 2             # the lane's upload buffers regrow
                # 16 queries fill the ring of query slots, each with room for 64 results; the 17th comes back to the first slot
                # with k = 70: that slot's result buffers regrow, and the 18th runs on a slot that did not
                got = [(k, p.query(rows[5], k)) for k in [3] * 16 + [70, 3]]
                p.sync()
                assert len(t) == 72
                for k, (idx, dist) in got:
                    assert np.array_equal(idx, want[k][0]) and same_bits(dist, want[k][1]), (cycle, k)
            finally:
                p.close()
                t.close()
    finally:
        ref.close()
        m.close()


def test_a_failed_load_leaves_nothing_in_the_way(tiny, mi, tmp_path):
    cfg, path, px = tiny
    m = Model.from_file(path, 0, PRECISION_BF16)
    before = m.forward(px[:3])
    m.close()
    bad = tmp_path / "bad.safetensors"
    bad.write_bytes(b"\x10\x00\x00\x00\x00\x00\x00\x00{\"a\":1}        ")   # the inputs of test_load_errors_are_codes
    h = ctypes.c_void_p()
    for load in (mi.mi_clip_load, mi.mi_clip_load_text):
        for _ in range(3):
            assert load(b"/nonexistent/x.safetensors", 0, 1, ctypes.byref(h)) == -2 and not h.value
            assert load(str(bad).encode(), 0, 1, ctypes.byref(h)) == -2 and not h.value
    # a file that fails AFTER most of the weights were uploaded: the last layer lacks its last tensor
    w = synth.vit_weights(cfg, 5)
    del w[f"vision_model.encoder.layers.{cfg.layers - 1}.mlp.fc2.bias"]
    cut = str(tmp_path / "cut.safetensors")
    synth.save_safetensors(w, cut, {"num_attention_heads": cfg.heads})
    assert mi.mi_clip_load(cut.encode(), 0, 1, ctypes.byref(h)) != 0 and not h.value
    m = Model.from_file(path, 0, PRECISION_BF16)
    try:
        assert same_bits(m.forward(px[:3]), before)
    finally:
        m.close()
