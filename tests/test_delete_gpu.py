"""Deleted rows (mi_knn_delete, mi_knn_sharded_delete, mi_index_remove) on a real MI355X: every search path treats a
deleted row as absent.  The oracle is orc_knn over the LIVE rows, each result ordinal mapped back to its id
(live_ids[ordinal]: ids are monotone in the ordinal, so ties keep their order).  Bar: bit-exact ids and distance bits."""
import os

import numpy as np
import pytest

from image_search_amd import synth
from image_search_amd._lib import MiError
from image_search_amd.search import EmbeddingTable, ImageIndex, ShardedTable, embed_all_images_in_dir
from oracle.binding import orc_knn

pytestmark = pytest.mark.gpu
NO_ID = 0xFFFFFFFFFFFFFFFF


def _oracle(orc, q, rows, dead, k):
    """the answer of a table that never held the rows `dead`"""
    live = np.setdiff1d(np.arange(rows.shape[0], dtype=np.uint64), np.asarray(dead, np.uint64))
    oi, od = orc_knn(orc, q, rows[live.astype(np.int64)], k)
    ids = np.full(k, NO_ID, np.uint64)
    m = oi != NO_ID
    ids[m] = live[oi[m].astype(np.int64)]
    return ids, od


def _same(got, want, what=""):
    gi, gd = got
    oi, od = want
    assert np.array_equal(gi, oi), (what, np.nonzero(gi != oi)[0][:5])
    assert np.array_equal(gd.view(np.uint32), od.view(np.uint32)), what


KS = [1, 10, 64, 65, 256, 1000, 1024, 1500, 2500]
N1 = 100_000


@pytest.mark.parametrize("pattern", ["random1pct", "tile", "ends", "topk"])
def test_single_pass_and_select_leave_deleted_rows_out(built, orc, pattern):
    rows = synth.corpus_rows(12, 0, N1)
    qs = synth.corpus_rows(1012, 0, 2)
    t = EmbeddingTable(768, 0)
    t.insert_synthetic(12, 0, N1)
    rng = np.random.default_rng(5)
    if pattern == "random1pct":
        dead = rng.choice(N1, N1 // 100, replace=False)
    elif pattern == "tile":
        dead = np.arange(64 * 700, 64 * 701)
    elif pattern == "ends":
        dead = np.array([0, N1 - 1])
    else:  # the unfiltered top-k of both queries: the threshold has to move
        dead = np.union1d(orc_knn(orc, qs[0], rows, 2500)[0], orc_knn(orc, qs[1], rows, 2500)[0])
    dead = np.unique(dead.astype(np.uint64))
    assert t.delete(dead) == dead.size
    assert np.array_equal(t.deleted(), dead)
    assert len(t) == N1                                      # ids and storage stay
    assert np.array_equal(t.rows(int(dead[0]), 1), rows[int(dead[0])][None])
    for k in KS:
        for u in range(2):
            _same(t.knn(qs[u], k), _oracle(orc, qs[u], rows, dead, k), (pattern, k, u))
    t.close()


def test_chained_lds_passes_and_fp32_groups(built, orc, monkeypatch):
    """the per-wave LDS lists (MI_KNN_SELECT=0 at creation), the chained passes for k > 1024, and the fp32 groups of 2/4/8"""
    import torch
    rows = synth.corpus_rows(13, 0, N1)
    qs = synth.corpus_rows(1013, 0, 8)
    dead = np.union1d(orc_knn(orc, qs[0], rows, 5000)[0], np.arange(0, N1, 97, dtype=np.uint64))
    monkeypatch.setenv("MI_KNN_SELECT", "0")
    t = EmbeddingTable(768, 0)
    monkeypatch.delenv("MI_KNN_SELECT")
    t.insert_synthetic(13, 0, N1)
    t.delete(dead)
    for k in (100, 1000, 1500, 5000):
        _same(t.knn(qs[0], k), _oracle(orc, qs[0], rows, dead, k), k)
    want = [_oracle(orc, q, rows, dead, 10) for q in qs]
    gi, gd = t.knn(qs, 10)                                   # mi_knn_search: groups of 8 / 4 / 2 over the fp32 rows
    for u in range(8):
        _same((gi[u], gd[u]), want[u], u)
    d_q = torch.from_numpy(qs).cuda()
    for nq in (2, 5, 8):
        d_i = torch.zeros((nq, 10), dtype=torch.int64, device="cuda")
        d_d = torch.zeros((nq, 10), dtype=torch.float32, device="cuda")
        t.knn_device(d_q.data_ptr(), nq, 10, d_i.data_ptr(), d_d.data_ptr(), torch.cuda.current_stream().cuda_stream, batched=True)
        torch.cuda.synchronize()
        for u in range(nq):
            _same((d_i.cpu().numpy()[u].view(np.uint64), d_d.cpu().numpy()[u]), want[u], (nq, u))
    t.close()


def test_edge_cases(built, orc):
    n = 3000
    rows = synth.corpus_rows(21, 0, n)
    rows[100:110] = 0.0                                       # zero-norm rows: NaN distances, ranked last
    q = synth.corpus_rows(1021, 0, 1)[0]
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    dead = np.array([100, 101, 102, 5, 2999], np.uint64)      # three of the zero rows deleted, seven stay
    assert t.delete(dead) == 5
    assert t.delete(dead[:2]) == 0                            # idempotent
    assert t.delete(np.array([5, 6], np.uint64)) == 1
    dead = np.union1d(dead, [6]).astype(np.uint64)
    assert np.array_equal(t.deleted(), dead)
    with pytest.raises(MiError) as e:
        t.delete(np.array([7, n], np.uint64))                 # one id out of range: nothing changes
    assert e.value.code == -1
    assert np.array_equal(t.deleted(), dead)
    for k in (10, 64, 2990, 2994, 3000, 4000):                # the live NaN rows at the tail, then the padding
        _same(t.knn(q, k), _oracle(orc, q, rows, dead, k), k)
    gi, gd = t.knn(q, 3000)
    assert set(range(103, 110)) <= set(int(i) for i in gi) and not set(int(i) for i in dead) & set(int(i) for i in gi)
    assert t.delete(np.arange(n, dtype=np.uint64)) == n - dead.size
    for k in (1, 64, 1000, 5000):
        gi, gd = t.knn(q, k)
        assert (gi == NO_ID).all() and np.isinf(gd).all()
    t.close()


N2 = 300_000   # above the 2^18 rows of the two-stage search


@pytest.fixture(scope="module")
def big(built, orc):
    rows = synth.corpus_rows(31, 0, N2)
    qs = np.concatenate([rows[[777, 123_456]], synth.corpus_rows(1031, 0, 14)])
    dead = set()
    for q in qs[:4]:
        dead.update(int(i) for i in orc_knn(orc, q, rows, 1000)[0])
    dead = np.array(sorted(dead | set(range(0, N2, 101))), np.uint64)
    want = {k: [_oracle(orc, q, rows, dead, k) for q in qs] for k in (10, 64, 1000)}
    return rows, qs, dead, want


@pytest.mark.parametrize("prefilter", [1, 2])
def test_two_stage_search_leaves_deleted_rows_out(big, prefilter):
    rows, qs, dead, want = big
    t = EmbeddingTable(768, 0)
    t.insert_synthetic(31, 0, N2)
    t.delete(dead)
    t.set_option("prefilter", prefilter)
    t.set_option("prefilter_adaptive", 0)
    for sample in (0, 1, 2):
        t.set_option("prefilter_sample", sample)
        for k in (10, 64, 1000):
            for u in range(4):
                _same(t.knn(qs[u], k), want[k][u], (prefilter, sample, k, u))
                cand, fell_back = t.prefilter_stats()
                assert cand > 0 and not fell_back, (cand, fell_back)
    t.close()


def test_groups_over_the_byte_mirror_and_the_fp32_rows(big):
    import torch
    rows, qs, dead, want = big
    t = EmbeddingTable(768, 0)
    t.insert_synthetic(31, 0, N2)
    t.delete(dead)
    d_q = torch.from_numpy(qs).cuda()
    for prefilter, stage1 in ((2, 1), (2, 0), (0, 1)):
        t.set_option("prefilter", prefilter)
        t.set_option("prefilter_adaptive", 0)
        t.set_option("batch_stage1", stage1)
        for k in (10, 64):
            singles = [t.knn(q, k) for q in qs]
            for nq in (2, 5, 8, 16):
                d_i = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
                d_d = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
                t.knn_device(d_q.data_ptr(), nq, k, d_i.data_ptr(), d_d.data_ptr(), torch.cuda.current_stream().cuda_stream,
                             batched=True)
                torch.cuda.synchronize()
                for u in range(nq):
                    got = (d_i.cpu().numpy()[u].view(np.uint64), d_d.cpu().numpy()[u])
                    _same(got, want[k][u], (prefilter, stage1, k, nq, u))
                    _same(got, singles[u], (prefilter, stage1, k, nq, u))
    t.close()


def test_delete_is_ordered_like_any_call_on_the_handle(built, orc):
    import torch
    n = 20_000
    rows = synth.corpus_rows(41, 0, n)
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    q = rows[4321]
    d_q = torch.from_numpy(q[None].copy()).cuda()
    s = torch.cuda.Stream()
    a_i = torch.zeros((1, 5), dtype=torch.int64, device="cuda"); a_d = torch.zeros((1, 5), dtype=torch.float32, device="cuda")
    b_i = torch.zeros_like(a_i); b_d = torch.zeros_like(a_d)
    with torch.cuda.stream(s):
        t.knn_device(d_q.data_ptr(), 1, 5, a_i.data_ptr(), a_d.data_ptr(), s.cuda_stream)
        t.delete([4321])
        t.knn_device(d_q.data_ptr(), 1, 5, b_i.data_ptr(), b_d.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert int(a_i.cpu()[0, 0]) == 4321                     # enqueued before: may (here: does) see the row
    assert 4321 not in [int(i) for i in b_i.cpu().numpy()[0].view(np.uint64)]
    _same((b_i.cpu().numpy()[0].view(np.uint64), b_d.cpu().numpy()[0]), _oracle(orc, q, rows, [4321], 5))
    more = synth.corpus_rows(42, 0, 100)
    t.insert(more)                                           # an append after a delete continues the ids
    assert len(t) == n + 100
    all_rows = np.concatenate([rows, more])
    _same(t.knn(more[7], 10), _oracle(orc, more[7], all_rows, [4321], 10))
    assert int(t.knn(more[7], 1)[0][0]) == n + 7
    t.close()


def test_persistence(built, orc, tmp_path):
    n = 5000
    rows = synth.corpus_rows(51, 0, n)
    q = synth.corpus_rows(1051, 0, 1)[0]
    t = EmbeddingTable(768, 0)
    t.insert(rows)
    p1 = str(tmp_path / "plain.miknn")
    from image_search_amd._lib import check, lib
    check(lib().mi_knn_save(t._h, p1.encode()))
    assert os.path.getsize(p1) == 32 + n * 768 * 4 and open(p1, "rb").read(8) == b"MIKNNv01"
    dead = np.array([3, 64, 65, 4999] + list(orc_knn(orc, q, rows, 20)[0]), np.uint64)
    dead = np.unique(dead)
    t.delete(dead)
    p2 = str(tmp_path / "dead.miknn")
    check(lib().mi_knn_save(t._h, p2.encode()))
    assert open(p2, "rb").read(8) == b"MIKNNv02" and os.path.getsize(p2) == 32 + n * 768 * 4 + 8 + 8 * dead.size
    u = EmbeddingTable(768, 0)
    check(lib().mi_knn_load(u._h, p2.encode()))
    assert np.array_equal(u.deleted(), dead) and len(u) == n
    for k in (10, 1000):
        _same(u.knn(q, k), _oracle(orc, q, rows, dead, k), k)
    # a file that continues a non-empty table's ids
    w = EmbeddingTable(768, 0, base=n)
    w.insert(rows[:1000])
    w.delete([n + 10])
    p3 = str(tmp_path / "cont.miknn")
    check(lib().mi_knn_save(w._h, p3.encode()))
    check(lib().mi_knn_load(u._h, p3.encode()))
    assert np.array_equal(u.deleted(), np.append(dead, n + 10).astype(np.uint64))
    both = np.concatenate([rows, rows[:1000]])
    _same(u.knn(q, 50), _oracle(orc, q, both, list(dead) + [n + 10], 50))
    for h in (t, u, w):
        h.close()


def test_sharded_tables(built, orc, tmp_path):
    n = 30_000
    rows = synth.corpus_rows(61, 0, n)
    qs = synth.corpus_rows(1061, 0, 3)
    rng = np.random.default_rng(61)
    dead = np.unique(np.concatenate([rng.choice(n, 500, replace=False), orc_knn(orc, qs[0], rows, 100)[0]]).astype(np.uint64))
    one = EmbeddingTable(768, 0)
    one.insert(rows)
    one.delete(dead)
    want = {k: one.knn(qs, k) for k in (10, 1000)}
    for k in (10, 1000):
        for u in range(3):
            _same((want[k][0][u], want[k][1][u]), _oracle(orc, qs[u], rows, dead, k), (k, u))
    prefix = str(tmp_path / "sh")
    for n_sh, block in ((1, 0), (3, 256), (8, 1024)):
        sh = ShardedTable(768, [0] * n_sh, block)
        sh.insert(rows)
        assert sh.delete(dead) == dead.size
        assert np.array_equal(sh.deleted(), dead)
        for k in (10, 1000):
            _same(sh.knn(qs, k), want[k], (n_sh, k))
            i, d = sh.knn_async(qs, k)
            sh.sync()
            _same((i, d), want[k], (n_sh, k, "async"))
        if n_sh == 3:
            sh.save(prefix)
            moved = ShardedTable(768, [0, 0], 512)             # another shard count and block size: the re-deal path
            moved.load(prefix)
            assert np.array_equal(moved.deleted(), dead)
            _same(moved.knn(qs, 10), want[10], "re-dealt")
            same = ShardedTable(768, [0, 0, 0], 256)
            same.load(prefix)
            assert np.array_equal(same.deleted(), dead)
            _same(same.knn(qs, 1000), want[1000], "same layout")
            re = ShardedTable(768, [0] * 5, 128)
            re.rebalance_from(sh)
            assert np.array_equal(re.deleted(), dead)
            _same(re.knn(qs, 10), want[10], "rebalanced")
            for h in (moved, same, re):
                h.close()
        with pytest.raises(MiError):
            sh.delete([n])
        sh.close()
    one.close()


def _tiny_model(tmp_path):
    from image_search_amd.clip import PRECISION_F32, Model
    cfg = synth.VitConfig.tiny()
    path = str(tmp_path / "tiny.safetensors")
    synth.save_safetensors(synth.vit_weights(cfg, 1), path, {"num_attention_heads": cfg.heads})
    return cfg, Model.from_file(path, 0, PRECISION_F32)


def test_pipeline_query_honours_deletions(built, orc, tmp_path):
    from image_search_amd.search import Pipeline
    cfg, m = _tiny_model(tmp_path)
    t = EmbeddingTable(cfg.proj, 0)
    pipe = Pipeline(m, t)
    px = synth.preprocess_rgb8(synth.images_u8(7, 24, cfg.image))
    assert pipe.ingest(px[:12]) == 0
    assert pipe.ingest(px[12:]) == 12
    pipe.sync()
    rows = t.rows(0, 24)
    dead = [2, 5, 13, 20]
    t.delete(dead)
    q = rows[5]
    i, d = pipe.query(q, 30)
    pipe.sync()
    _same((i, d), _oracle(orc, q, rows, dead, 30))
    assert pipe.ingest(px[:4]) == 24                          # ingest after a delete works unchanged
    pipe.sync()
    pipe.close(); t.close(); m.close()


def test_index_remove(built, orc, tmp_path):
    dim = 768
    rows = synth.corpus_rows(71, 0, 40)
    paths = [f"/m/img{i}.jpg" for i in range(40)]
    paths[30] = "/m/img3.jpg"                                  # a path that owns two rows: 3 and 30
    ix = ImageIndex(dim, 0, "/m/")
    ix.insert(paths, rows)
    assert ix.remove(["/m/img3.jpg", "/m/img7.jpg", "/m/not-there.jpg"]) == 3
    assert ix.existing(["/m/img3.jpg", "/m/img7.jpg", "/m/img8.jpg"]) == {"/m/img8.jpg"}
    assert ix.embeddings_of(["/m/img3.jpg", "/m/img8.jpg"])[0] == [8]
    gone = [3, 7, 30]
    res = ix.web_search_text(rows[3], (), 50)                 # k above the live count
    assert len(res) == 37 and not {r[0] for r in res} & set(gone)
    with pytest.raises(MiError) as e:
        ix.path(30)
    assert e.value.code == -1 and "removed" in str(e.value)
    # a removed path named by the client does not refine the query
    assert ix.web_search_text(rows[9], ["media/img3.jpg"], 5) == ix.web_search_text(rows[9], (), 5)
    ix.save(str(tmp_path / "ix"))
    ix2 = ImageIndex.load(str(tmp_path / "ix"), 0, dim)
    assert ix2.existing(["/m/img3.jpg", "/m/img8.jpg"]) == {"/m/img8.jpg"}
    assert [r[0] for r in ix2.web_search_text(rows[3], (), 50)] == [r[0] for r in res]
    with pytest.raises(MiError):
        ix2.path(3)
    new = synth.corpus_rows(72, 0, 1)
    assert ix2.insert(["/m/img3.jpg"], new) == 40              # the path comes back: a new id, found
    assert ix2.web_search_text(new[0], (), 1)[0][0] == 40
    assert ix2.embeddings_of(["/m/img3.jpg"])[0] == [40]
    ix.close(); ix2.close()


def test_scan_prunes_deleted_and_moved_files(built, tmp_path):
    from PIL import Image
    cfg, m = _tiny_model(tmp_path)
    out = {}
    for prune in (True, False):                              # the same media dir and the same changes, scanned both ways
        media = tmp_path / f"media_{prune}"
        (media / "a").mkdir(parents=True)
        for i in range(4):
            Image.fromarray(synth.photo_u8(80 + i, 48, 64)).save(media / "a" / f"im{i}.png")
        ix = ImageIndex(cfg.proj, 0, str(media) + "/")
        assert embed_all_images_in_dir(m, ix, str(media), image_chunk_size=3, shuffle_seed=1) == 4
        os.remove(media / "a" / "im0.png")                  # a deleted photo
        (media / "b").mkdir()
        os.rename(media / "a" / "im1.png", media / "b" / "im1.png")   # a moved one
        assert embed_all_images_in_dir(m, ix, str(media), image_chunk_size=3, prune=prune) == 1   # the moved file, once
        assert embed_all_images_in_dir(m, ix, str(media), image_chunk_size=3, prune=prune) == 0
        a = [str(media / "a" / f"im{i}.png") for i in range(4)]
        out[prune] = (ix.live_paths(), set(int(i) for i in ix.table.deleted()), a, str(media / "b" / "im1.png"))
        ix.close()
    live, dead, a, moved = out[True]
    assert live == {a[2], a[3], moved} and len(dead) == 2   # exactly the rows of the deleted and the moved file
    live, dead, a, moved = out[False]
    assert live == set(a) | {moved} and not dead              # the reference's behaviour: the stale rows stay
    m.close()
