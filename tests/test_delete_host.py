"""Deleted rows without a GPU: the new entry points are declared and bound, and prune_missing_images picks exactly the
stale paths of a scan (deleted files, moved folders) under media_dir."""
import os
import re

from conftest import ROOT
from image_search_amd import _lib
from image_search_amd.search import embed_all_images_in_dir, prune_missing_images

NEW = ["mi_knn_delete", "mi_knn_deleted", "mi_knn_sharded_delete", "mi_knn_sharded_deleted", "mi_index_remove",
       "mi_index_live_paths"]


def test_delete_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mi355clip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert name in _lib.SYMBOLS, name


class FakeIndex:
    def __init__(self, paths):
        self.rows = list(paths)
        self.gone = set()

    def live_paths(self):
        return {p for i, p in enumerate(self.rows) if i not in self.gone}

    def remove(self, paths):
        paths = set(paths)
        hit = [i for i, p in enumerate(self.rows) if p in paths and i not in self.gone]
        self.gone.update(hit)
        return len(hit)


def _touch(p):
    os.makedirs(os.path.dirname(p), exist_ok=True)
    open(p, "wb").close()


def test_prune_picks_missing_files_under_media_dir_only(tmp_path):
    media = str(tmp_path / "media")
    keep = [f"{media}/a/x.jpg", f"{media}/a/y.PNG", f"{media}/b/z.webp"]
    for p in keep:
        _touch(p)
    _touch(f"{media}/notes.txt")
    stored = keep + [f"{media}/a/gone.jpg",             # deleted photo
                     f"{media}/old/z.webp",             # the old path of a moved folder
                     f"{media}/notes.txt",              # no longer allow-listed: not an image file
                     f"{media}2/other.jpg",             # a sibling directory that shares the prefix: not under media_dir
                     "/elsewhere/p.jpg",
                     f"{media}/a/gone.jpg"]             # a path that owns two rows
    ix = FakeIndex(stored)
    assert prune_missing_images(ix, media + "/") == 4
    assert ix.live_paths() == set(keep) | {f"{media}2/other.jpg", "/elsewhere/p.jpg"}
    assert prune_missing_images(ix, media) == 0                    # with or without the trailing slash; idempotent


def test_prune_follows_symlinked_dirs_and_takes_the_walk_from_the_caller(tmp_path):
    media = str(tmp_path / "media")
    real = str(tmp_path / "real")
    _touch(f"{real}/r.jpg")
    _touch(f"{media}/m.jpg")
    os.symlink(real, f"{media}/linked")
    ix = FakeIndex([f"{media}/m.jpg", f"{media}/linked/r.jpg", f"{media}/linked/s.jpg"])
    assert prune_missing_images(ix, media) == 1                    # r.jpg is reached through the link
    assert ix.live_paths() == {f"{media}/m.jpg", f"{media}/linked/r.jpg"}
    ix = FakeIndex([f"{media}/m.jpg", f"{media}/linked/r.jpg"])
    assert prune_missing_images(ix, media, found=[f"{media}/m.jpg"]) == 1   # what the caller's walk found decides
    assert ix.live_paths() == {f"{media}/m.jpg"}


def test_scan_prunes_only_when_asked(tmp_path):
    media = str(tmp_path / "media")
    ix = FakeIndex([f"{media}/gone.jpg"])
    os.makedirs(media)

    class NoModel:
        def forward_images(self, images):
            raise AssertionError("nothing to embed")

    ix.existing = lambda paths: set()
    assert embed_all_images_in_dir(NoModel(), ix, media) == 0
    assert ix.live_paths() == {f"{media}/gone.jpg"}                 # the reference's behaviour: rows are never removed
    assert embed_all_images_in_dir(NoModel(), ix, media, prune=True) == 0
    assert ix.live_paths() == set()


def test_an_incomplete_walk_prunes_nothing(tmp_path):
    media = str(tmp_path / "media")
    _touch(f"{media}/a/x.jpg")
    os.symlink(str(tmp_path / "unmounted"), f"{media}/photos")          # a folder whose target is gone (unmounted)
    ix = FakeIndex([f"{media}/a/x.jpg", f"{media}/photos/p.jpg"])
    try:
        prune_missing_images(ix, media)
        raise AssertionError("an incomplete walk must not prune")
    except OSError:
        pass
    assert ix.live_paths() == {f"{media}/a/x.jpg", f"{media}/photos/p.jpg"}
    ix.existing = lambda paths: set(paths)

    class NoModel:
        def forward_images(self, images):
            raise AssertionError("nothing to embed")

    assert embed_all_images_in_dir(NoModel(), ix, media, prune=True) == 0
    assert ix.live_paths() == {f"{media}/a/x.jpg", f"{media}/photos/p.jpg"}   # the scan skips the prune, loses nothing
    try:
        prune_missing_images(ix, str(tmp_path / "no-such-dir"))
        raise AssertionError("a media dir that cannot be walked must not prune")
    except OSError:
        pass
