"""What the six command lines share (brush_amd/cli.py), without a GPU: the option rows every parser() declares, the
choice of views, and the one dataset reader behind the command lines and train_loop.load_dataset."""
import importlib
import shutil

import numpy as np
import pytest

from tests import eval_data as E

# module, the positional arguments, --views' default (None: no such option), has --export
COMMANDS = [("eval", ["s.ply", "scene"], None, False),
            ("train_loop", ["scene"], None, True),
            ("prune", ["s.ply", "scene"], "train", True),
            ("lift", ["s.ply", "scene", "--labels", "seg"], "train", True),
            ("mesh", ["s.ply", "scene"], "train", True),
            ("compress", ["s.ply"], "eval", True)]


@pytest.mark.parametrize("name,positional,views,export", COMMANDS, ids=[c[0] for c in COMMANDS])
def test_shared_options_keep_names_and_defaults(name, positional, views, export):
    parser = importlib.import_module(f"brush_amd.{name}").parser
    a = parser().parse_args(positional)
    assert (a.format, a.eval_split_every, a.max_resolution, a.no_undistort) == ("auto", None, None, False)
    assert (a.antialiased, a.json) == (False, None)
    assert getattr(a, "views", None) == views
    assert (a.export is None) if export else not hasattr(a, "export")
    more = ["--format", "colmap", "--eval-split-every", "8", "--max-resolution", "800", "--no-undistort",
            "--antialiased", "--json", "o.json"] + (["--views", "all"] if views else []) \
        + (["--export", "o.ply"] if export else [])
    a = parser().parse_args(positional + more)
    assert (a.format, a.eval_split_every, a.max_resolution, a.no_undistort) == ("colmap", 8, 800, True)
    assert (a.antialiased, a.json) == (True, "o.json")
    assert getattr(a, "views", None) == ("all" if views else None)
    assert not export or a.export == "o.ply"
    for bad in [["--format", "ply"], ["--max-resolution", "big"]] + ([["--views", "val"]] if views else []):
        with pytest.raises(SystemExit):
            parser().parse_args(positional + bad)


def test_chosen_views():
    from brush_amd.cli import chosen_views
    from brush_amd.dataset import Dataset

    with_eval, without = Dataset.from_views(["t0", "t1"], ["e0"]), Dataset.from_views(["t0", "t1"], [])
    assert without.eval is None
    assert chosen_views(without, "eval") == [] and chosen_views(without, "all") == ["t0", "t1"]
    assert chosen_views(without, "train") == ["t0", "t1"]
    assert [chosen_views(with_eval, w) for w in ("train", "eval", "all")] == [["t0", "t1"], ["e0"], ["t0", "t1", "e0"]]
    assert chosen_views(with_eval, "train") is not with_eval.train.views  # a list of the caller's own


def _same_views(a, b):
    assert [v.name for v in a] == [v.name for v in b]
    for x, y in zip(a, b):
        assert np.array_equal(x.image, y.image)
        assert np.array_equal(x.camera.position, y.camera.position)
        assert np.array_equal(x.camera.rotation, y.camera.rotation)
        assert (x.camera.fov_x, x.camera.fov_y) == (y.camera.fov_x, y.camera.fov_y)


def test_read_dataset_is_the_reader_of_load_dataset(tmp_path):
    from brush_amd.dataset import read_dataset, read_nerf_synthetic
    from brush_amd.train_loop import load_dataset

    E.write_nerf(str(tmp_path / "nerf"), 24, 16, n_train=2, n_val=1)
    tree = str(tmp_path / "nerf")
    zipped = shutil.make_archive(str(tmp_path / "nerf_zip"), "zip", tree)
    want = read_nerf_synthetic(tree)
    assert len(want.train.views) == 2 and len(want.eval.views) == 1
    for root in (tree, zipped):
        got, (loaded, points) = read_dataset(root), load_dataset(root)
        assert points is None
        for data in (got, loaded, read_dataset(root, "nerf")):
            _same_views(data.train.views, want.train.views)
            _same_views(data.eval.views, want.eval.views)
    # the keyword arguments reach the reader
    small, _ = load_dataset(tree, "auto", 12, 2)
    for data in (small, read_dataset(tree, max_resolution=12, eval_split_every=2)):
        assert max(data.train.views[0].image.shape[:2]) == 12
    _same_views(small.train.views, read_dataset(tree, max_resolution=12, eval_split_every=2).train.views)
