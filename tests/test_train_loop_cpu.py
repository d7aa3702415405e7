"""Host-side checks of the training loop's pieces (brush_amd.scene_loader, brush_amd.train_loop, the Splats
initialisations): no GPU needed."""
import math
import os

import numpy as np
import pytest

from tests import eval_data as E


def _scene(n=5, w=6, h=4):
    from brush_amd.dataset import Scene, SceneView, nerf_camera

    views = []
    for i in range(n):
        a = 2.0 * math.pi * i / n
        c2w = E.look_at_gl((3.0 * math.cos(a), 2.0 * math.sin(a), 0.5 + 0.1 * i))
        img = np.full((h, w, 3 + (i % 2)), i, dtype=np.uint8)
        views.append(SceneView(f"v{i}", nerf_camera(c2w, 0.7, w, h), img))
    return Scene(views)


def test_scene_loader_sequence_is_seeded():
    from brush_amd.scene_loader import SceneLoader

    scene = _scene()

    def seq(seed):
        loader = SceneLoader(scene, seed, "cpu")
        return [loader.next_index() for _ in range(50)]

    a, b, c = seq(42), seq(42), seq(43)
    assert a == b and a != c
    r = np.random.default_rng(42)
    assert a == [int(r.integers(0, 5)) for _ in range(50)]
    assert set(a) == set(range(5))

    loader = SceneLoader(scene, 7, "cpu")
    expect = np.random.default_rng(7)
    for _ in range(10):
        view, img = loader.next_batch()
        i = int(expect.integers(0, 5))
        assert view is scene.views[i]
        assert img.dtype.is_floating_point is False and tuple(img.shape) == scene.views[i].image.shape
        assert int(img[0, 0, 0]) == i  # the view's own u8 image, alpha kept
    assert loader.total_bytes == sum(v.image.nbytes for v in scene.views)
    with pytest.raises(ValueError):
        SceneLoader(scene, 7, "cpu", batch_size=2)


def test_scene_extent_and_random_init_bounds():
    from brush_amd.scene_loader import SceneLoader, scene_extent
    from brush_amd.train_loop import random_init_bounds

    scene = _scene()
    lo, hi = scene.bounds(0.0, 0.0)
    # camera positions only: x in [-3*cos(36deg) .. 3], y in +-2*sin(72deg), z in [0.5, 0.9]
    xs = [3.0 * math.cos(2 * math.pi * i / 5) for i in range(5)]
    ys = [2.0 * math.sin(2 * math.pi * i / 5) for i in range(5)]
    half = [(max(xs) - min(xs)) / 2, (max(ys) - min(ys)) / 2, 0.4 / 2]
    assert scene_extent(scene) == pytest.approx(max(half), rel=1e-6)
    assert scene_extent(scene) == float(np.max((hi - lo) / np.float32(2)))
    assert SceneLoader(scene, 0, "cpu").scene_extent == scene_extent(scene)
    e = float(np.linalg.norm((hi - lo) / np.float32(2)))
    assert e == pytest.approx(math.sqrt(sum(x * x for x in half)), rel=1e-6)
    blo, bhi = random_init_bounds(scene)
    rlo, rhi = scene.bounds(0.25 * e, e)
    assert np.array_equal(blo, rlo) and np.array_equal(bhi, rhi)


def test_from_random_config_on_the_host():
    from brush_amd import Splats

    lo, hi = np.array([-1.0, 2.0, -0.5], np.float32), np.array([1.0, 2.5, 3.0], np.float32)
    s = Splats.from_random_config(500, 1, (lo, hi), np.random.default_rng(0), "cpu")
    m = s.means.detach().numpy()
    assert m.shape == (500, 3) and (m >= lo).all() and (m < hi).all()
    assert tuple(s.sh_coeffs.shape) == (500, 4, 3) and tuple(s.rotation.shape) == (500, 4)
    assert tuple(s.log_scales.shape) == (500, 3) and tuple(s.raw_opacity.shape) == (500,)
    assert np.array_equal(s.rotation.detach().numpy(), np.tile([1.0, 0.0, 0.0, 0.0], (500, 1)).astype(np.float32))
    assert np.allclose(s.raw_opacity.detach().numpy(), math.log(0.1 / 0.9))
    sh = s.sh_coeffs.detach().numpy()
    assert (sh[:, 1:] == 0).all()
    colors = sh[:, 0] * np.float32(0.2820947917738781) + 0.5
    assert (colors > -1e-6).all() and (colors < 1.0 + 1e-6).all()
    ls = s.log_scales.detach().numpy()
    assert (ls[:, 0] == ls[:, 1]).all() and np.isfinite(ls).all()
    # the same generator state gives the same splats; the draws are positions first, then colours
    t = Splats.from_random_config(500, 1, (lo, hi), np.random.default_rng(0), "cpu")
    assert np.array_equal(t.means.detach().numpy(), m)
    r = np.random.default_rng(0)
    pos = r.uniform(lo, hi, size=(500, 3)).astype(np.float32)
    assert np.array_equal(np.minimum(pos, np.nextafter(hi, lo)), m)
    with pytest.raises(ValueError):
        Splats.from_random_config(10, 0, None, np.random.default_rng(0), "cpu")


def test_from_point_cloud_matches_dataset_init():
    from brush_amd import Splats
    from brush_amd.dataset import splat_init_from_point_cloud

    rng = np.random.default_rng(4)
    pos, col = rng.random((64, 3), dtype=np.float32), rng.random((64, 3), dtype=np.float32)
    s = Splats.from_point_cloud(pos, col, 3, "cpu")
    d = splat_init_from_point_cloud(pos, col, 3)
    for name, key in (("means", "means"), ("sh_coeffs", "sh"), ("rotation", "quats"), ("raw_opacity", "raw_opac"),
                      ("log_scales", "log_scales")):
        assert np.array_equal(getattr(s, name).detach().numpy(), d[key]), name


def test_cli_argument_errors(tmp_path, capsys):
    from brush_amd import train_loop

    with pytest.raises(SystemExit) as e:
        train_loop.main([str(tmp_path / "missing")])
    assert e.value.code == 2
    root = str(tmp_path / "nerf")
    E.write_nerf(root, 8, 6, n_train=3, with_val=False)
    assert train_loop.main([root, "--eval-every", "10", "--steps", "20"]) == 2
    assert "eval views" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        train_loop.main([root, "--steps", "-1"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        train_loop.main([root, "--init", os.path.join(root, "nope.ply")])
    assert e.value.code == 2


def test_train_loop_is_imported_lazily():
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys, brush_amd; assert 'brush_amd.train_loop' not in sys.modules; brush_amd.train_scene; " \
           "assert 'brush_amd.train_loop' in sys.modules"
    subprocess.run([sys.executable, "-c", code], cwd=root, check=True)
