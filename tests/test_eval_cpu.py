"""CPU-side checks of the evaluation path (brush_amd.eval): view selection, dataset-format detection, the command
line's exit status on a dataset without eval views, the exported names, the ABI's argument checks, and the cameras
the readers build for the test-written datasets tests/test_gpu_eval.py renders."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import eval_data as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_names_are_exported():
    import brush_amd
    from brush_amd import EvalStats, EvalView, eval_metrics, eval_stats  # noqa: F401

    assert callable(brush_amd.eval_stats) and callable(brush_amd.eval_metrics)
    s = EvalStats([EvalView(None, None, 20.0, 0.5), EvalView(None, None, 30.0, 0.7)])
    assert s.mean_psnr() == 25.0 and abs(s.mean_ssim() - 0.6) < 1e-12
    assert np.isnan(EvalStats().mean_psnr())


def test_view_selection():
    from brush_amd.eval import select_views

    assert select_views(7) == list(range(7))
    assert select_views(7, None, np.random.default_rng(1)) == list(range(7))
    assert select_views(7, 7, np.random.default_rng(1)) == list(range(7))
    assert select_views(7, 100, np.random.default_rng(1)) == list(range(7))
    a = select_views(50, 9, np.random.default_rng(123))
    assert len(a) == 9 and len(set(a)) == 9 and all(0 <= i < 50 for i in a)
    assert select_views(50, 9, np.random.default_rng(123)) == a
    assert select_views(50, 0, np.random.default_rng(3)) == []


def test_format_detection(tmp_path):
    from brush_amd.eval import detect_format

    E.write_nerf(str(tmp_path / "nerf"), 24, 16, n_train=1, n_val=1)
    E.write_colmap(str(tmp_path / "colmap"), 24, 16, n_images=2)
    assert detect_format(str(tmp_path / "nerf")) == "nerf"
    assert detect_format(str(tmp_path / "colmap")) == "colmap"
    # a zip of the NeRF tree, nested one directory down
    import shutil

    z = shutil.make_archive(str(tmp_path / "nerf_zip"), "zip", str(tmp_path), "nerf")
    assert detect_format(z) == "nerf"


def test_cli_without_eval_views_exits_2(tmp_path):
    """No transforms_val.json and no --eval-split-every: no eval views.  The command must stop with status 2 before it
    loads the splats (the file does not even exist) or touches a GPU."""
    E.write_nerf(str(tmp_path / "nerf"), 24, 16, n_train=2, with_val=False)
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "brush_amd.eval", str(tmp_path / "missing.ply"), str(tmp_path / "nerf"),
                        "--json", str(tmp_path / "out.json")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "no eval views" in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert not (tmp_path / "out.json").exists()


def test_reader_cameras_match_hand_built_uniforms(tmp_path):
    """The cameras the readers build for the test datasets pack into the uniforms tests/test_gpu_eval.py expects."""
    from brush_amd import dataset as D
    from brush_amd.render import pack_uniforms

    def unpack(u):
        return {"viewmat": np.array(u.viewmat[:]), "focal": np.array(u.focal[:]), "img_size": np.array(u.img_size[:]),
                "pixel_center": np.array(u.pixel_center[:])}

    rec = E.write_nerf(str(tmp_path / "nerf"), 40, 30)
    views = D.read_nerf_synthetic(str(tmp_path / "nerf")).eval.views
    assert len(views) == 3
    for v, (_, c2w, img) in zip(views, rec["val"]):
        assert np.array_equal(v.image, img)
        E.uniforms_close(unpack(pack_uniforms(v.camera, (40, 30), 3, 10)),
                         E.nerf_uniforms(c2w, rec["camera_angle_x"], 40, 30, 3))
    rec = E.write_colmap(str(tmp_path / "colmap"), 40, 30)
    views = D.read_colmap(str(tmp_path / "colmap"), eval_split_every=1).eval.views
    assert len(views) == 3
    for v, (_, q, t, img) in zip(views, rec["images"]):
        assert np.array_equal(v.image, img)
        E.uniforms_close(unpack(pack_uniforms(v.camera, (40, 30), 3, 10)), E.colmap_uniforms(q, t, rec["camera"], 3))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def test_eval_abi_rejects_bad_arguments_without_gpu(lib):
    """Every check runs on the host before anything is enqueued (so it needs no device)."""
    n = C.c_size_t()
    assert lib.brush_eval_workspace_size(1920, 1080, C.byref(n)) == 0 and n.value > 0
    assert lib.brush_eval_workspace_size(0, 1080, C.byref(n)) == -1
    assert lib.brush_eval_workspace_size(8, 8, None) == -1
    lib.brush_eval_workspace_size(8, 8, C.byref(n))
    fake = 4096  # never dereferenced: every call below is rejected first
    ok = dict(pred=fake, gt=fake, dt=0, w=8, h=8, c=3, win=11, out=fake, ws=fake, nb=n.value)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.brush_eval_metrics(a["pred"], a["gt"], a["dt"], a["w"], a["h"], a["c"], a["win"], a["out"], a["ws"],
                                      a["nb"], None)

    for bad in (dict(pred=None), dict(gt=None), dict(out=None), dict(ws=None), dict(w=0), dict(h=0), dict(dt=2),
                dict(c=2), dict(c=5), dict(win=1), dict(win=2), dict(win=12), dict(win=17), dict(w=1 << 14, h=1 << 14)):
        assert call(**bad) == -1, bad
    assert call(nb=n.value - 1) == -2
