"""Host checks of the undistortion (no GPU): the float32 restatement of tests/undistort_ref.py against the float64
model on every case of the GPU list, fit_scale, Distortion.from_colmap, read_colmap's `distortion` field, and the argument
checks of the two entry points (refused before any GPU call)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import undistort_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dist(model="SIMPLE_RADIAL", w=640, h=480, fx=500.0, fy=500.0, cx=320.0, cy=240.0, **k):
    from brush_amd.undistort import Distortion

    return Distortion(model, w, h, fx, fy, cx, cy, **k)


def _map_of(d, s):
    """The restatement's map of Distortion `d` at scale `s` (output: the source's size and principal point)."""
    return R.make_map(d.fx, d.fy, d.cx, d.cy, s * d.fx, s * d.fy, d.cx, d.cy,
                      **{k: getattr(d, k) for k in R.COEFFS})


# ---------------------------------------------------------------------------- restatement against float64
@pytest.mark.parametrize("case", R.all_cases(), ids=lambda c: c[0])
def test_restatement_is_within_one_q8_unit_of_float64(case):
    """Every pixel of every case, valid or not: the float32 recipe's Q8 coordinates are within 1 unit (1/256 px) of the
    float64 model's.  (0.5 of it is the rint; the list was fixed after this held.)"""
    _, w, h, ow, oh, m = case
    qx, qy, valid = R.q8_f32(m, w, h, ow, oh)
    fx, fy = R.q8_f64(m, ow, oh)
    assert np.isfinite(fx).all() and np.isfinite(fy).all()
    assert np.abs(qx - fx).max() <= 1.0 and np.abs(qy - fy).max() <= 1.0


def test_case_list_covers_what_it_names():
    cases = R.all_cases()
    assert len({c[0] for c in cases}) == len(cases)
    shapes = {(c[1], c[2], c[3], c[4]) for c in cases}
    assert {(1, 1, 1, 1), (17, 13, 17, 13), (64, 64, 64, 64), (65, 9, 65, 9), (257, 5, 257, 5)} <= shapes
    assert any((w, h) != (ow, oh) for w, h, ow, oh in shapes)
    valid = {c[0]: R.q8_f32(c[5], c[1], c[2], c[3], c[4])[2].mean() for c in cases}
    # zoomed out four times, most of the output is invalid; zoomed in twice, none of it
    assert all(0 < v < 0.5 for k, v in valid.items() if k.endswith("scale 0.25"))
    assert all(v == 1 for k, v in valid.items() if k.endswith("scale 2.0"))
    m = cases[8][5]
    assert m["fx"] != m["fy"] and m["cx"] != 0.5 * cases[8][1]


def test_restatement_identity_and_invalid_sentinels():
    img = R.pattern_image(40, 30, 3, 1)
    m = R.make_map(37.0, 41.0, 20.0, 15.0, 37.0, 41.0, 20.0, 15.0)
    out, valid = R.undistort_u8_ref(img, m, 40, 30)
    assert np.array_equal(out, img) and valid.all()
    # coordinates beyond 2^30 Q8 units, infinite ones and NaN (inf / inf) are invalid, never wrapped into the image
    for bad in (dict(m, k1=1e30), dict(m, k1=3e38), dict(m, k1=float("inf"), k4=float("inf"))):
        out, valid = R.undistort_u8_ref(img, bad, 40, 30)
        assert not valid.any() and not out.any()


# ---------------------------------------------------------------------------- fit_scale
FIT_CASES = {
    "barrel": dict(k1=-0.3),
    "pincushion": dict(k1=0.2),
    "mild": dict(k1=-0.05),
    "opencv": dict(model="OPENCV", fx=500.0, fy=520.0, cx=310.0, cy=250.0, k1=-0.12, k2=0.03, p1=0.003, p2=-0.002),
    "full_opencv": dict(model="FULL_OPENCV", fx=480.0, fy=500.0, cx=330.0, cy=236.0, k1=0.3, k2=-0.1, p1=0.001,
                        p2=-0.0015, k3=0.02, k4=0.35, k5=-0.05, k6=0.01),
}


def _border_f64(d, s):
    """Source pixel coordinates (float64, through the restatement module's model) of the output's border centres."""
    w, h = d.width, d.height
    xs, ys = np.arange(w) + 0.5, np.arange(h) + 0.5
    px = np.concatenate([xs, xs, np.full(h, 0.5), np.full(h, w - 0.5)])
    py = np.concatenate([np.full(w, 0.5), np.full(w, h - 0.5), ys, ys])
    m = {"fx": d.fx, "fy": d.fy, "cx": d.cx, "cy": d.cy, "ocx": d.cx, "ocy": d.cy, "iofx": 1.0 / (s * d.fx),
         "iofy": 1.0 / (s * d.fy), **{k: getattr(d, k) for k in R.COEFFS}}
    return R.distort_f64(m, px, py)


def _inside(d, s, margin):
    u, v = _border_f64(d, s)
    return bool(((u >= 0.5 + margin) & (u <= d.width - 0.5 - margin) & (v >= 0.5 + margin)
                 & (v <= d.height - 0.5 - margin)).all())


@pytest.mark.parametrize("name", list(FIT_CASES))
def test_fit_scale_is_the_smallest_scale_that_keeps_the_border_inside(name):
    from brush_amd.undistort import fit_scale

    d = _dist(**FIT_CASES[name])
    s = fit_scale(d)
    assert 0.25 < s < 4.0
    assert _inside(d, s, 1.0 / 64.0)
    assert not _inside(d, s * (1.0 - 1e-5), 1.0 / 64.0)
    # and in float32 no pixel of the output is invalid: the margin absorbs the rounding
    _, _, valid = R.q8_f32(_map_of(d, s), d.width, d.height, d.width, d.height)
    assert valid.all()
    assert fit_scale(d, margin=0.5) > s


def test_fit_scale_direction():
    """On the edge midpoint of the x axis the model reads xd = x (1 + k1 x^2).  With k1 < 0 (barrel: the source pulls
    points towards the centre) the output's border at s = 1 maps strictly inside the source, so a smaller focal still
    fits and s < 1: the output shows the inscribed rectangle, which is wider than the source's own frame.  With k1 > 0
    (pincushion) the border at s = 1 maps outside and only a longer focal fits: s > 1.  Both signs were also determined
    by running the cases (0.918 and 1.105 on this camera), not assumed."""
    from brush_amd.undistort import fit_scale

    barrel, pincushion = fit_scale(_dist(k1=-0.3)), fit_scale(_dist(k1=0.2))
    assert barrel < 1.0 < pincushion
    assert abs(barrel - 0.9185) < 1e-3 and abs(pincushion - 1.1046) < 1e-3
    # corners pulled in while the edge midpoints are pushed out: the midpoints decide, s > 1
    assert fit_scale(_dist("RADIAL", k1=0.3, k2=-0.6)) > 1.0


def test_fit_scale_refuses_what_cannot_fit():
    from brush_amd.undistort import fit_scale

    with pytest.raises(ValueError):
        fit_scale(_dist(k1=500.0))  # even four times the focal leaves the border outside
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):
        fit_scale(_dist("OPENCV_FISHEYE", k1=0.1))


# ---------------------------------------------------------------------------- Distortion.from_colmap
def test_from_colmap_none_cases():
    from brush_amd import dataset as D
    from brush_amd.undistort import Distortion

    assert Distortion.from_colmap(D.ColmapCamera(1, 0, 640, 480, [500.0, 320.0, 240.0]), 640, 480) is None
    assert Distortion.from_colmap(D.ColmapCamera(1, 1, 640, 480, [500.0, 510.0, 320.0, 240.0]), 640, 480) is None
    assert Distortion.from_colmap(D.ColmapCamera(1, 2, 640, 480, [500.0, 320.0, 240.0, 0.0]), 640, 480) is None
    assert Distortion.from_colmap(D.ColmapCamera(1, 4, 640, 480, [500.0, 510.0, 320.0, 240.0, 0, 0, 0, 0]), 640, 480) is None
    assert Distortion.from_colmap(D.ColmapCamera(1, 5, 640, 480, [500.0, 510.0, 320.0, 240.0, 0, 0, 0, 0]), 640, 480) is None


def test_from_colmap_fields_and_scaling():
    from brush_amd import dataset as D
    from brush_amd.undistort import Distortion

    d = Distortion.from_colmap(D.ColmapCamera(1, 2, 640, 480, [500.0, 321.0, 239.0, -0.1]), 640, 480)
    assert d == Distortion("SIMPLE_RADIAL", 640, 480, 500.0, 500.0, 321.0, 239.0, k1=-0.1)
    d = Distortion.from_colmap(D.ColmapCamera(1, 3, 640, 480, [500.0, 321.0, 239.0, -0.1, 0.02]), 640, 480)
    assert (d.model, d.k1, d.k2, d.k3, d.p1) == ("RADIAL", -0.1, 0.02, 0.0, 0.0)
    full = [500.0, 510.0, 321.0, 239.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
    d = Distortion.from_colmap(D.ColmapCamera(1, 6, 640, 480, full), 640, 480)
    assert (d.k1, d.k2, d.p1, d.p2, d.k3, d.k4, d.k5, d.k6) == tuple(full[4:])
    # max_resolution shrank the image to 320 x 120: focal and principal point follow per axis, coefficients do not
    d = Distortion.from_colmap(D.ColmapCamera(1, 4, 640, 480, [500.0, 510.0, 321.0, 239.0, -0.1, 0.02, 1e-3, -2e-3]),
                               320, 120)
    assert (d.width, d.height, d.fx, d.fy, d.cx, d.cy) == (320, 120, 250.0, 127.5, 160.5, 59.75)
    assert (d.k1, d.k2, d.p1, d.p2, d.k3) == (-0.1, 0.02, 1e-3, -2e-3, 0.0)


@pytest.mark.parametrize("mid,params", [(5, [500.0, 510.0, 320.0, 240.0, 0.1, 0, 0, 0]), (7, [500.0, 510.0, 320.0, 240.0, 0.9]),
                                        (8, [500.0, 320.0, 240.0, 0.1]), (9, [500.0, 320.0, 240.0, 0.0, 0.1]),
                                        (10, [500.0, 510.0, 320.0, 240.0] + [0.0] * 7 + [1e-3])])
def test_unsupported_models_raise_on_use_not_on_read(mid, params):
    from brush_amd import dataset as D
    from brush_amd.undistort import Distortion, fit_scale, undistort_map, undistorted_camera

    d = Distortion.from_colmap(D.ColmapCamera(1, mid, 640, 480, params), 640, 480)  # does not raise
    name = D._COLMAP_MODELS[mid][0]
    assert d is not None and d.model == name
    cam = D.colmap_camera([1, 0, 0, 0], [0, 0, 4], D.ColmapCamera(1, mid, 640, 480, params))
    for use in (lambda: fit_scale(d), lambda: undistort_map(d, 1.0), lambda: undistorted_camera(cam, d, 1.0)):
        with pytest.raises(ValueError, match=name):
            use()


def test_undistorted_camera():
    import brush_amd
    from brush_amd.undistort import undistorted_camera

    d = _dist("OPENCV", fx=500.0, fy=520.0, cx=310.0, cy=250.0, k1=-0.1)
    cam = brush_amd.Camera([1.0, 2.0, 3.0], [0.0, 0.0, 0.0, 1.0], 1.0, 0.8, (310.0 / 640, 250.0 / 480))
    out = undistorted_camera(cam, d, 0.9)
    assert np.array_equal(out.position, cam.position) and np.array_equal(out.rotation, cam.rotation)
    assert out.center_uv == cam.center_uv
    assert abs(brush_amd.fov_to_focal(out.fov_x, 640) - 450.0) < 1e-9
    assert abs(brush_amd.fov_to_focal(out.fov_y, 480) - 468.0) < 1e-9


def test_map_matches_the_restatements():
    from brush_amd.undistort import undistort_map

    d = _dist(**FIT_CASES["full_opencv"])
    got, want = undistort_map(d, 0.93), _map_of(d, 0.93)
    assert {k: getattr(got, k) for k in R.FIELDS} == want


# ---------------------------------------------------------------------------- read_colmap
def test_read_colmap_fills_distortion_and_nothing_else(tmp_path):
    from brush_amd import dataset as D
    from brush_amd.undistort import Distortion

    root = str(tmp_path / "scene")
    cams = [("PINHOLE", [40.0, 42.0, 24.0, 18.0]), ("SIMPLE_RADIAL", [40.0, 23.0, 19.0, -0.2])]
    images = R.write_colmap_tree(root, cams)
    views = D.read_colmap(root).train.views
    assert len(views) == 2
    assert views[0].distortion is None
    assert views[1].distortion == Distortion("SIMPLE_RADIAL", 48, 36, 40.0, 40.0, 23.0, 19.0, k1=-0.2)
    for i, (v, (model, params)) in enumerate(zip(views, cams)):
        want = D.colmap_camera([1.0, 0.0, 0.0, 0.0], [0.1 * i, 0.0, 4.0],
                               D.ColmapCamera(i + 1, D._COLMAP_MODEL_IDS[model], 48, 36, params))
        assert np.array_equal(v.camera.position, want.position) and np.array_equal(v.camera.rotation, want.rotation)
        assert (v.camera.fov_x, v.camera.fov_y, v.camera.center_uv) == (want.fov_x, want.fov_y, want.center_uv)
        assert np.array_equal(v.image, images[i]) and v.depth is None
    small = D.read_colmap(root, max_resolution=24).train.views[1]
    assert small.image.shape == (18, 24, 3)
    assert small.distortion == Distortion("SIMPLE_RADIAL", 24, 18, 20.0, 20.0, 11.5, 9.5, k1=-0.2)
    bare = D.read_colmap(root, load_images=False).train.views[1]  # no image: the camera's own size
    assert (bare.distortion.width, bare.distortion.height, bare.distortion.fx) == (48, 36, 40.0)


def test_scene_view_default_and_exports():
    import brush_amd
    from brush_amd.dataset import SceneView

    v = SceneView("a", None, np.zeros((1, 1, 3), np.uint8))
    assert v.distortion is None
    for name in ("Distortion", "fit_scale", "undistort_image", "undistort_depth", "undistorted_camera",
                 "undistort_dataset"):
        assert hasattr(brush_amd, name), name


# ---------------------------------------------------------------------------- the ABI without a GPU
def test_argument_checks_return_before_any_gpu_call():
    """Every refused call returns BRUSH_ERR_INVALID_ARG from the host-side checks: this machine has no GPU, so a launch
    would show as a HIP error instead."""
    from brush_amd import _lib

    l = _lib.lib()
    m = _lib.BrushUndistort()
    st = None
    a, b = 0x10000000, 0x20000000  # never dereferenced
    assert l.brush_undistort_u8(None, 8, 8, 3, b, 8, 8, None, m, st) == -1
    assert l.brush_undistort_u8(a, 8, 8, 3, None, 8, 8, None, m, st) == -1
    assert l.brush_undistort_u8(a, 8, 8, 3, b, 8, 8, None, None, st) == -1
    assert l.brush_undistort_u8(a, 8, 8, 2, b, 8, 8, None, m, st) == -1
    assert l.brush_undistort_u8(a, 8, 8, 5, b, 8, 8, None, m, st) == -1
    assert l.brush_undistort_u8(a, 0, 8, 3, b, 8, 8, None, m, st) == -1
    assert l.brush_undistort_u8(a, 8, 8, 3, b, 8, 0, None, m, st) == -1
    assert l.brush_undistort_u8(a, 8193, 8, 3, b, 8, 8, None, m, st) == -1
    assert l.brush_undistort_u8(a, 8, 8, 3, b, 8, 8193, None, m, st) == -1
    assert l.brush_undistort_u8(a, 8, 8, 3, a + 8 * 8 * 3 - 1, 8, 8, None, m, st) == -1   # dst begins in src's last byte
    assert l.brush_undistort_u8(a, 8, 8, 3, b, 8, 8, b + 8 * 8 * 3 - 1, m, st) == -1       # the mask overlaps dst
    assert l.brush_undistort_nearest(None, 4, 8, 8, b, 8, 8, m, st) == -1
    assert l.brush_undistort_nearest(a, 4, 8, 8, b, 8, 8, None, st) == -1
    assert l.brush_undistort_nearest(a, 3, 8, 8, b, 8, 8, m, st) == -1
    assert l.brush_undistort_nearest(a, 4, 8, 8, b + 2, 8, 8, m, st) == -1                  # misaligned
    assert l.brush_undistort_nearest(a, 2, 8, 8193, b, 8, 8, m, st) == -1
    assert l.brush_undistort_nearest(a, 2, 8, 8, a + 64, 8, 8, m, st) == -1                 # overlap
    assert C.sizeof(_lib.BrushUndistort) == 64


def test_cli_flag():
    from brush_amd import eval as E
    from brush_amd import train_loop as T

    assert T.parser().parse_args(["scene"]).no_undistort is False
    assert T.parser().parse_args(["scene", "--no-undistort"]).no_undistort is True
    assert E.parser().parse_args(["a.ply", "scene", "--no-undistort"]).no_undistort is True


def test_undistort_for_cli_leaves_pinhole_datasets_alone(tmp_path, capsys):
    from brush_amd import dataset as D
    from brush_amd.undistort import undistort_for_cli

    root = str(tmp_path / "scene")
    R.write_colmap_tree(root, [("PINHOLE", [40.0, 42.0, 24.0, 18.0]), ("SIMPLE_RADIAL", [40.0, 23.0, 19.0, -0.2])])
    data = D.read_colmap(root)
    assert undistort_for_cli(data, enabled=False) is data  # --no-undistort: as loaded, nothing printed, no device
    pin = D.Dataset(D.Scene(data.train.views[:1]))
    assert undistort_for_cli(pin) is pin
    assert capsys.readouterr().out == ""
