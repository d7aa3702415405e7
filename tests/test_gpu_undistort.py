"""GPU checks of the undistortion (brush_amd/undistort.py, brush_amd/csrc/undistort.hip): the two kernels against the
float32 restatement of tests/undistort_ref.py, bit for bit (image, mask, both depth dtypes); the identity; invalid pixels
and NaN payloads; the geometry against a float64 evaluation of an analytic pattern, independent of the restatement;
undistort_dataset on a tiny COLMAP tree; refused arguments; graph replay; both command lines."""
import ctypes as C
import dataclasses
import math
import os

import numpy as np
import pytest

from tests import undistort_ref as R

pytestmark = pytest.mark.gpu

INVALID_ARG = -1  # BRUSH_ERR_INVALID_ARG
GUARD = 0xA5


@pytest.fixture(scope="module")
def dev():
    import torch

    import brush_amd  # noqa: F401

    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _struct(m):
    from brush_amd import _lib

    s = _lib.BrushUndistort()
    for k in R.FIELDS:
        setattr(s, k, m[k])
    return s


def _depth_map(w, h, dtype, seed):
    """A depth map with "no measurement" zeros; float32 ones also carry NaNs with payloads, infinities and -0."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint16:
        d = rng.integers(1, 65536, (h, w)).astype(np.uint16)
    else:
        d = (rng.random((h, w), dtype=np.float32) * 10).astype(np.float32)
        bits = d.reshape(-1).view(np.uint32)
        bits[::5] = 0x7FC00000 | (np.arange(bits[::5].size, dtype=np.uint32) * 2654435761 & 0x3FFFFF)  # quiet, payload
        bits[1::7] = 0x7F800001 + (np.arange(bits[1::7].size, dtype=np.uint32) & 0xFFFF)             # signalling
        bits[2::11] = 0xFF800000
        bits[3::13] = 0x80000000
    d.reshape(-1)[4::3] = 0
    return d


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------------------- 1. equality with the restatement
@pytest.mark.parametrize("case", R.all_cases(), ids=lambda c: c[0])
def test_kernels_equal_the_restatement(dev, case):
    import torch

    from brush_amd.undistort import remap_depth, remap_image

    name, w, h, ow, oh, m = case
    s = _struct(m)
    _, _, valid = R.q8_f32(m, w, h, ow, oh)
    for channels in (3, 4):
        img = R.pattern_image(w, h, channels, 7 * w + h + channels)
        got, mask = remap_image(torch.from_numpy(img).to(dev), s, (ow, oh), True)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (oh, ow, channels) and got.is_contiguous()
        want, want_mask = R.undistort_u8_ref(img, m, ow, oh)
        assert np.array_equal(_np(mask), want_mask), name
        assert np.array_equal(_np(got), want), f"{name} x{channels}"
        assert np.array_equal(_np(remap_image(torch.from_numpy(img).to(dev), s, (ow, oh))), want)  # without the mask
    for dtype in (np.uint16, np.float32):
        d = _depth_map(w, h, dtype, 3 * w + h)
        got = remap_depth(torch.from_numpy(d).to(dev), s, (ow, oh))
        want = R.undistort_nearest_ref(d, m, ow, oh)
        assert np.array_equal(_bits(_np(got)), _bits(want)), f"{name} {dtype.__name__}"
        assert not _bits(_np(got))[~valid].any()


@pytest.mark.parametrize("pname", ["opencv_tangential", "full_opencv_rational"])
def test_rgb_source_at_an_odd_address(dev, pname):
    """An RGB source whose first byte sits one byte into a larger buffer (and a destination that does, too)."""
    import torch

    from brush_amd import _lib

    w, h, ow, oh = 65, 9, 65, 9
    m = R.case_map(w, h, ow, oh, R.PARAMS[pname])
    img = R.pattern_image(w, h, 3, 11)
    buf = torch.zeros(w * h * 3 + 1, dtype=torch.uint8, device=dev)
    src = buf[1:]
    src.copy_(torch.from_numpy(img.reshape(-1)).to(dev))
    out = torch.full((ow * oh * 3 + 2,), GUARD, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 2 == 1 and out[1:].data_ptr() % 2 == 1
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().brush_undistort_u8(src.data_ptr(), w, h, 3, out[1:].data_ptr(), ow, oh, None, _struct(m), st),
               "brush_undistort_u8")
    got = _np(out)
    assert got[0] == GUARD and got[-1] == GUARD
    assert np.array_equal(got[1:-1].reshape(oh, ow, 3), R.undistort_u8_ref(img, m, ow, oh)[0])


def test_python_surface_equals_the_restatement(dev):
    """undistort_image / undistort_depth (the source's size, fitted or given scale) against the restatement's map."""
    import torch

    from brush_amd import Distortion, fit_scale, undistort_depth, undistort_image

    d = Distortion("OPENCV", 70, 50, 52.0, 55.0, 33.5, 26.25, k1=-0.15, k2=0.03, p1=0.004, p2=-0.003)
    img = R.pattern_image(70, 50, 4, 5)
    depth = _depth_map(70, 50, np.uint16, 6)
    for scale in (None, 0.8, 1.5):
        s = fit_scale(d) if scale is None else scale
        m = R.make_map(d.fx, d.fy, d.cx, d.cy, s * d.fx, s * d.fy, d.cx, d.cy, k1=d.k1, k2=d.k2, p1=d.p1, p2=d.p2)
        got, mask = undistort_image(torch.from_numpy(img).to(dev), d, scale, return_valid=True)
        want, want_mask = R.undistort_u8_ref(img, m, 70, 50)
        assert np.array_equal(_np(got), want) and np.array_equal(_np(mask), want_mask)
        assert bool(want_mask.all()) == (scale != 0.8)
        assert np.array_equal(_np(undistort_depth(torch.from_numpy(depth).to(dev), d, scale)),
                              R.undistort_nearest_ref(depth, m, 70, 50))
    with pytest.raises(ValueError, match="70x50"):
        undistort_image(torch.from_numpy(img[:, :60].copy()).to(dev), d)
    with pytest.raises(ValueError, match="RADIAL_FISHEYE"):
        undistort_image(torch.from_numpy(img).to(dev), dataclasses.replace(d, model="RADIAL_FISHEYE"))


# ---------------------------------------------------------------------------- 2. the identity
@pytest.mark.parametrize("w,h,cx,cy", [(1, 1, 0.0, 1.0), (257, 5, 128.0, 2.0), (512, 300, 250.0, 161.0), (333, 512, 0.0, 511.0)])
def test_identity_is_exact(dev, w, h, cx, cy):
    import torch

    from brush_amd.undistort import remap_depth, remap_image

    m = R.make_map(0.83 * w + 3, 0.91 * w + 1, cx, cy, 0.83 * w + 3, 0.91 * w + 1, cx, cy)
    for channels in (3, 4):
        img = R.pattern_image(w, h, channels, w + channels)
        got, mask = remap_image(torch.from_numpy(img).to(dev), _struct(m), (w, h), True)
        assert np.array_equal(_np(got), img) and bool((mask == 1).all())
    d = _depth_map(w, h, np.float32, w)
    assert np.array_equal(_bits(_np(remap_depth(torch.from_numpy(d).to(dev), _struct(m), (w, h)))), _bits(d))


# ---------------------------------------------------------------------------- 3. invalid pixels
def test_invalid_pixels_are_zero_and_nan_payloads_survive(dev):
    import torch

    from brush_amd.undistort import remap_depth, remap_image

    w, h, ow, oh = 64, 48, 80, 33
    m = R.case_map(w, h, ow, oh, R.PARAMS["full_opencv_rational"], 0.25)
    _, _, valid = R.q8_f32(m, w, h, ow, oh)
    assert 0 < valid.sum() < valid.size
    full = np.full((h, w, 4), 255, np.uint8)  # every valid pixel is 255, so the zeros are the invalid ones, exactly
    got, mask = remap_image(torch.from_numpy(full).to(dev), _struct(m), (ow, oh), True)
    assert np.array_equal(_np(mask).astype(bool), valid)
    assert np.array_equal(_np(got), np.repeat(np.where(valid, 255, 0).astype(np.uint8)[..., None], 4, axis=2))
    nan = np.full((h, w), 0x7FC12345, np.uint32)
    nan.reshape(-1)[1::2] = 0xFFA54321  # a negative signalling NaN
    got = _np(remap_depth(torch.from_numpy(nan.view(np.float32)).to(dev), _struct(m), (ow, oh))).view(np.uint32)
    want = R.undistort_nearest_ref(nan, m, ow, oh)
    assert np.array_equal(got, want) and not got[~valid].any()
    assert set(np.unique(got[valid]).tolist()) == {0x7FC12345, 0xFFA54321}
    # coordinates that overflow, are infinite or NaN: all invalid
    for bad in (dict(m, k1=1e30), dict(m, k1=3e38), dict(m, k1=float("inf"), k4=float("inf"))):
        got, mask = remap_image(torch.from_numpy(full).to(dev), _struct(bad), (ow, oh), True)
        assert not _np(got).any() and not _np(mask).any()


# ---------------------------------------------------------------------------- 4. geometry against float64
AMP, PERIOD_U, PERIOD_V = 60.0, 37.0, 23.0


def _pattern(u, v):
    """I(u, v) = 127.5 + 60 sin(2 pi u / 37 + 0.3) + 60 sin(2 pi v / 23 + 1.1), inside [7.5, 247.5]: no clipping."""
    return 127.5 + AMP * np.sin(2 * np.pi * u / PERIOD_U + 0.3) + AMP * np.sin(2 * np.pi * v / PERIOD_V + 1.1)


@pytest.mark.parametrize("pname,scale", [("simple_radial_barrel", 1.0), ("simple_radial_pincushion", 1.0),
                                         ("opencv_tangential", 1.0), ("full_opencv_rational", 1.0),
                                         ("radial", 2.0), ("full_opencv_rational", 0.25)])
def test_geometry_against_float64(dev, pname, scale):
    """The source holds I at its pixel centres, rounded; the kernel's output is compared with I at the float64 model's
    source position of every valid output pixel.  The tolerance is derived from the pattern, not measured:
      * the source's rounding: each tap is within 0.5 of I, and the bilinear weights are a convex combination: 0.5;
      * the bilinear interpolation of I itself: I = f(u) + g(v), so it is the sum of two linear interpolations over an
        interval of length 1, each within max|f''| / 8: (A (2 pi / 37)^2 + A (2 pi / 23)^2) / 8;
      * the kernel's coordinates are rounded to 1/256 px, at most 1/512 px away per axis, times the largest slope per
        axis: (A 2 pi / 37 + A 2 pi / 23) / 512;
      * the output's own rounding: 0.5."""
    import torch

    from brush_amd.undistort import remap_image

    w, h, ow, oh = 200, 150, 190, 160
    m = R.case_map(w, h, ow, oh, R.PARAMS[pname], scale)
    ku, kv = 2 * np.pi / PERIOD_U, 2 * np.pi / PERIOD_V
    tol = 0.5 + AMP * (ku * ku + kv * kv) / 8 + AMP * (ku + kv) / 512 + 0.5
    assert tol < 1.85
    su, sv = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    src = np.rint(_pattern(su, sv)).astype(np.uint8)
    img = np.repeat(src[..., None], 3, axis=2)
    got, mask = remap_image(torch.from_numpy(img).to(dev), _struct(m), (ow, oh), True)
    got, mask = _np(got).astype(np.float64), _np(mask).astype(bool)
    px, py = np.meshgrid(np.arange(ow) + 0.5, np.arange(oh) + 0.5)
    u, v = R.distort_f64(m, px, py)
    # valid in float64 up to the 1/256 px the two can differ by at the frame's edge
    inside = (u >= 0.5 + 1 / 128) & (u <= w - 0.5 - 1 / 128) & (v >= 0.5 + 1 / 128) & (v <= h - 0.5 - 1 / 128)
    outside = (u < 0.5 - 1 / 128) | (u > w - 0.5 + 1 / 128) | (v < 0.5 - 1 / 128) | (v > h - 0.5 + 1 / 128)
    assert mask[inside].all() and not mask[outside].any()
    assert mask.sum() > (0.02 if scale < 1 else 0.5) * mask.size
    err = np.abs(got - _pattern(u, v)[..., None])[mask]  # every valid pixel
    print(f"{pname} scale {scale}: max |kernel - I(distort64)| = {err.max():.4f}, tolerance {tol:.4f}")
    assert err.max() <= tol


# ---------------------------------------------------------------------------- 5. undistort_dataset
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("colmap") / "scene")
    cams = [("PINHOLE", [40.0, 42.0, 24.0, 18.0]), ("SIMPLE_RADIAL", [40.0, 23.0, 19.0, -0.2]),
            ("SIMPLE_RADIAL", [40.0, 23.0, 19.0, -0.2]), ("OPENCV", [40.0, 42.0, 23.0, 19.0, 0.1, -0.02, 0.01, -0.01])]
    return root, cams, R.write_colmap_tree(root, cams)


def test_undistort_dataset(dev, tree):
    import brush_amd
    from brush_amd import dataset as D
    from brush_amd import fit_scale, undistort_dataset

    root, cams, images = tree
    data = D.read_colmap(root, eval_split_every=4)
    assert len(data.train.views) == 3 and len(data.eval.views) == 1
    depth = _depth_map(48, 36, np.uint16, 1)
    data.train.views[0].depth = depth  # (im1: the first SIMPLE_RADIAL view)
    out = undistort_dataset(data, dev)
    assert out is not data and len(out.train.views) == 3 and len(out.eval.views) == 1
    assert out.eval.views[0] is data.eval.views[0]  # the pinhole view is shared
    for i, (new, old) in enumerate(zip(out.train.views, data.train.views)):
        d = old.distortion
        s = fit_scale(d)
        assert new is not old and new.distortion is None and old.distortion is d and new.name == old.name
        assert abs(brush_amd.fov_to_focal(new.camera.fov_x, 48) - s * d.fx) < 1e-9 * d.fx
        assert abs(brush_amd.fov_to_focal(new.camera.fov_y, 36) - s * d.fy) < 1e-9 * d.fy
        assert new.camera.center_uv == old.camera.center_uv
        assert np.array_equal(new.camera.position, old.camera.position)
        assert np.array_equal(new.camera.rotation, old.camera.rotation)
        m = R.make_map(d.fx, d.fy, d.cx, d.cy, s * d.fx, s * d.fy, d.cx, d.cy, **{k: getattr(d, k) for k in R.COEFFS})
        want, valid = R.undistort_u8_ref(images[i + 1], m, 48, 36)
        assert valid.all() and new.image.dtype == np.uint8 and np.array_equal(new.image, want)
        assert np.array_equal(old.image, images[i + 1])  # the input dataset is untouched
        if i == 0:
            assert new.depth.dtype == np.uint16 and np.array_equal(new.depth, R.undistort_nearest_ref(depth, m, 48, 36))
            assert (new.depth_scale, new.depth_offset) == (old.depth_scale, old.depth_offset)
        else:
            assert new.depth is None
    assert fit_scale(data.train.views[0].distortion) < 1 < fit_scale(data.train.views[2].distortion)
    # a given scale that leaves part of the output without a source is refused
    with pytest.raises(ValueError, match="no source pixel"):
        undistort_dataset(data, dev, scale=0.5)
    # an undistorted dataset has nothing left to do
    again = undistort_dataset(out, dev)
    assert all(a is b for a, b in zip(again.train.views, out.train.views))


def test_undistort_dataset_names_an_unsupported_model(dev, tmp_path):
    from brush_amd import dataset as D
    from brush_amd import undistort_dataset

    root = str(tmp_path / "scene")
    R.write_colmap_tree(root, [("OPENCV_FISHEYE", [40.0, 42.0, 24.0, 18.0, 0.05, 0.0, 0.0, 0.0])])
    data = D.read_colmap(root)  # reading does not raise
    assert data.train.views[0].distortion.model == "OPENCV_FISHEYE"
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):
        undistort_dataset(data, dev)


# ---------------------------------------------------------------------------- 6. refused arguments, graph replay
def test_refused_arguments_write_nothing(dev):
    import torch

    from brush_amd import _lib

    l = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    m = _struct(R.make_map(10.0, 10.0, 4.0, 4.0, 10.0, 10.0, 4.0, 4.0))
    src = torch.zeros(8 * 8 * 4, dtype=torch.uint8, device=dev)
    dst = torch.full((8 * 8 * 4,), GUARD, dtype=torch.uint8, device=dev)
    mask = torch.full((64,), GUARD, dtype=torch.uint8, device=dev)
    s, d, v = src.data_ptr(), dst.data_ptr(), mask.data_ptr()
    u8, near = l.brush_undistort_u8, l.brush_undistort_nearest
    assert u8(s, 8, 8, 3, s + 100, 8, 8, None, m, st) == INVALID_ARG      # dst inside src
    assert u8(s, 8, 8, 3, d, 8, 8, d + 10, m, st) == INVALID_ARG          # the mask inside dst
    assert u8(s, 8, 8, 3, d, 8, 8, s, m, st) == INVALID_ARG               # the mask over src
    assert u8(s, 8, 8, 2, d, 8, 8, v, m, st) == INVALID_ARG
    assert u8(s, 8, 8, 5, d, 8, 8, v, m, st) == INVALID_ARG
    assert u8(s, 8193, 8, 3, d, 8, 8, v, m, st) == INVALID_ARG
    assert u8(s, 8, 8, 3, d, 8193, 8, v, m, st) == INVALID_ARG
    assert u8(s, 8, 0, 3, d, 8, 8, v, m, st) == INVALID_ARG
    assert u8(None, 8, 8, 3, d, 8, 8, v, m, st) == INVALID_ARG
    assert u8(s, 8, 8, 3, None, 8, 8, v, m, st) == INVALID_ARG
    assert u8(s, 8, 8, 3, d, 8, 8, v, None, st) == INVALID_ARG
    assert near(s, 4, 8, 8, s + 64, 8, 8, m, st) == INVALID_ARG
    assert near(s, 3, 8, 8, d, 8, 8, m, st) == INVALID_ARG
    assert near(s, 4, 8, 8, d + 2, 8, 8, m, st) == INVALID_ARG
    assert near(s, 2, 8, 8193, d, 8, 8, m, st) == INVALID_ARG
    assert near(None, 2, 8, 8, d, 8, 8, m, st) == INVALID_ARG
    assert near(s, 2, 8, 8, d, 8, 8, None, st) == INVALID_ARG
    torch.cuda.synchronize()
    assert bool((dst == GUARD).all()) and bool((mask == GUARD).all()) and not bool(src.any())
    assert C.sizeof(_lib.BrushUndistort) == 64


def test_graph_replay_gives_the_same_bits(dev):
    import torch

    from brush_amd.undistort import remap_depth, remap_image

    w, h, ow, oh = 257, 65, 300, 40
    m = R.case_map(w, h, ow, oh, R.PARAMS["full_opencv_rational"])
    img = torch.from_numpy(R.pattern_image(w, h, 3, 2)).to(dev)
    dep = torch.from_numpy(_depth_map(w, h, np.float32, 2)).to(dev)
    eager = remap_image(img, _struct(m), (ow, oh), True) + (remap_depth(dep, _struct(m), (ow, oh)),)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = remap_image(img, _struct(m), (ow, oh), True) + (remap_depth(dep, _struct(m), (ow, oh)),)
    for _ in range(2):
        for t in captured:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert np.array_equal(_np(eager[0]), R.undistort_u8_ref(_np(img), m, ow, oh)[0])


# ---------------------------------------------------------------------------- 7. command lines
def test_command_lines_undistort_unless_told_not_to(dev, tree, tmp_path, capsys):
    from brush_amd import eval as E
    from brush_amd import fit_scale
    from brush_amd import dataset as D
    from brush_amd import train_loop as T

    root = tree[0]
    ply = str(tmp_path / "out.ply")
    common = [root, "--steps", "3", "--init-count", "300", "--sh-degree", "1", "--eval-split-every", "2"]
    assert T.main(common + ["--export", ply]) == 0
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("undistorting")]
    d = D.read_colmap(root).train.views[1].distortion
    assert len(lines) == 1 and "undistorting 3 views" in lines[0]
    assert f"SIMPLE_RADIAL 48x36 scale {fit_scale(d):.6f}" in lines[0] and "OPENCV 48x36 scale" in lines[0]
    assert T.main(common + ["--no-undistort"]) == 0
    assert "undistorting" not in capsys.readouterr().out
    assert E.main([ply, root, "--eval-split-every", "2"]) == 0
    out = capsys.readouterr().out
    assert sum(1 for ln in out.splitlines() if ln.startswith("undistorting")) == 1 and "mean (2 views)" in out
    assert E.main([ply, root, "--eval-split-every", "2", "--no-undistort"]) == 0
    assert "undistorting" not in capsys.readouterr().out
    assert math.isfinite(fit_scale(d))
