"""Depth supervision without a GPU: the numpy restatement (tests/depth_loss_ref64.py) against float64 autograd, the
validity rules pixel by pixel, the argument checks of the entry points, the dataset readers' depth maps and the Python
surface (trainer argument checks, command-line flags)."""
import ctypes as C
import io
import json
import os

import numpy as np
import pytest

from tests import depth_loss_ref64 as DR
from tests import eval_data as ED

F = np.float32
U = 2.0 ** -24


# ---------------------------------------------------------------------------- 1. the restatement against autograd
def _smooth_case(mode, gt_dtype, seed=3, w=37, h=29):
    scale, offset = (0.00105, -0.05) if gt_dtype == np.uint16 else (1.7, -0.03)
    if gt_dtype == np.uint16 and mode == "disparity":
        scale, offset = 1e-4, -0.001
    return DR.make_case(w, h, gt_dtype, mode, seed, scale, offset), scale, offset


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("gt_dtype", [np.uint16, np.float32])
def test_restatement_equals_float64_autograd(mode, gt_dtype):
    import torch

    case, scale, offset = _smooth_case(mode, gt_dtype)
    kw = dict(weight=0.7, scale=scale, offset=offset, alpha_min=case["alpha_min"], mode=mode)
    r64 = DR.reference_f64(case["alpha"], case["D"], case["raw"], **kw)
    r32 = DR.reference_f32(case["alpha"], case["D"], case["raw"], **kw)
    assert np.array_equal(r64["valid"], r32["valid"])
    frac = r64["valid"].mean()
    assert 0.25 <= frac <= 0.75, frac
    # float64 autograd of the same formula on the valid pixels (fixed mask: validity is piecewise constant)
    a = torch.tensor(case["alpha"].astype(np.float64), requires_grad=True)
    D = torch.tensor(case["D"].astype(np.float64), requires_grad=True)
    with np.errstate(invalid="ignore"):
        t = torch.tensor(np.where(r64["valid"], case["raw"].astype(np.float64) * float(F(scale)) + float(F(offset)), 1.0))
    m = torch.tensor(r64["valid"])
    safe_a, safe_D = torch.where(m, a, torch.ones_like(a)), torch.where(m, D, torch.ones_like(D))
    r = (safe_D / safe_a - t) if mode == "depth" else (safe_a / safe_D - t)
    loss = r64["c"] * torch.where(m, r.abs(), torch.zeros_like(r)).sum()
    loss.backward()
    assert float(loss.detach()) == pytest.approx(r64["loss"], rel=1e-13)
    # away from r = 0 (make_case keeps |r| above 2 % of the rendered value) the gradients are those of the restatement
    assert np.abs(r64["abs_r"][r64["valid"]]).min() > 1e-4
    for got, want in ((D.grad.numpy(), r64["v_depth"]), (a.grad.numpy(), r64["v_alpha"])):
        assert np.allclose(got, want, rtol=1e-13, atol=0.0)
        assert not got[~r64["valid"]].any()
    # the f32 form: at most three correctly rounded f32 operations on top of the same f32 c
    for k in ("v_depth", "v_alpha"):
        err = np.abs(r32[k].astype(np.float64) - r64[k])
        assert (err <= 4 * U * np.abs(r64[k])).all(), (k, float((err / np.abs(r64[k]).clip(1e-300)).max() / U))
        assert r32[k][r32["valid"]].all()  # every valid pixel has a gradient
    assert DR.loss_f64(r32) == pytest.approx(r64["loss"], rel=4 * U)


def test_sign_of_zero_is_zero():
    r = DR.reference_f32(F([[0.5]]), F([[1.0]]), F([[2.0]]), alpha_min=0.5, mode="depth")  # d = 2 = t
    assert r["valid"].all() and r["v_depth"][0, 0] == 0 and r["v_alpha"][0, 0] == 0 and r["abs_r"][0, 0] == 0


# ---------------------------------------------------------------------------- 2. validity rules, one pixel each
def _one(alpha, D, raw, **kw):
    raw = np.asarray([[raw]], dtype=kw.pop("dtype", np.float32))
    kw.setdefault("alpha_min", 0.5)
    return DR.reference_f32(F([[alpha]]), F([[D]]), raw, **kw)


@pytest.mark.parametrize("mode", DR.MODES)
def test_validity_rules_one_directed_pixel_each(mode):
    ok = _one(0.8, 1.6, 3.0, mode=mode)
    assert ok["valid"][0, 0] and ok["v_depth"][0, 0] != 0 and ok["v_alpha"][0, 0] != 0
    assert _one(0.8, 1.6, 3000, dtype=np.uint16, scale=0.001, mode=mode)["valid"][0, 0]
    invalid = [
        _one(0.8, 1.6, 0, dtype=np.uint16, mode=mode),                    # u16: raw = 0 is "no measurement"
        _one(0.8, 1.6, 0.0, mode=mode),                                   # f32: 0
        _one(0.8, 1.6, np.nan, mode=mode),
        _one(0.8, 1.6, np.inf, mode=mode),
        _one(0.8, 1.6, -2.0, mode=mode),
        _one(0.8, 1.6, 3.0, offset=-3.0, mode=mode),                      # t = 0 through the offset
        _one(0.8, 1.6, 3.0, offset=-4.0, mode=mode),                      # t < 0
        _one(0.8, 1.6, 40, dtype=np.uint16, scale=0.001, offset=-0.05, mode=mode),
        _one(np.nextafter(F(0.5), F(0)), 1.6, 3.0, mode=mode),            # alpha just below alpha_min
        _one(0.8, 0.0, 3.0, mode=mode),                                   # D = 0
        _one(0.8, -1.0, 3.0, mode=mode),
    ]
    for k, r in enumerate(invalid):
        assert not r["valid"][0, 0], k
        assert r["v_depth"][0, 0] == 0 and r["v_alpha"][0, 0] == 0 and DR.loss_f64(r) == 0.0, k
    assert _one(0.5, 1.6, 3.0, mode=mode)["valid"][0, 0]                  # alpha exactly at alpha_min counts


# ---------------------------------------------------------------------------- 3. entry points validate without a GPU
def test_depth_loss_entry_points_validate_arguments_without_gpu():
    """Every check runs before the first GPU call: bad arguments come back as BRUSH_ERR_INVALID_ARG (-1) or
    BRUSH_ERR_WORKSPACE_SMALL (-2) on a machine without a device (the pointers are never dereferenced)."""
    from brush_amd import _lib as L

    l = L.lib()
    n = C.c_size_t()
    assert l.brush_depth_loss_workspace_size(0, 4, C.byref(n)) == -1
    assert l.brush_depth_loss_workspace_size(4, 0, C.byref(n)) == -1
    assert l.brush_depth_loss_workspace_size(1 << 14, 1 << 14, C.byref(n)) == -1   # 2^28 pixels
    assert l.brush_depth_loss_workspace_size(4, 4, None) == -1
    assert l.brush_depth_loss_workspace_size(1, 1, C.byref(n)) == 0 and n.value >= 16 and n.value % 8 == 0
    assert l.brush_depth_loss_workspace_size(1920, 1080, C.byref(n)) == 0 and n.value <= 16 * 1024
    big = n.value
    assert l.brush_depth_loss_workspace_size((1 << 14) - 1, 1 << 14, C.byref(n)) == 0 and n.value == big  # capped grid

    good = dict(pred=0x1000, depth=0x2000, target=0x3000, v_depth=0x4000, v_pred=0x5000, stats=0x6000, accum=0x7000,
                ws=0x8000, ws_bytes=1 << 20, w=8, h=8)

    def call(cfg=None, **kw):
        a = dict(good, **kw)
        cfg = L.BrushDepthLoss(1.0, 1.0, 0.0, 0.5, L.DEPTH_LOSS_DEPTH, L.DEPTH_GT_F32) if cfg is None else cfg
        return l.brush_depth_loss(a["pred"], a["depth"], a["target"], C.byref(cfg) if cfg else None, a["w"], a["h"],
                                  a["v_depth"], a["v_pred"], a["stats"], a["accum"], a["ws"], a["ws_bytes"], None)

    for k in ("pred", "depth", "target", "stats", "ws"):
        assert call(**{k: None}) == -1, k
    assert l.brush_depth_loss(0x1000, 0x2000, 0x3000, None, 8, 8, None, None, 0x6000, None, 0x8000, 1 << 20, None) == -1
    assert call(w=0) == -1 and call(h=0) == -1 and call(w=1 << 14, h=1 << 14) == -1
    assert call(pred=0x1004) == -1 and call(v_pred=0x5008) == -1        # images: 16-byte aligned
    assert call(depth=0x2002) == -1 and call(v_depth=0x4001) == -1 and call(stats=0x6002) == -1
    assert call(accum=0x7002) == -1 and call(ws=0x8004) == -1
    assert call(target=0x3002) == -1                                    # f32 target: 4 bytes
    assert call(v_pred=good["pred"]) == -1                              # the gradient image is not the render
    assert call(ws_bytes=8) == -2
    mk = lambda **kw: L.BrushDepthLoss(**{**dict(weight=1.0, scale=1.0, offset=0.0, alpha_min=0.5, mode=0, gt_dtype=1),
                                          **kw})
    assert call(mk(alpha_min=0.0)) == -1 and call(mk(alpha_min=-0.5)) == -1 and call(mk(alpha_min=float("nan"))) == -1
    assert call(mk(mode=2)) == -1 and call(mk(gt_dtype=2)) == -1
    assert call(mk(gt_dtype=L.DEPTH_GT_U16), target=0x3001) == -1       # u16 target: 2 bytes
    assert "brush_depth_loss" in L.SYMBOL_NAMES and "brush_depth_loss_workspace_size" in L.SYMBOL_NAMES


def test_python_surface_checks_arguments_without_gpu():
    import torch

    import brush_amd
    from brush_amd import depth_loss as fn
    from brush_amd.depth_loss import depth_loss_into, workspace_bytes

    assert callable(brush_amd.depth_loss) and fn is brush_amd.depth_loss and callable(brush_amd.depth_loss_into)
    assert workspace_bytes(1920, 1080) <= 16 * 1024
    with pytest.raises(AssertionError, match="no CPU path"):
        depth_loss_into(torch.zeros((4, 4, 4)), torch.zeros((4, 4)), torch.zeros((4, 4)), None)


# ---------------------------------------------------------------------------- 4. readers
def _png16(a):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a, dtype=np.uint16)).save(buf, format="PNG")
    return buf.getvalue()


def _depth_maps(w, h):
    rng = np.random.default_rng(w * 100 + h)
    d16 = rng.integers(1, 65535, (h, w)).astype(np.uint16)
    d16[rng.random((h, w)) < 0.2] = 0
    d32 = rng.uniform(0.5, 9.0, (h, w)).astype(np.float32)
    d32[0, 0] = 0.0
    return d16, d32


def _write_nerf(root, w, h, unit=None, depth_size=None):
    """Three frames: a 16-bit PNG depth map, a .npy one, none."""
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    os.makedirs(os.path.join(root, "depth"), exist_ok=True)
    dw, dh = depth_size or (w, h)
    d16, d32 = _depth_maps(dw, dh)
    frames = []
    for i in range(3):
        with open(os.path.join(root, "train", f"r_{i}.png"), "wb") as f:
            f.write(ED.png_bytes(ED.noise_image(w, h, 3, 7 + i)))
        fr = {"file_path": f"./train/r_{i}", "transform_matrix": ED.look_at_gl((3.0, 0.5 * i, 1.0)).tolist()}
        if i == 0:
            fr["depth_file_path"] = "depth/r_0.png"
            with open(os.path.join(root, "depth", "r_0.png"), "wb") as f:
                f.write(_png16(d16))
        elif i == 1:
            fr["depth_file_path"] = "./depth/r_1.npy"
            np.save(os.path.join(root, "depth", "r_1.npy"), d32)
        frames.append(fr)
    doc = {"camera_angle_x": 0.69, "frames": frames}
    if unit is not None:
        doc["depth_unit_scale_factor"] = unit
    with open(os.path.join(root, "transforms_train.json"), "w") as f:
        json.dump(doc, f)
    return d16, d32


def test_nerf_reader_keeps_dtype_scale_and_none(tmp_path):
    from brush_amd import dataset as D

    d16, d32 = _write_nerf(str(tmp_path / "a"), 24, 16)
    views = D.read_nerf_synthetic(str(tmp_path / "a")).train.views
    assert views[0].depth.dtype == np.uint16 and np.array_equal(views[0].depth, d16)      # exact round trip
    assert views[0].depth_scale == 0.001 and views[0].depth_offset == 0.0                 # 16-bit default: millimetres
    assert views[1].depth.dtype == np.float32 and np.array_equal(views[1].depth, d32) and views[1].depth_scale == 1.0
    assert views[2].depth is None and views[2].depth_scale == 1.0 and views[2].depth_offset == 0.0
    assert views[0].depth.shape == views[0].image.shape[:2]
    _write_nerf(str(tmp_path / "b"), 24, 16, unit=0.00025)
    views = D.read_nerf_synthetic(str(tmp_path / "b")).train.views
    assert views[0].depth_scale == 0.00025 and views[1].depth_scale == 0.00025 and views[2].depth is None
    # positional construction is unchanged
    v = D.SceneView("n", views[0].camera, views[0].image)
    assert v.depth is None and v.depth_scale == 1.0 and v.depth_offset == 0.0


def test_nerf_reader_resizes_depth_with_nearest_neighbour(tmp_path):
    from brush_amd import dataset as D

    d16, d32 = _write_nerf(str(tmp_path / "a"), 48, 32)
    views = D.read_nerf_synthetic(str(tmp_path / "a"), max_resolution=24).train.views
    assert views[0].image.shape[:2] == (16, 24)
    for v, src in ((views[0], d16), (views[1], d32)):
        assert v.depth.shape == (16, 24) and v.depth.dtype == src.dtype
        assert np.array_equal(v.depth, src[1::2, 1::2])        # the source pixel under each output pixel's centre
        assert np.isin(v.depth, src).all()                      # nothing blended: zeros stay zeros, values stay values
    # a depth map already at the final size is taken as it is
    d16s, _ = _write_nerf(str(tmp_path / "b"), 48, 32, depth_size=(24, 16))
    views = D.read_nerf_synthetic(str(tmp_path / "b"), max_resolution=24).train.views
    assert np.array_equal(views[0].depth, d16s)
    assert np.array_equal(D.resize_nearest(np.arange(12).reshape(3, 4), (3, 4)), np.arange(12).reshape(3, 4))


def test_depth_size_mismatch_raises_and_names_the_view(tmp_path):
    from brush_amd import dataset as D

    _write_nerf(str(tmp_path / "a"), 24, 16, depth_size=(20, 16))
    with pytest.raises(ValueError, match=r"r_0\.png.*20x16.*24x16"):
        D.read_nerf_synthetic(str(tmp_path / "a"))


def _write_colmap(root, w, h, params=None):
    os.makedirs(os.path.join(root, "sparse", "0"))
    os.makedirs(os.path.join(root, "images"))
    os.makedirs(os.path.join(root, "depths"))
    d16, d32 = _depth_maps(w, h)
    with open(os.path.join(root, "sparse", "0", "cameras.txt"), "w") as f:
        f.write(f"1 PINHOLE {w} {h} 30.0 30.0 {w / 2} {h / 2}\n")
    with open(os.path.join(root, "sparse", "0", "images.txt"), "w") as f:
        for i, name in enumerate(("a.png", "b.png", "c.png")):
            f.write(f"{i + 1} 1 0 0 0 0.1 0.2 {3 + i} 1 {name}\n\n")
            with open(os.path.join(root, "images", name), "wb") as g:
                g.write(ED.png_bytes(ED.noise_image(w, h, 3, 20 + i)))
    with open(os.path.join(root, "depths", "a.png"), "wb") as f:
        f.write(_png16(d16))
    np.save(os.path.join(root, "depths", "b.npy"), d32)
    if params is not None:
        with open(os.path.join(root, "sparse", "0", "depth_params.json"), "w") as f:
            json.dump(params, f)
    return d16, d32


def test_colmap_reader_depths_and_depth_params(tmp_path):
    from brush_amd import dataset as D

    d16, d32 = _write_colmap(str(tmp_path / "a"), 20, 12)
    views = D.read_colmap(str(tmp_path / "a")).train.views
    assert [os.path.basename(v.name) for v in views] == ["a.png", "b.png", "c.png"]
    assert views[0].depth.dtype == np.uint16 and np.array_equal(views[0].depth, d16) and views[0].depth_scale == 0.001
    assert views[1].depth.dtype == np.float32 and np.array_equal(views[1].depth, d32) and views[1].depth_scale == 1.0
    assert views[2].depth is None
    _write_colmap(str(tmp_path / "b"), 20, 12, params={"a": {"scale": 0.002, "offset": 0.25}, "b": {"scale": 3.0}})
    views = D.read_colmap(str(tmp_path / "b")).train.views
    assert (views[0].depth_scale, views[0].depth_offset) == (0.002, 0.25)
    assert (views[1].depth_scale, views[1].depth_offset) == (3.0, 0.0)
    assert views[2].depth is None
    views = D.read_colmap(str(tmp_path / "b"), max_resolution=10).train.views
    assert views[0].depth.shape == views[0].image.shape[:2] == (6, 10) and np.array_equal(views[0].depth, d16[1::2, 1::2])
    assert all(v.depth is None for v in D.read_colmap(str(tmp_path / "b"), load_images=False).train.views)
    os.remove(str(tmp_path / "b" / "depths" / "b.npy"))
    np.save(str(tmp_path / "b" / "depths" / "b.npy"), d32[:, :-1])
    with pytest.raises(ValueError, match=r"b\.png"):
        D.read_colmap(str(tmp_path / "b"))


# ---------------------------------------------------------------------------- 5. Python surface
def test_step_rejects_gt_depth_with_exchange():
    """The check runs before any device work: a trainer that was never initialised and no splats are enough."""
    import brush_amd

    tr = brush_amd.SplatTrainer.__new__(brush_amd.SplatTrainer)
    tr.config = brush_amd.TrainConfig(depth_weight=0.1)
    with pytest.raises(ValueError, match="single-view"):
        tr.step(None, None, None, exchange=object(), gt_depth=object())
    with pytest.raises(ValueError, match="single-view"):
        tr.step(None, None, None, grad_sync=lambda b, a: None, gt_depth=object())


def test_config_defaults_and_weight_schedule():
    import brush_amd

    c = brush_amd.TrainConfig()
    assert c.depth_weight == 0.0 and c.depth_weight_final is None and c.depth_mode == "depth"
    assert c.depth_alpha_min == 0.5
    tr = brush_amd.SplatTrainer.__new__(brush_amd.SplatTrainer)
    tr.config = brush_amd.TrainConfig(total_steps=1000, depth_weight=0.2)
    tr.iter = 500
    assert tr._depth_weight() == 0.2                      # no final weight: constant
    tr.config = brush_amd.TrainConfig(total_steps=1000, depth_weight=0.2, depth_weight_final=0.002)
    tr.iter = 0
    assert tr._depth_weight() == 0.2
    tr.iter = 500
    assert abs(tr._depth_weight() - 0.02) < 1e-12         # exponential: the geometric mean half way
    tr.iter = 1000
    assert abs(tr._depth_weight() - 0.002) < 1e-12


def test_cli_flags_parse():
    from brush_amd import eval as EV
    from brush_amd import train_loop as TL

    a = TL.parser().parse_args(["data"])
    assert a.depth_weight == 0.0 and a.depth_weight_final is None and a.depth_mode == "depth"
    a = TL.parser().parse_args(["data", "--depth-weight", "0.3", "--depth-weight-final", "0.01", "--depth-mode",
                                "disparity"])
    assert (a.depth_weight, a.depth_weight_final, a.depth_mode) == (0.3, 0.01, "disparity")
    with pytest.raises(SystemExit):
        TL.parser().parse_args(["data", "--depth-mode", "inverse"])
    e = EV.parser().parse_args(["s.ply", "data"])
    assert e.depth_metrics is False and e.depth_mode == "depth"
    e = EV.parser().parse_args(["s.ply", "data", "--depth-metrics", "--depth-mode", "disparity"])
    assert e.depth_metrics is True and e.depth_mode == "disparity"
