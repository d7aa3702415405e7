"""Undistortion of COLMAP views: every view resampled once, on the device, into the pinhole camera the rasterizer assumes.

COLMAP's default camera models for real captures (SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV) carry lens distortion; the
render, loss and backward kernels know pinhole cameras only.  The fix sits in the data path, as COLMAP's
`image_undistorter` does it and as 3DGS and gsplat expect it to have been done: nothing above the images changes.

    Distortion          a view's source camera: model, size, focal, principal point, k1..k6, p1, p2
                        (`Distortion.from_colmap`; `read_colmap` fills `SceneView.distortion` with it)
    fit_scale           the zoom of the output camera at which no output pixel falls outside the source (crop to valid:
                        COLMAP's blank_pixels = 0)
    undistort_image     uint8 [h,w,3|4] images: bilinear in Q8 fixed point, defined exactly (include/brush_hip.h:
                        brush_undistort_u8; brush_amd/csrc/undistort.hip)
    undistort_depth     uint16 / float32 [h,w] depth maps: the nearest element (brush_undistort_nearest), so a "no
                        measurement" zero never blends into its neighbours
    undistorted_camera  the pinhole camera of the resampled view
    undistort_dataset   all of it for a Dataset

Supported: the four models above, sides of at most 8192 pixels.  The fisheye, FOV and thin-prism models are read, and
raise a ValueError naming the model when a view that has one (with a non-zero coefficient) is used here.
"""
from __future__ import annotations

import dataclasses
import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .camera import Camera, focal_to_fov

MAX_SIDE = 8192
SUPPORTED_MODELS = ("SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV")
_COEFFS = ("k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2")
# where a model's parameters behind focal and principal point go (COLMAP's order per model)
_COLMAP_COEFFS = {"SIMPLE_RADIAL": ("k1",), "RADIAL": ("k1", "k2"), "OPENCV": ("k1", "k2", "p1", "p2"),
                  "FULL_OPENCV": ("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")}


@dataclass(frozen=True)
class Distortion:
    """The distorted camera of a view: `model` (COLMAP's name), the source image's size, focal and principal point in
    its pixels (pixel centres at +0.5) and the coefficients of OpenCV's rational model; a model's missing ones are 0.
    For a model this module does not support the coefficient fields hold the model's own parameters in file order: they
    only say that the camera is distorted, and every use raises."""
    model: str
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    k1: float = 0.0
    k2: float = 0.0
    k3: float = 0.0
    k4: float = 0.0
    k5: float = 0.0
    k6: float = 0.0
    p1: float = 0.0
    p2: float = 0.0

    @classmethod
    def from_colmap(cls, cam, img_w: int, img_h: int) -> Optional["Distortion"]:
        """The distortion of COLMAP camera `cam` for an image loaded at img_w x img_h (`max_resolution` may have shrunk
        it: focal and principal point scale by img_w / cam.width and img_h / cam.height, the coefficients are
        dimensionless).  None for SIMPLE_PINHOLE / PINHOLE and when every coefficient is zero."""
        from .dataset import _COLMAP_MODELS

        name, _, fy_i, cx_i, cy_i = _COLMAP_MODELS[cam.model]
        rest = [float(p) for p in cam.params[cy_i + 1:]]
        if not any(rest):
            return None
        img_w, img_h = int(img_w) or int(cam.width), int(img_h) or int(cam.height)
        sx, sy = img_w / float(cam.width), img_h / float(cam.height)
        names = _COLMAP_COEFFS.get(name, _COEFFS)
        return cls(name, img_w, img_h, float(cam.params[0]) * sx, float(cam.params[fy_i]) * sy,
                   float(cam.params[cx_i]) * sx, float(cam.params[cy_i]) * sy, **dict(zip(names, rest)))

    def check_supported(self) -> None:
        if self.model not in SUPPORTED_MODELS:
            raise ValueError(f"camera model {self.model} cannot be undistorted here (supported: "
                             f"{', '.join(SUPPORTED_MODELS)}); undistort the dataset with COLMAP's image_undistorter")
        if not (1 <= self.width <= MAX_SIDE and 1 <= self.height <= MAX_SIDE):
            raise ValueError(f"a distorted view must be 1..{MAX_SIDE} pixels on each side, got "
                             f"{(self.width, self.height)}")

    def distort(self, x, y):
        """The model in float64: normalised pinhole coordinates -> source pixel coordinates (centres at +0.5)."""
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        r2 = x * x + y * y
        rad = (1 + r2 * (self.k1 + r2 * (self.k2 + r2 * self.k3))) / (1 + r2 * (self.k4 + r2 * (self.k5 + r2 * self.k6)))
        a = x * y
        xd = x * rad + (2 * self.p1 * a + self.p2 * (r2 + 2 * x * x))
        yd = y * rad + (self.p1 * (r2 + 2 * y * y) + 2 * self.p2 * a)
        return self.fx * xd + self.cx, self.fy * yd + self.cy


def _border_inside(d: Distortion, s: float, margin: float) -> bool:
    w, h = d.width, d.height
    xs, ys = np.arange(w) + 0.5, np.arange(h) + 0.5
    px = np.concatenate([xs, xs, np.full(h, 0.5), np.full(h, w - 0.5)])
    py = np.concatenate([np.full(w, 0.5), np.full(w, h - 0.5), ys, ys])
    with np.errstate(all="ignore"):
        u, v = d.distort((px - d.cx) / (s * d.fx), (py - d.cy) / (s * d.fy))
        ok = (u >= 0.5 + margin) & (u <= w - 0.5 - margin) & (v >= 0.5 + margin) & (v <= h - 0.5 - margin)
    return bool(ok.all())


@functools.lru_cache(maxsize=256)
def _fit_scale(d: Distortion, margin: float) -> float:
    d.check_supported()
    lo, hi = 0.25, 4.0
    if not _border_inside(d, hi, margin):
        raise ValueError(f"{d.model} {d.width}x{d.height}: no output focal within [1/4, 4] of the source's keeps the "
                         "whole output inside the source image")
    if _border_inside(d, lo, margin):
        return lo
    while hi - lo > 1e-6 * hi:
        mid = 0.5 * (lo + hi)
        if _border_inside(d, mid, margin):
            hi = mid
        else:
            lo = mid
    return hi


def fit_scale(d: Distortion, margin: float = 1.0 / 64.0) -> float:
    """The scale s of the output camera (the source's size and principal point, focal (s fx, s fy)): the smallest s in
    [1/4, 4] at which every border pixel centre of the output maps inside [0.5 + margin, w - 0.5 - margin] x
    [0.5 + margin, h - 0.5 - margin] of the source, i.e. no output pixel is blank (COLMAP's blank_pixels = 0).  Float64,
    bisected to a relative width of 1e-6; the margin keeps float32 rounding from invalidating a border pixel.
    ValueError when no s in the range does it."""
    return _fit_scale(d, float(margin))


def undistort_map(d: Distortion, scale: float, out_size: Optional[Tuple[int, int]] = None,
                  out_center: Optional[Tuple[float, float]] = None) -> "_lib.BrushUndistort":
    """The BrushUndistort of `d` seen through the output camera of `scale`: focal (scale fx, scale fy), the source's
    principal point (or `out_center`), inverse focal divided in float32."""
    d.check_supported()
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError(f"the scale must be positive, got {scale!r}")
    ocx, ocy = (d.cx, d.cy) if out_center is None else out_center
    m = _lib.BrushUndistort()
    m.fx, m.fy, m.cx, m.cy = d.fx, d.fy, d.cx, d.cy
    m.iofx = float(np.float32(1.0) / np.float32(scale * d.fx))
    m.iofy = float(np.float32(1.0) / np.float32(scale * d.fy))
    m.ocx, m.ocy = ocx, ocy
    for name in _COEFFS:
        setattr(m, name, getattr(d, name))
    return m


def _out_size(d: Distortion, size) -> Tuple[int, int]:
    ow, oh = (d.width, d.height) if size is None else (int(size[0]), int(size[1]))
    if not (1 <= ow <= MAX_SIDE and 1 <= oh <= MAX_SIDE):
        raise ValueError(f"the output must be 1..{MAX_SIDE} pixels on each side, got {(ow, oh)}")
    return ow, oh


def remap_image(image: torch.Tensor, m, size: Tuple[int, int], return_valid: bool = False):
    """brush_undistort_u8 with the map `m` (a BrushUndistort) to `size` = (ow, oh): a new uint8 [oh,ow,c] tensor, and
    the uint8 [oh,ow] validity mask when asked for.  Runs on the current stream; does not synchronise."""
    assert image.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    if image.dim() != 3 or image.dtype != torch.uint8 or image.shape[2] not in (3, 4):
        raise ValueError(f"image must be a uint8 [h,w,3|4] tensor, got {image.dtype} {tuple(image.shape)}")
    h, w, c = (int(x) for x in image.shape)
    ow, oh = int(size[0]), int(size[1])
    image = image.contiguous()
    out = torch.empty((oh, ow, c), dtype=torch.uint8, device=image.device)
    valid = torch.empty((oh, ow), dtype=torch.uint8, device=image.device) if return_valid else None
    with torch.cuda.device(image.device):
        _lib.check(_lib.lib().brush_undistort_u8(image.data_ptr(), w, h, c, out.data_ptr(), ow, oh,
                                                 valid.data_ptr() if return_valid else None, m,
                                                 _lib.current_stream(image.device)),
                   "brush_undistort_u8")
    return (out, valid) if return_valid else out


def remap_depth(t: torch.Tensor, m, size: Tuple[int, int]) -> torch.Tensor:
    """brush_undistort_nearest with the map `m` to `size` = (ow, oh): a new [oh,ow] tensor of t's dtype."""
    assert t.is_cuda, "brush_amd has no CPU path: tensors must live on the GPU"
    if t.dim() != 2 or t.dtype not in (torch.uint16, torch.float32):
        raise ValueError(f"t must be a uint16 or float32 [h,w] tensor, got {t.dtype} {tuple(t.shape)}")
    h, w = int(t.shape[0]), int(t.shape[1])
    ow, oh = int(size[0]), int(size[1])
    t = t.contiguous()
    out = torch.empty((oh, ow), dtype=t.dtype, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.lib().brush_undistort_nearest(t.data_ptr(), t.element_size(), w, h, out.data_ptr(), ow, oh, m,
                                                      _lib.current_stream(t.device)),
                   "brush_undistort_nearest")
    return out


def _check_source(shape_hw, d: Distortion, what: str) -> None:
    if (int(shape_hw[0]), int(shape_hw[1])) != (d.height, d.width):
        raise ValueError(f"{what} is {int(shape_hw[1])}x{int(shape_hw[0])}, its distortion describes a "
                         f"{d.width}x{d.height} image")


def undistort_image(image: torch.Tensor, d: Distortion, scale: Optional[float] = None, return_valid: bool = False):
    """`image`, a uint8 [h,w,3|4] device tensor taken through the camera `d`, resampled into the pinhole camera of
    `scale` (None: fit_scale(d)) at the same size: a new uint8 [h,w,c] tensor, with `return_valid` also the uint8 [h,w]
    mask of the pixels whose source lies inside the image (the others are 0).  Runs on the current stream; does not
    synchronise."""
    m = undistort_map(d, fit_scale(d) if scale is None else float(scale))
    if image.dim() == 3:
        _check_source(image.shape[:2], d, "the image")
    return remap_image(image, m, _out_size(d, None), return_valid)


def undistort_depth(t: torch.Tensor, d: Distortion, scale: Optional[float] = None) -> torch.Tensor:
    """`t`, a uint16 or float32 [h,w] device tensor (a depth map taken through `d`), resampled like undistort_image but
    by taking the nearest element, moved as bits; a pixel whose source lies outside is 0, "no measurement".  Runs on the
    current stream; does not synchronise."""
    m = undistort_map(d, fit_scale(d) if scale is None else float(scale))
    if t.dim() == 2:
        _check_source(t.shape, d, "the depth map")
    return remap_depth(t, m, _out_size(d, None))


def undistorted_camera(camera: Camera, d: Distortion, scale: float) -> Camera:
    """The pinhole camera of a view undistorted at `scale`: the pose and center_uv of `camera`, the field of view of
    the focal (scale fx, scale fy) on the source's size."""
    d.check_supported()
    return Camera(camera.position, camera.rotation, focal_to_fov(scale * d.fx, d.width),
                  focal_to_fov(scale * d.fy, d.height), camera.center_uv)


def dataset_distortions(dataset) -> list:
    """The distinct Distortions of the dataset's views, in order of first appearance."""
    seen = []
    for scene in (dataset.train, dataset.eval):
        for v in (scene.views if scene is not None else ()):
            d = getattr(v, "distortion", None)
            if d is not None and d not in seen:
                seen.append(d)
    return seen


def undistort_dataset(dataset, device=None, scale: Optional[float] = None):
    """A new Dataset in which every view that has a `distortion` carries its image, depth map and loss mask resampled
    on the device (undistort_image / undistort_depth at `scale`, None: fit_scale per camera; the mask goes through the
    depth maps' nearest remap, so a pixel whose source lies outside the frame is 0, not kept), the undistorted camera and
    `distortion=None`; the other views are shared unchanged.  Plans are kept per (Distortion, scale): COLMAP datasets
    usually share one camera.  The first view of each plan also fetches the validity mask, which is checked once:
    ValueError if any pixel is invalid (the distortion folds inside the frame, or `scale` is too small).

    The results are copied back to the host on purpose: a load-time cost of one round trip per view that keeps every
    consumer of `dataset.*.views` as it is (SceneLoader's upload, pose and exposure tables, camera export, eval, depth
    maps)."""
    from .dataset import Dataset, Scene

    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    plans = {}

    def convert(view):
        d = getattr(view, "distortion", None)
        if d is None:
            return view
        s = fit_scale(d) if scale is None else float(scale)
        first = (d, s) not in plans
        if first:
            plans[(d, s)] = undistort_map(d, s)
        m, size = plans[(d, s)], (d.width, d.height)
        _check_source(view.image.shape[:2], d, f"{view.name}: the image")
        src = torch.from_numpy(np.array(view.image, copy=True, order="C")).to(dev)
        if first:
            out, valid = remap_image(src, m, size, True)
            if not bool(valid.all()):
                raise ValueError(f"{view.name}: at scale {s:.6f} {int((valid == 0).sum())} pixels of the undistorted "
                                 f"{d.model} view have no source pixel: the distortion folds inside the frame")
        else:
            out = remap_image(src, m, size)
        depth = view.depth
        if depth is not None:
            _check_source(depth.shape, d, f"{view.name}: the depth map")
            depth = remap_depth(torch.from_numpy(np.array(depth, copy=True, order="C")).to(dev), m, size).cpu().numpy()
        mask = getattr(view, "mask", None)
        if mask is not None:  # the nearest remap of the depth maps, on the mask as uint16: a pixel without a source is 0
            _check_source(mask.shape, d, f"{view.name}: the mask")
            wide = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint16)).to(dev)
            mask = remap_depth(wide, m, size).cpu().numpy().astype(np.uint8)
        return dataclasses.replace(view, image=out.cpu().numpy(), depth=depth, mask=mask,
                                   camera=undistorted_camera(view.camera, d, s), distortion=None)

    train = Scene([convert(v) for v in dataset.train.views])
    evals = Scene([convert(v) for v in dataset.eval.views]) if dataset.eval is not None else None
    return Dataset(train, evals)


def undistort_for_cli(dataset, enabled: bool = True, device=None):
    """What both command lines do after loading: `dataset` itself when no view carries a distortion or `enabled` is
    False (--no-undistort), else undistort_dataset(dataset) behind one line that names every camera's fitted scale."""
    ds = dataset_distortions(dataset) if enabled else []
    if not ds:
        return dataset
    n = sum(1 for scene in (dataset.train, dataset.eval) if scene is not None for v in scene.views
            if v.distortion is not None)
    cams = ", ".join(f"{d.model} {d.width}x{d.height} scale {fit_scale(d):.6f}" for d in ds)
    print(f"undistorting {n} views on the device ({cams}); --no-undistort keeps them as loaded", flush=True)
    return undistort_dataset(dataset, device)
